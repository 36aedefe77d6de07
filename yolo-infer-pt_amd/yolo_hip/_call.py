"""What every handle-free wrapper of a yh_X / yh_X_host twin pair does, written once: the check of
a tensor argument, the call of the device entry point on the current stream or of the host twin,
the walk over a batch of frames, and the rule for stream ids given on the host. Plain functions;
each wrapper keeps its own signature, sizes and `out=` allocation.
"""
import torch

from ._lib import YhFrame, check, lib

Tensor = torch.Tensor


def tensor(who, name, t, shape, dtype, device):
    """t is a contiguous `dtype` tensor of `shape` (None: any length) on `device`, or raise."""
    if not isinstance(t, Tensor):
        raise TypeError(f"{who}: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{who}: {name} is on {t.device}, expected {device}")
    if len(shape) != t.dim() or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        want = tuple("*" if w is None else w for w in shape)
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {want}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _unsupported(who, dev):
    return ValueError(f"{who}: unsupported device {dev}")


_entries = {}   # name -> (yh_<name>, yh_<name>_host, what, what_host), resolved at the first call


def _resolve(name, what):
    what = what or name
    e = _entries[name] = (getattr(lib(), "yh_" + name), getattr(lib(), f"yh_{name}_host"), what, what + "_host")
    return e


def run(who, name, dev, args, threads, *, what=None, device_tail=(), host_tail=(), keep=()):
    """yh_<name>(*args, *device_tail, stream) on the current stream of a cuda `dev`, or
    yh_<name>_host(*args, *host_tail, threads) for the CPU. Tensors among the arguments are passed
    as their addresses (None: a null pointer), taken only once the device is known to be one of the
    two. `what` names the call in a failure's message (default: name); the tensors of `keep` are
    marked as in use on the stream, so that the allocator does not hand them out while the kernels
    are queued."""
    device_fn, host_fn, what, what_host = _entries.get(name) or _resolve(name, what)
    kind = dev.type
    if kind == "cuda":
        if device_tail:
            args = (*args, *device_tail)
        stream = torch.cuda.current_stream(dev)
        c = [v.data_ptr() if isinstance(v, Tensor) else v for v in args]
        with torch.cuda.device(dev):
            check(device_fn(*c, stream.cuda_stream), what)
        for t in keep:
            t.record_stream(stream)
    elif kind == "cpu":
        if host_tail:
            args = (*args, *host_tail)
        c = [v.data_ptr() if isinstance(v, Tensor) else v for v in args]
        check(host_fn(*c, int(threads)), what_host)
    else:
        raise _unsupported(who, dev)


def frame_descs(who, frames, dev, what, host_rule="the CPU needs host frames"):
    """The yh_frame array of a batch of frames - (h, w, 3) uint8 BGR tensors / arrays and `NV12`,
    mixed - and the tensors it points into: -> (descs, srcs). A cuda `dev` gets the frames copied
    there without blocking; the CPU takes host frames only (`host_rule` is its complaint). `what`
    names the caller in the complaint about an image's layout. Keep srcs until the call has been
    made, and on a device until its stream has run it (`run`'s keep)."""
    from .preprocess import NV12, _bgr, _bgr_desc
    if dev.type not in ("cuda", "cpu"):
        raise _unsupported(who, dev)
    srcs, descs = [], (YhFrame * max(1, len(frames)))()
    for k, f in enumerate(frames):
        nv12 = isinstance(f, NV12)
        if not nv12:
            f = _bgr(f, what)
        if dev.type == "cuda":
            f = f.to(dev, non_blocking=True)
        elif f.device != dev:
            raise ValueError(f"{who}: {host_rule}")
        srcs.extend(f.tensors() if nv12 else (f,))
        descs[k] = f._desc() if nv12 else _bgr_desc(f)
    return descs, srcs


def host_stream_ids(who, stream_ids, streams, batch, device, noun):
    """The stream ids of a batch as the kernels take them. A host sequence is checked (distinct, inside
    [0, streams)) and becomes an int32 tensor on `device`; a tensor is passed on unread; None stands
    for row b = stream b, so the batch (`batch` `noun`) must not exceed the streams."""
    if stream_ids is not None and not isinstance(stream_ids, Tensor):
        host = [int(v) for v in stream_ids]
        if len(set(host)) != len(host):
            raise ValueError(f"{who}: stream_ids must be distinct")
        if any(not 0 <= v < streams for v in host):
            raise ValueError(f"{who}: stream_ids must lie in [0, {streams})")
        return torch.tensor(host, dtype=torch.int32).to(device, non_blocking=True)
    if stream_ids is None and batch > streams:
        raise ValueError(f"{who}: a batch of {batch} {noun} for {streams} streams")
    return stream_ids
