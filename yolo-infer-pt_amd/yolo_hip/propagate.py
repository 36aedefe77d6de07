"""Track propagation: carry a stream's tracks over the frames the detector skips.

Running the network on every N-th frame divides its cost by N, if the frames in between still give
the tracker something measured. On a detector frame `remember` stores, per track the tracker
reports, a 32 x 32 luma template of the box at the box's own scale; on a skipped frame `propagate`
searches each template in the new frame around the track's last place (yh_propagate: a SAD search
over +-radius cells, sub-cell refinement, a gate on the match and on the frame's edge) and returns
the moved boxes as rows in detection format, which feed the unchanged tracker:

  propagate_state  the zeroed state of `streams` streams (their remembered tracks)
  remember         yh_propagate_remember and its host twin: the tracks of a detector frame
  propagate        yh_propagate and its host twin: one skipped frame of every stream of a batch
  Propagated       (dets (B, max_out, 6) f32, ids (B, max_out) i32, sad (B, max_out) i32, counts (B,) i32)
  Propagator       the state, the parameters and the device workspace of a set of streams

    prop = yolo_hip.Propagator(streams, device)
    dets = detector.predict(frames, keep_frames=True)      # a detector frame
    tracks = tracker.update(dets)
    prop.remember(dets.frames, tracks)
    p = prop.propagate(frames)                             # a skipped frame
    tracks = tracker.update(p.dets, p.counts)

The model is a translation per object of at most `radius` cells per frame (a cell is 1/32 of the
box's side); no scale change, and no deformation beyond what the gate tolerates. The template is
only refreshed by `remember`, and the sub-cell fraction is never accumulated, so nothing drifts.
There is no counterpart in the reference; the semantics are those stated in include/yolo_hip.h,
pinned by the numpy restatement in tests/_propagate_cases.py.
"""
from typing import NamedTuple

import torch

from ._call import frame_descs, host_stream_ids, run, tensor
from ._lib import lib

MAX_RADIUS = 16      # YH_PROPAGATE_MAX_RADIUS
MAX_TRACKS = 256     # YH_PROPAGATE_MAX_TRACKS
_HDR, _ENTRY = 16, 1088   # csrc/propagate_host.h: header bytes per stream, bytes per entry
_WHO = "yolo_hip.propagate"


def propagate_state(streams, max_tracks=256, device="cpu"):
    """The empty state of `streams` streams of up to `max_tracks` remembered tracks: (streams,
    16 + 1088 * max_tracks) uint8 zeros. The bytes are opaque, hold no addresses and mean the same
    on host and device."""
    streams, max_tracks = int(streams), int(max_tracks)
    if streams < 0 or not 1 <= max_tracks <= MAX_TRACKS:
        raise ValueError(f"{_WHO}: streams must be >= 0 and max_tracks in [1, {MAX_TRACKS}]")
    per = _HDR + _ENTRY * max_tracks
    if lib().yh_propagate_state_bytes(streams, max_tracks) != streams * per:
        raise RuntimeError(f"{_WHO}: the library's state size differs from propagate_state's")
    return torch.zeros((streams, per), dtype=torch.uint8, device=device)


class Propagated(NamedTuple):
    """Result of `propagate`: dets (B, max_out, 6) f32 = the moved x1, y1, x2, y2, then the
    remembered score and class; ids (B, max_out) i32 the remembered track ids; sad (B, max_out) i32
    the best match's sum of absolute differences over the 1024 template cells; counts (B,) i32.
    Rows beyond a count are 0."""
    dets: torch.Tensor
    ids: torch.Tensor
    sad: torch.Tensor
    counts: torch.Tensor


def _state(state):
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 2 or not state.is_contiguous() \
            or state.shape[1] < _HDR + _ENTRY or (state.shape[1] - _HDR) % _ENTRY:
        raise ValueError(f"{_WHO}: state must be a propagate_state tensor")
    return state.device, state.shape[0], (state.shape[1] - _HDR) // _ENTRY


def remember(frames, tracks, state, stream_ids=None, threads=0):
    """Store the tracks of a detector frame (yh_propagate_remember). frames: the B frames the
    detector saw, as `Detections.frames` holds them; tracks: the `Tracks` the tracker returned for
    them (any tuple of dets (B, max_det, 6), ids (B, max_det), ..., counts (B,)); state: a
    `propagate_state` tensor, changed in place: a stream's rows replace its whole table.
    stream_ids as `propagate`'s. Runs where the state lives; nothing is read on the host."""
    dev, S, mt = _state(state)
    dets, ids, counts = tracks[0], tracks[1], tracks[-1]
    B = len(frames)
    if not isinstance(dets, torch.Tensor) or dets.dim() != 3:
        raise ValueError(f"{_WHO}: tracks.dets must be a (B, max_det, 6) tensor")
    md = dets.shape[1]
    tensor(_WHO, "tracks.dets", dets, (B, md, 6), torch.float32, dev)
    tensor(_WHO, "tracks.ids", ids, (B, md), torch.int32, dev)
    tensor(_WHO, "tracks.counts", counts, (B,), torch.int32, dev)
    if stream_ids is not None:
        tensor(_WHO, "stream_ids", stream_ids, (B,), torch.int32, dev)
    descs, srcs = frame_descs(_WHO, frames, dev, "propagate.remember", "a CPU state needs host frames")
    run(_WHO, "propagate_remember", dev, (descs, B, stream_ids, dets, ids, counts, md, state, S, mt), threads, keep=srcs)
    return state


def propagate(frames, state, radius=8, max_mad=24, stream_ids=None, out=None, threads=0, max_out=None, workspace=None):
    """The remembered tracks of every stream of a batch, found in the stream's current frame
    (yh_propagate).

    frames: B frames (BGR tensors / arrays and `NV12`, mixed). state: a `propagate_state` tensor,
    advanced in place; its device decides where the call runs. radius: the search radius in cells,
    1 .. 16. max_mad: a best match whose mean absolute difference per template cell is above it drops
    the track from the table (an occlusion, a scene cut); negative: no such gate. A track whose moved
    centre leaves the frame is dropped as well. stream_ids (B,) i32 on the state's device or None:
    row b is a frame of stream stream_ids[b] (None: of stream b); distinct; a row whose id is outside
    [0, streams) gets count 0 and touches no state. max_out: rows per batch row (default: the state's
    max_tracks). workspace: a uint8 tensor of yh_propagate_workspace_bytes for the device path (None:
    allocated here).
    -> Propagated; out=(dets, ids, sad, counts) reuses buffers. Every byte is written.

    A cuda state runs the HIP kernels asynchronously on the current stream (host frames are copied
    there first), a CPU state with host frames the host twin (`threads` <= 0: every hardware
    thread); both give the same bytes, state included."""
    dev, S, mt = _state(state)
    B = len(frames)
    max_out = mt if max_out is None else int(max_out)
    descs, srcs = frame_descs(_WHO, frames, dev, "propagate.propagate", "a CPU state needs host frames")
    if stream_ids is not None:
        tensor(_WHO, "stream_ids", stream_ids, (B,), torch.int32, dev)
    if out is None:
        out = Propagated(torch.empty((B, max(max_out, 0), 6), dtype=torch.float32, device=dev),
                         torch.empty((B, max(max_out, 0)), dtype=torch.int32, device=dev),
                         torch.empty((B, max(max_out, 0)), dtype=torch.int32, device=dev),
                         torch.empty((B,), dtype=torch.int32, device=dev))
    else:
        out = Propagated(*out)
        tensor(_WHO, "out dets", out.dets, (B, max_out, 6), torch.float32, dev)
        tensor(_WHO, "out ids", out.ids, (B, max_out), torch.int32, dev)
        tensor(_WHO, "out sad", out.sad, (B, max_out), torch.int32, dev)
        tensor(_WHO, "out counts", out.counts, (B,), torch.int32, dev)
    device_tail = ()
    if dev.type == "cuda":
        need = lib().yh_propagate_workspace_bytes(B, mt)
        if workspace is None:
            workspace = torch.empty((max(need, 4),), dtype=torch.uint8, device=dev)
        else:
            tensor(_WHO, "workspace", workspace, (None,), torch.uint8, dev)
            if workspace.numel() < need:
                raise ValueError(f"{_WHO}: workspace must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
        device_tail = (workspace, workspace.numel())
        srcs.append(workspace)
    args = (descs, B, stream_ids, state, S, mt, int(radius), int(max_mad), max_out, out.dets, out.ids, out.sad, out.counts)
    run(_WHO, "propagate", dev, args, threads, device_tail=device_tail, keep=srcs)
    return out


class Propagator:
    """The remembered tracks of `streams` video streams on one device.

    remember(frames, tracks, stream_ids=None) on the frames the detector ran on, with the tracker's
    `Tracks`; propagate(frames, stream_ids=None) on the frames it skipped returns `Propagated`, whose
    dets and counts go to `Tracker.update`. stream_ids as `Tracker.update`'s: None, a host sequence of
    ints (checked) or an int32 tensor on the device (not checked). reset() forgets every track;
    `state` is the state tensor. The launches of one propagator must run on one stream, frames of a
    stream in order. Nothing here reads a device value on the host."""

    def __init__(self, streams, device, max_tracks=256, radius=8, max_mad=24):
        self.device = torch.device(device)
        self.radius, self.max_mad = int(radius), int(max_mad)
        if not 1 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"yolo_hip.Propagator: radius must be in [1, {MAX_RADIUS}]")
        self.streams, self.max_tracks = int(streams), int(max_tracks)
        self.state = propagate_state(self.streams, self.max_tracks, self.device)
        self.workspace = None
        if self.device.type == "cuda":
            n = lib().yh_propagate_workspace_bytes(32, self.max_tracks)   # a launch's rows: the most a call needs
            self.workspace = torch.empty((n,), dtype=torch.uint8, device=self.device)

    def reset(self):
        self.state.zero_()

    def remember(self, frames, tracks, stream_ids=None, threads=0):
        stream_ids = host_stream_ids("yolo_hip.Propagator", stream_ids, self.streams, len(frames), self.device, "frames")
        remember(frames, tracks, self.state, stream_ids=stream_ids, threads=threads)

    def propagate(self, frames, stream_ids=None, out=None, threads=0):
        stream_ids = host_stream_ids("yolo_hip.Propagator", stream_ids, self.streams, len(frames), self.device, "frames")
        return propagate(frames, self.state, self.radius, self.max_mad, stream_ids=stream_ids, out=out, threads=threads,
                         workspace=self.workspace)
