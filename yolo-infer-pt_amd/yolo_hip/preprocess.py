"""Eval-mode image preprocessing of the reference's loader (yh_letterbox / _host) and the
video front end (yh_letterbox_frames / _host).

The reference's Dataset (utils/dataset.py:30-90, augment=False) turns a decoded
BGR image into the network input in three steps: load_image's cv2.resize to
int(w r) x int(h r) with r = input_size / max(h, w) (dataset.py:95-103),
resize()'s zero border to a centred square canvas (dataset.py:292-313) and the
HWC -> CHW, BGR -> RGB flip (dataset.py:86-88). `letterbox` runs all three for a
whole batch in one kernel on the device; `letterbox_host` runs the same per-pixel
code on the host (C++). The resize restates OpenCV's INTER_LINEAR 8-bit algorithm
(csrc/preprocess.hip); cv2 is not in this image, so parity against cv2 itself is
unpinned - the tests pin the kernels to the independent numpy restatement in
oracle/preprocess.py and to torch's bilinear resize within one level.

`letterbox_frames` is the same kernel for video: a frame may be BGR or NV12 (`NV12`: the
decoder's Y plane and interleaved half-resolution UV plane, converted tap by tap inside the
resize, include/yolo_hip.h) and the canvas may be a rectangle (`rect_canvas`), so a 16:9 frame
does not pay for the zero rows of a square canvas.

`crop_rois` (yh_crop_rois / _host) is the step after the detector: one fixed-size RGB crop per box,
cut from the full-resolution BGR or NV12 frame with the same resize, for a second-stage model.
"""
from ctypes import byref, c_int, c_void_p
from typing import NamedTuple

import numpy as np
import torch

from ._lib import YH_PIX_BGR, YH_PIX_NV12, YH_YUV_BT601, YH_YUV_BT709, YhFrame, check, lib


def _hw(size):
    """(H, W) of a canvas given as an int (square) or a pair."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError("a canvas is an int or (H, W)")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def geometry(height, width, size):
    """(new_h, new_w, top, left) of the letterbox of an height x width image on a canvas: size x size
    for an int, H x W for size = (H, W)."""
    ch, cw = _hw(size)
    nh, nw, top, left = c_int(), c_int(), c_int(), c_int()
    check(lib().yh_letterbox_geometry2(int(height), int(width), ch, cw, byref(nh), byref(nw), byref(top),
                                       byref(left)), "letterbox_geometry")
    return nh.value, nw.value, top.value, left.value


def rect_canvas(height, width, size=640, stride=32):
    """(H, W) of the smallest canvas of whole `stride`s that holds a height x width frame resized by
    r = size / max(height, width): the resized sides, each rounded up to a multiple of `stride`.
    1080 x 1920 at 640 gives (384, 640)."""
    height, width, size, stride = int(height), int(width), int(size), int(stride)
    if height < 1 or width < 1 or size < 1 or stride < 1:
        raise ValueError("rect_canvas: height, width, size and stride must be positive")
    r = size / max(height, width)
    nh, nw = (int(height * r), int(width * r)) if r != 1 else (height, width)
    return tuple(max(1, -(-s // stride)) * stride for s in (nh, nw))


class NV12:
    """One NV12 frame: y (h, w) and uv (h / 2, w) uint8 tensors or arrays (uv holds interleaved U, V
    at half resolution), h and w even; the last axis contiguous, rows may be strided. matrix: 601 or
    709 (limited range)."""

    def __init__(self, y, uv, matrix=601):
        y, uv = torch.as_tensor(y), torch.as_tensor(uv)
        if y.dtype != torch.uint8 or uv.dtype != torch.uint8 or y.dim() != 2 or uv.dim() != 2:
            raise ValueError("NV12 needs (h, w) and (h / 2, w) uint8 planes")
        h, w = y.shape
        if h < 2 or w < 2 or h % 2 or w % 2 or tuple(uv.shape) != (h // 2, w):
            raise ValueError(f"NV12: planes {tuple(y.shape)} and {tuple(uv.shape)} are not (h, w) and (h / 2, w) "
                             "with even h, w")
        if y.device != uv.device:
            raise ValueError("NV12: the planes are on different devices")
        if matrix not in (601, 709):
            raise ValueError("NV12: matrix must be 601 or 709")
        self.y = y if y.stride(1) == 1 and y.stride(0) >= w else y.contiguous()
        self.uv = uv if uv.stride(1) == 1 and uv.stride(0) >= w else uv.contiguous()
        self.matrix = matrix

    @classmethod
    def from_packed(cls, buf, height, width, matrix=601):
        """From the decoder's single (height * 3 / 2, width) buffer: Y rows, then UV rows (views)."""
        buf = torch.as_tensor(buf)
        height, width = int(height), int(width)
        if height % 2 or buf.dim() != 2 or tuple(buf.shape) != (height * 3 // 2, width):
            raise ValueError(f"NV12.from_packed: expected a ({height} * 3 / 2, {width}) buffer, got {tuple(buf.shape)}")
        return cls(buf[:height], buf[height:], matrix)

    @property
    def height(self):
        return self.y.shape[0]

    @property
    def width(self):
        return self.y.shape[1]

    @property
    def device(self):
        return self.y.device

    def to(self, device, non_blocking=False):
        return NV12(self.y.to(device, non_blocking=non_blocking), self.uv.to(device, non_blocking=non_blocking),
                    self.matrix)

    def tensors(self):
        return (self.y, self.uv)

    def _desc(self):
        return YhFrame(self.y.data_ptr(), self.uv.data_ptr(), self.height, self.width, self.y.stride(0),
                       self.uv.stride(0), YH_PIX_NV12, YH_YUV_BT709 if self.matrix == 709 else YH_YUV_BT601)


def _bgr(image, what):
    """(h, w, 3) uint8 tensor with packed pixels (rows may be strided)."""
    t = torch.as_tensor(image)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{what} needs (h, w, 3) uint8 images")
    if t.stride(2) != 1 or t.stride(1) != 3:
        t = t.contiguous()
    return t


def _bgr_desc(t):
    return YhFrame(t.data_ptr(), None, t.shape[0], t.shape[1], t.stride(0), 0, YH_PIX_BGR, 0)


def letterbox_host(image, size, threads=1):
    """uint8 HWC BGR numpy image -> uint8 (3, size, size) RGB CHW numpy array (host C++)."""
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("letterbox_host needs an (h, w, 3) uint8 image")
    out = np.empty((3, size, size), dtype=np.uint8)
    check(lib().yh_letterbox_host(c_void_p(img.ctypes.data), img.shape[0], img.shape[1], img.strides[0], int(size),
                                  c_void_p(out.ctypes.data), int(threads)), "letterbox_host")
    return out


def letterbox_frames_host(frame, canvas, threads=1):
    """One host frame (an (h, w, 3) uint8 BGR array or an `NV12` of host planes) -> uint8 (3, H, W)
    RGB CHW numpy array on canvas = int or (H, W): yh_letterbox_frames_host, the twin of the kernel."""
    ch, cw = _hw(canvas)
    if isinstance(frame, NV12):
        if frame.device.type != "cpu":
            raise ValueError("letterbox_frames_host needs host planes")
        desc, keep = frame._desc(), frame
    else:
        keep = _bgr(frame, "letterbox_frames_host")
        desc = _bgr_desc(keep)
    out = np.empty((3, ch, cw), dtype=np.uint8)
    check(lib().yh_letterbox_frames_host(byref(desc), ch, cw, c_void_p(out.ctypes.data), int(threads)),
          "letterbox_frames_host")
    del keep
    return out


def nv12_to_bgr_host(frame):
    """`NV12` of host planes -> (h, w, 3) uint8 BGR numpy array (yh_nv12_to_bgr_host)."""
    if not isinstance(frame, NV12) or frame.device.type != "cpu":
        raise ValueError("nv12_to_bgr_host needs an NV12 of host planes")
    out = np.empty((frame.height, frame.width, 3), dtype=np.uint8)
    desc = frame._desc()
    check(lib().yh_nv12_to_bgr_host(byref(desc), c_void_p(out.ctypes.data)), "nv12_to_bgr_host")
    return out


def resize_linear_host(image, new_h, new_w):
    """cv2.resize(image, (new_w, new_h), interpolation=cv2.INTER_LINEAR) of a uint8 (h, w, 3) image (host C++)."""
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("resize_linear_host needs an (h, w, 3) uint8 image")
    out = np.empty((int(new_h), int(new_w), 3), dtype=np.uint8)
    check(lib().yh_resize_linear_host(c_void_p(img.ctypes.data), img.shape[0], img.shape[1], img.strides[0],
                                      int(new_h), int(new_w), c_void_p(out.ctypes.data)), "resize_linear_host")
    return out


def _default_device(images):
    for im in images:
        d = im.device if isinstance(im, (torch.Tensor, NV12)) else None
        if d is not None and d.type == "cuda":
            return d
    return torch.device("cuda", 0)


def letterbox(images, size, device=None, out=None):
    """Batch of uint8 HWC BGR images (tensors or arrays, any sizes) -> uint8 (B, 3, size, size) RGB
    CHW cuda tensor, on the current stream of `device` (default: the first cuda image's device,
    else cuda:0). Host images are copied to the device first."""
    if device is None:
        device = _default_device(images)
    device = torch.device(device)
    srcs = [_bgr(im, "letterbox").to(device, non_blocking=True) for im in images]
    B = len(srcs)
    if out is None:
        out = torch.empty((B, 3, size, size), dtype=torch.uint8, device=device)
    elif out.shape != (B, 3, size, size) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("letterbox: bad out tensor")
    if B == 0:
        return out
    ptrs = (c_void_p * B)(*[t.data_ptr() for t in srcs])
    hs = (c_int * B)(*[t.shape[0] for t in srcs])
    ws = (c_int * B)(*[t.shape[1] for t in srcs])
    st = (c_int * B)(*[t.stride(0) for t in srcs])
    with torch.cuda.device(device):
        check(lib().yh_letterbox(ptrs, hs, ws, st, B, int(size), c_void_p(out.data_ptr()),
                                 c_void_p(torch.cuda.current_stream(device).cuda_stream)), "letterbox")
    for t in srcs:   # keep the sources alive for the queued kernel
        t.record_stream(torch.cuda.current_stream(device))
    return out


def letterbox_frames(frames, canvas, device=None, out=None):
    """Batch of frames - (h, w, 3) uint8 BGR tensors / arrays and `NV12` objects, mixed, any sizes -
    -> uint8 (B, 3, H, W) RGB CHW cuda tensor for canvas = int or (H, W) (W a multiple of 4), on the
    current stream of `device` (default: the first cuda frame's device, else cuda:0). Host frames
    are copied to the device first. One launch per 32 frames (yh_letterbox_frames)."""
    if device is None:
        device = _default_device(frames)
    device = torch.device(device)
    ch, cw = _hw(canvas)
    srcs, descs = [], (YhFrame * max(1, len(frames)))()
    for k, f in enumerate(frames):
        if isinstance(f, NV12):
            f = f.to(device, non_blocking=True)
            srcs.extend(f.tensors())
            descs[k] = f._desc()
        else:
            t = _bgr(f, "letterbox_frames").to(device, non_blocking=True)
            srcs.append(t)
            descs[k] = _bgr_desc(t)
    B = len(frames)
    if out is None:
        out = torch.empty((B, 3, ch, cw), dtype=torch.uint8, device=device)
    elif out.shape != (B, 3, ch, cw) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("letterbox_frames: bad out tensor")
    if B == 0:
        return out
    stream = torch.cuda.current_stream(device)
    with torch.cuda.device(device):
        check(lib().yh_letterbox_frames(descs, B, ch, cw, c_void_p(out.data_ptr()), c_void_p(stream.cuda_stream)),
              "letterbox_frames")
    for t in srcs:   # keep the sources alive for the queued kernel
        t.record_stream(stream)
    return out


class Crops(NamedTuple):
    """Result of `crop_rois`: data (capacity, 3, h, w) uint8 RGB CHW, rois (capacity, 6) i32 rows of
    frame, row, x0, y0, w, h and total (1,) i32, all on the device of the boxes. Slots at or beyond
    total are zero, and so is the crop of an empty ROI (w = h = 0)."""
    data: torch.Tensor
    rois: torch.Tensor
    total: torch.Tensor

    def gather(self, t):
        """t (B, max_rois, ...) -> (capacity, ...): t[frame, row] of every slot, so that scores,
        classes or track ids follow their crops. No synchronisation; slots at or beyond total (rois
        rows of zeros) pick t[0, 0]."""
        if t.shape[0] == 0 or t.shape[1] == 0:
            return t.new_zeros((self.rois.shape[0],) + tuple(t.shape[2:]))
        idx = self.rois.long()
        return t[idx[:, 0], idx[:, 1]]

    def tolist(self):
        """[(crop (3, h, w), (frame, row, x0, y0, w, h)), ...] of the first total slots (reads total
        on the host: synchronises the current stream)."""
        n = int(self.total.item())
        return [(self.data[i], tuple(r)) for i, r in enumerate(self.rois[:n].tolist())]


def _check_crop(name, t, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"yolo_hip.crop_rois: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"yolo_hip.crop_rois: {name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"yolo_hip.crop_rois: {name} is on {t.device}, expected {device}")
    if len(shape) != t.dim() or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        want = tuple("*" if w is None else w for w in shape)
        raise ValueError(f"yolo_hip.crop_rois: {name} has shape {tuple(t.shape)}, expected {want}")
    if not t.is_contiguous():
        raise ValueError(f"yolo_hip.crop_rois: {name} must be contiguous")


def crop_rois(frames, boxes, counts, size, keep_aspect=False, pad=0.0, capacity=None, device=None, out=None,
              threads=0):
    """One fixed-size RGB crop per box, cut from the boxes' source frames: all frames of a call in
    one launch per 32 frames, nothing read back (yh_crop_rois; include/yolo_hip.h is the spec).

    frames: B frames as for `letterbox_frames` (BGR tensors / arrays and `NV12`, mixed, any sizes);
    boxes (B, max_rois, S >= 4) f32 with x1, y1, x2, y2 in frame pixels first - `Detections.dets` and
    `Tracks.dets` as they lie; counts (B,) i32 (rows at or beyond it are never read). size: int or
    (h, w), w a multiple of 4. keep_aspect=False stretches the box to the crop; True letterboxes it
    on a zero border. pad widens the box by that fraction of its size on every side. capacity
    (default B * max_rois) is the number of slots; rows beyond it are dropped.
    -> Crops(data, rois, total); out=(data, rois, total) reuses buffers. Every byte is written.

    cuda boxes run the HIP kernel asynchronously on the current stream of their device (host frames
    are copied there first); CPU boxes with host frames run the host twin (yh_crop_rois_host,
    `threads` <= 0: every hardware thread), which computes the same bytes."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3:
        raise ValueError("yolo_hip.crop_rois: boxes must be a (B, max_rois, S) tensor")
    dev = boxes.device
    if device is not None and torch.device(device) != dev:
        raise ValueError(f"yolo_hip.crop_rois: boxes are on {dev}, expected {torch.device(device)}")
    B, M, S = boxes.shape
    if len(frames) != B:
        raise ValueError(f"yolo_hip.crop_rois: {len(frames)} frames for boxes of {B} frames")
    _check_crop("boxes", boxes, (B, M, S), torch.float32, dev)
    _check_crop("counts", counts, (B,), torch.int32, dev)
    oh, ow = _hw(size)
    capacity = B * M if capacity is None else int(capacity)
    srcs, descs = [], (YhFrame * max(1, B))()
    for k, f in enumerate(frames):
        if isinstance(f, NV12):
            if dev.type == "cuda":
                f = f.to(dev, non_blocking=True)
            elif f.device != dev:
                raise ValueError("yolo_hip.crop_rois: CPU boxes need host frames")
            srcs.extend(f.tensors())
            descs[k] = f._desc()
        else:
            t = _bgr(f, "crop_rois")
            if dev.type == "cuda":
                t = t.to(dev, non_blocking=True)
            elif t.device != dev:
                raise ValueError("yolo_hip.crop_rois: CPU boxes need host frames")
            srcs.append(t)
            descs[k] = _bgr_desc(t)
    if out is None:
        data = torch.empty((max(capacity, 0), 3, max(oh, 0), max(ow, 0)), dtype=torch.uint8, device=dev)
        rois = torch.empty((max(capacity, 0), 6), dtype=torch.int32, device=dev)
        total = torch.empty((1,), dtype=torch.int32, device=dev)
    else:
        data, rois, total = out
        _check_crop("out data", data, (capacity, 3, oh, ow), torch.uint8, dev)
        _check_crop("out rois", rois, (capacity, 6), torch.int32, dev)
        _check_crop("out total", total, (1,), torch.int32, dev)

    def ptr(t):
        return c_void_p(t.data_ptr())

    args = (descs, B, ptr(boxes), S, ptr(counts), M, oh, ow, int(keep_aspect), float(pad), capacity, ptr(data),
            ptr(rois), ptr(total))
    if dev.type == "cuda":
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            check(lib().yh_crop_rois(*args, c_void_p(stream.cuda_stream)), "crop_rois")
        for t in srcs:   # keep the sources alive for the queued kernel
            t.record_stream(stream)
    elif dev.type == "cpu":
        check(lib().yh_crop_rois_host(*args, int(threads)), "crop_rois_host")
    else:
        raise ValueError(f"yolo_hip.crop_rois: unsupported device {dev}")
    del srcs
    return Crops(data, rois, total)
