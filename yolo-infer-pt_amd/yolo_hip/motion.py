"""Camera-motion compensation for the tracker: the global translation between consecutive frames.

`track` predicts a track with its own velocity and gates on the IoU with the new detections, which
assumes a camera at rest. A pan of one box width between two frames takes every IoU of the frame to
zero: every track is lost and every object is born again under a new id. This module estimates the
camera's translation from the frames themselves (yh_motion: a luma thumbnail per frame, block matching
against the stream's previous thumbnail, sub-pixel refinement), and `track.warp` /
`Tracker.update(motion=...)` moves the tracks by it before the association - BoT-SORT's and
ultralytics' global-motion step, without a host read:

  motion_state     the zeroed state of `streams` streams (their last thumbnails)
  estimate         yh_motion / yh_motion_host: one frame of every stream of a batch (functional)
  Motion           (motion (B, 3) f32 = s, tx, ty; sad (B, 2) i32 = best SAD, SAD at no shift)
  MotionEstimator  the state and the parameters of a set of streams

    dets = detector.predict(frames, keep_frames=True)
    tracks = tracker.update(dets, motion=estimator.estimate(dets.frames))

The model is one translation per frame, at most `radius` thumbnail pixels long; rotation, zoom,
rolling shutter and parallax are not modelled, and a moving foreground that fills much of the frame
biases the estimate. There is no counterpart in the reference; the semantics are those stated in
include/yolo_hip.h, pinned by the numpy restatement in tests/_motion_cases.py.
"""
from ctypes import c_void_p
from typing import NamedTuple

import torch

from ._lib import YhFrame, check, lib
from .preprocess import NV12, _bgr, _bgr_desc

MAX_RADIUS = 32      # YH_MOTION_MAX_RADIUS
MAX_THUMB = 32768    # YH_MOTION_MAX_THUMB
_HDR, _LAUNCH = 16, 32   # csrc/motion_host.h: header bytes per stream, staging thumbnails behind the streams


def _thumb(thumb):
    if not isinstance(thumb, (tuple, list)) or len(thumb) != 2:
        raise ValueError("yolo_hip.motion: thumb is (thumb_h, thumb_w)")
    th, tw = int(thumb[0]), int(thumb[1])
    if th < 1 or tw < 1 or tw % 4 or th * tw > MAX_THUMB:
        raise ValueError(f"yolo_hip.motion: thumb_w must be a positive multiple of 4 and thumb_h * thumb_w <= {MAX_THUMB}")
    return th, tw


def motion_state(streams, thumb=(96, 160), device="cpu"):
    """The empty state of `streams` streams for thumbnails of thumb = (h, w): uint8 zeros, per stream
    a 16-byte header and the last thumbnail, then a staging area of 32 thumbnails. The bytes are
    opaque, hold no addresses and mean the same on host and device."""
    streams = int(streams)
    th, tw = _thumb(thumb)
    if streams < 0:
        raise ValueError("yolo_hip.motion: streams must be >= 0")
    n = streams * (_HDR + th * tw) + _LAUNCH * th * tw
    if lib().yh_motion_state_bytes(streams, th, tw) != n:
        raise RuntimeError("yolo_hip.motion: the library's state size differs from motion_state's")
    return torch.zeros((n,), dtype=torch.uint8, device=device)


class Motion(NamedTuple):
    """Result of `estimate`: motion (B, 3) f32 rows of s, tx, ty (s is always 1) in source pixels -
    content at (x, y) of the previous frame is at about (x + tx, y + ty) now; sad (B, 2) i32: the
    best candidate's sum of absolute differences and the one at no shift."""
    motion: torch.Tensor
    sad: torch.Tensor


def estimate(frames, state, thumb=(96, 160), radius=8, max_mad=24, stream_ids=None, out=None, threads=0):
    """The translation of every frame of a batch against its stream's previous frame (yh_motion).

    frames: B frames as `Detections.frames` holds and `letterbox_frames` takes them (BGR tensors /
    arrays and `NV12`, mixed, any sizes at least the thumbnail's). state: a `motion_state` tensor,
    advanced in place; its device decides where the call runs. thumb, radius: the thumbnail's (h, w)
    and the search radius in thumbnail pixels (1 .. 32, thumb - 2 * radius >= 4 on both sides).
    max_mad: a best match whose mean absolute difference per window pixel is above it gives the
    identity (a scene cut); negative: no gate. stream_ids (B,) i32 on the state's device or None: row
    b is the next frame of stream stream_ids[b] (None: of stream b); distinct; a row whose id is
    outside [0, streams) gets the identity and touches no state.
    -> Motion of (B, 3) and (B, 2); out=(motion, sad) reuses buffers. Every byte is written.

    A cuda state runs the HIP kernels asynchronously on the current stream (host frames are copied
    there first), a CPU state with host frames the host twin (`threads` <= 0: every hardware
    thread); both give the same bytes, state included."""
    who = "yolo_hip.motion"
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 1 or not state.is_contiguous():
        raise ValueError(f"{who}: state must be a motion_state tensor")
    dev = state.device
    th, tw = _thumb(thumb)
    per = _HDR + th * tw
    rest = state.numel() - _LAUNCH * th * tw
    if rest < 0 or rest % per:
        raise ValueError(f"{who}: state has {state.numel()} bytes, not a motion_state of {th} x {tw} thumbnails")
    S = rest // per
    B = len(frames)
    srcs, descs = [], (YhFrame * max(1, B))()
    for k, f in enumerate(frames):
        if isinstance(f, NV12):
            if dev.type == "cuda":
                f = f.to(dev, non_blocking=True)
            elif f.device != dev:
                raise ValueError(f"{who}: a CPU state needs host frames")
            srcs.extend(f.tensors())
            descs[k] = f._desc()
        else:
            t = _bgr(f, "motion.estimate")
            if dev.type == "cuda":
                t = t.to(dev, non_blocking=True)
            elif t.device != dev:
                raise ValueError(f"{who}: a CPU state needs host frames")
            srcs.append(t)
            descs[k] = _bgr_desc(t)
    if stream_ids is not None:
        if (not isinstance(stream_ids, torch.Tensor) or stream_ids.dtype != torch.int32 or stream_ids.device != dev
                or tuple(stream_ids.shape) != (B,) or not stream_ids.is_contiguous()):
            raise ValueError(f"{who}: stream_ids must be a contiguous (B,) int32 tensor on {dev}")
    if out is None:
        out = Motion(torch.empty((B, 3), dtype=torch.float32, device=dev),
                     torch.empty((B, 2), dtype=torch.int32, device=dev))
    else:
        out = Motion(*out)
        for name, t, shape, dt in (("motion", out.motion, (B, 3), torch.float32), ("sad", out.sad, (B, 2), torch.int32)):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != dev or tuple(t.shape) != shape
                    or not t.is_contiguous()):
                raise ValueError(f"{who}: out {name} must be a contiguous {shape} {dt} tensor on {dev}")

    def ptr(t):
        return c_void_p(t.data_ptr()) if t is not None else None

    args = (descs, B, ptr(stream_ids), ptr(state), S, th, tw, int(radius), int(max_mad), ptr(out.motion), ptr(out.sad))
    if dev.type == "cuda":
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            check(lib().yh_motion(*args, c_void_p(stream.cuda_stream)), "motion")
        for t in srcs:   # keep the sources alive for the queued kernels
            t.record_stream(stream)
    elif dev.type == "cpu":
        check(lib().yh_motion_host(*args, int(threads)), "motion_host")
    else:
        raise ValueError(f"{who}: unsupported device {dev}")
    del srcs
    return out


class MotionEstimator:
    """The last thumbnails of `streams` video streams on one device.

    estimate(frames, stream_ids=None) returns the `Motion` of the batch against each stream's previous
    frame and keeps the new thumbnails; the first frame of a stream, and a frame the gate rejects,
    give the identity. stream_ids as `Tracker.update`'s: None, a host sequence of ints (checked) or
    an int32 tensor on the device (not checked). reset() forgets every frame; `state` is the state
    tensor. The launches of one estimator must run on one stream, frames of a stream in order."""

    def __init__(self, streams, device, thumb=(96, 160), radius=8, max_mad=24):
        self.device = torch.device(device)
        self.thumb = _thumb(thumb)
        self.radius, self.max_mad = int(radius), int(max_mad)
        if not 1 <= self.radius <= MAX_RADIUS or min(self.thumb) - 2 * self.radius < 4:
            raise ValueError(f"yolo_hip.MotionEstimator: radius must be in [1, {MAX_RADIUS}] and leave a window of "
                             "at least 4 x 4 (thumb - 2 * radius)")
        self.streams = int(streams)
        self.state = motion_state(self.streams, self.thumb, self.device)

    def reset(self):
        self.state.zero_()

    def estimate(self, frames, stream_ids=None, out=None, threads=0):
        if stream_ids is not None and not isinstance(stream_ids, torch.Tensor):
            host = [int(v) for v in stream_ids]
            if len(set(host)) != len(host):
                raise ValueError("yolo_hip.MotionEstimator: stream_ids must be distinct")
            if any(not 0 <= v < self.streams for v in host):
                raise ValueError(f"yolo_hip.MotionEstimator: stream_ids must lie in [0, {self.streams})")
            stream_ids = torch.tensor(host, dtype=torch.int32).to(self.device, non_blocking=True)
        elif stream_ids is None and len(frames) > self.streams:
            raise ValueError(f"yolo_hip.MotionEstimator: a batch of {len(frames)} frames for {self.streams} streams")
        return estimate(frames, self.state, self.thumb, self.radius, self.max_mad, stream_ids=stream_ids, out=out,
                        threads=threads)
