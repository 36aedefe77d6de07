"""Camera-motion compensation for the tracker: the global translation between consecutive frames.

`track` predicts a track with its own velocity and gates on the IoU with the new detections, which
assumes a camera at rest. A pan of one box width between two frames takes every IoU of the frame to
zero: every track is lost and every object is born again under a new id. This module estimates the
camera's translation from the frames themselves (yh_motion: a luma thumbnail per frame, block matching
against the stream's previous thumbnail, sub-pixel refinement), and `track.warp` /
`Tracker.update(motion=...)` moves the tracks by it before the association - BoT-SORT's and
ultralytics' global-motion step, without a host read:

  motion_state     the zeroed state of `streams` streams (their last thumbnails)
  estimate         yh_motion / yh_motion_field and their host twins: one frame of every stream of a batch
  field_workspace  the device workspace of model="similarity"
  Motion           (motion (B, 3) f32 = s, tx, ty; sad (B, 2) i32 = best SAD, SAD at no shift)
  MotionEstimator  the state and the parameters of a set of streams

    dets = detector.predict(frames, keep_frames=True)
    tracks = tracker.update(dets, motion=estimator.estimate(dets.frames))

The default model is one translation per frame, at most `radius` thumbnail pixels long.
model="similarity" (yh_motion_field) adds an isotropic zoom for PTZ cameras and drones that climb or
descend: a shift per block of a grid over the thumbnail, a consensus among the blocks with texture,
and a least-squares (s, tx, ty) - the row `warp` takes - with the translation model's row as the
fallback. Rotation, rolling shutter and parallax are not modelled, and a moving foreground that fills
much of the frame biases either estimate. There is no counterpart in the reference; the semantics are
those stated in include/yolo_hip.h, pinned by the numpy restatements in tests/_motion_cases.py and
tests/_motion_field_cases.py.
"""
from ctypes import byref
from typing import NamedTuple

import torch

from ._call import frame_descs, host_stream_ids, run, tensor
from ._lib import YhMotionFieldParams, lib

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
    """Result of `estimate`: motion (B, 3) f32 rows of s, tx, ty in source pixels (s is 1 under the
    translation model) - content at (x, y) of the previous frame is at about (s x + tx, s y + ty)
    now; sad (B, 2) i32: the best global candidate's sum of absolute differences and the one at no
    shift."""
    motion: torch.Tensor
    sad: torch.Tensor


def _field_params(grid, radius, max_mad, min_contrast, tol, min_blocks):
    if not isinstance(grid, (tuple, list)) or len(grid) != 2:
        raise ValueError("yolo_hip.motion: grid is (grid_h, grid_w)")
    return YhMotionFieldParams(int(grid[0]), int(grid[1]), int(radius), int(max_mad), int(min_contrast), int(tol),
                               int(min_blocks), 0)


def field_workspace(batch, grid=(6, 10), radius=8, device="cuda"):
    """The caller-owned workspace of `estimate(model="similarity")` on a device, for batches of up to
    `batch` frames (uint8; yh_motion_field_workspace_bytes). Its contents mean nothing between calls."""
    n = lib().yh_motion_field_workspace_bytes(int(batch), int(grid[0]), int(grid[1]), int(radius))
    if n == 0 and batch > 0:
        raise ValueError("yolo_hip.motion: illegal grid or radius")
    return torch.empty((n,), dtype=torch.uint8, device=device)


def estimate(frames, state, thumb=(96, 160), radius=8, max_mad=24, stream_ids=None, out=None, threads=0,
             model="translation", grid=(6, 10), min_contrast=4, tol=1, min_blocks=6, field=None, workspace=None):
    """The motion of every frame of a batch against its stream's previous frame: one translation
    (model="translation", yh_motion) or translation plus zoom (model="similarity", yh_motion_field).

    model="similarity": the search window is cut into grid = (grid_h, grid_w) blocks, each block finds
    its own shift, the blocks that found texture and a match vote (max_mad and min_contrast per
    pixel), and s, tx, ty are fitted to a consensus of the votes within `tol` thumbnail pixels; with
    fewer than `min_blocks` votes, no consensus, a scene cut or a scale outside [0.8, 1.25] the row is
    the translation model's, byte for byte. field: an optional (B, grid_h * grid_w, 4) int32 tensor
    that receives per block dy, dx, best SAD, flags (1: voted, 2: inlier of the fit). workspace: a
    `field_workspace` tensor for the device path (None: allocated here). Both models advance the same
    state: a stream may change model from frame to frame.

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
    descs, srcs = frame_descs(who, frames, dev, "motion.estimate", "a CPU state needs host frames")
    if stream_ids is not None:
        tensor(who, "stream_ids", stream_ids, (B,), torch.int32, dev)
    if out is None:
        out = Motion(torch.empty((B, 3), dtype=torch.float32, device=dev),
                     torch.empty((B, 2), dtype=torch.int32, device=dev))
    else:
        out = Motion(*out)
        tensor(who, "out motion", out.motion, (B, 3), torch.float32, dev)
        tensor(who, "out sad", out.sad, (B, 2), torch.int32, dev)
    if model == "translation":
        args = (descs, B, stream_ids, state, S, th, tw, int(radius), int(max_mad), out.motion, out.sad)
        run(who, "motion", dev, args, threads, keep=srcs)   # the sources stay alive for the queued kernels
    elif model == "similarity":
        fp = _field_params(grid, radius, max_mad, min_contrast, tol, min_blocks)
        if field is not None:
            tensor(who, "field", field, (B, fp.grid_h * fp.grid_w, 4), torch.int32, dev)
        device_tail = ()
        if dev.type == "cuda":
            need = lib().yh_motion_field_workspace_bytes(B, fp.grid_h, fp.grid_w, fp.radius)
            if workspace is None:
                workspace = torch.empty((max(need, 4),), dtype=torch.uint8, device=dev)
            else:
                tensor(who, "workspace", workspace, (None,), torch.uint8, dev)
                if workspace.numel() < need:
                    raise ValueError(f"{who}: workspace must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
            device_tail = (workspace, workspace.numel())
            srcs.append(workspace)
        args = (descs, B, stream_ids, state, S, th, tw, byref(fp), out.motion, out.sad, field)
        run(who, "motion_field", dev, args, threads, device_tail=device_tail, keep=srcs)
    else:
        raise ValueError(f"{who}: model is 'translation' or 'similarity'")
    return out


class MotionEstimator:
    """The last thumbnails of `streams` video streams on one device.

    estimate(frames, stream_ids=None) returns the `Motion` of the batch against each stream's previous
    frame and keeps the new thumbnails; the first frame of a stream, and a frame the gate rejects,
    give the identity. stream_ids as `Tracker.update`'s: None, a host sequence of ints (checked) or
    an int32 tensor on the device (not checked). reset() forgets every frame; `state` is the state
    tensor. The launches of one estimator must run on one stream, frames of a stream in order.
    model="similarity" estimates a zoom as well (`estimate`'s grid, min_contrast, tol, min_blocks);
    the estimator then owns the device workspace. estimate(..., field=t) fills a per-block tensor."""

    def __init__(self, streams, device, thumb=(96, 160), radius=8, max_mad=24, model="translation", grid=(6, 10),
                 min_contrast=4, tol=1, min_blocks=6):
        self.device = torch.device(device)
        self.thumb = _thumb(thumb)
        self.radius, self.max_mad = int(radius), int(max_mad)
        if model not in ("translation", "similarity"):
            raise ValueError("yolo_hip.MotionEstimator: model is 'translation' or 'similarity'")
        self.model = model
        self.field = dict(grid=(int(grid[0]), int(grid[1])), min_contrast=int(min_contrast), tol=int(tol),
                          min_blocks=int(min_blocks))
        self.workspace = None
        if model == "similarity" and self.device.type == "cuda":
            self.workspace = field_workspace(_LAUNCH, self.field["grid"], self.radius, self.device)
        if not 1 <= self.radius <= MAX_RADIUS or min(self.thumb) - 2 * self.radius < 4:
            raise ValueError(f"yolo_hip.MotionEstimator: radius must be in [1, {MAX_RADIUS}] and leave a window of "
                             "at least 4 x 4 (thumb - 2 * radius)")
        self.streams = int(streams)
        self.state = motion_state(self.streams, self.thumb, self.device)

    def reset(self):
        self.state.zero_()

    def estimate(self, frames, stream_ids=None, out=None, threads=0, field=None):
        stream_ids = host_stream_ids("yolo_hip.MotionEstimator", stream_ids, self.streams, len(frames), self.device,
                                     "frames")
        if self.model == "translation":
            return estimate(frames, self.state, self.thumb, self.radius, self.max_mad, stream_ids=stream_ids, out=out,
                            threads=threads)
        return estimate(frames, self.state, self.thumb, self.radius, self.max_mad, stream_ids=stream_ids, out=out,
                        threads=threads, model="similarity", field=field, workspace=self.workspace, **self.field)
