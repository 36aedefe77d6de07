"""Object identities across the frames of many video streams, on the device.

`nms` (and `Detector`) return boxes per frame; video users also need to know which box of this
frame is which box of the last. This module keeps a track table per stream and advances all
streams of a batch by one frame in a single launch, reading the fixed-size NMS output where it
lies - no copy to the host, no synchronisation:

  track        yh_track / yh_track_host: one frame of every stream of a batch (functional)
  track_state  the zeroed state tensor of `streams` streams
  Tracks       (dets, ids, det_index, counts) of one call
  track_reid   yh_track_reid: `track` with an appearance term (int8 features, cosine by int8 MFMA)
  warp         yh_track_warp: a camera motion (yolo_hip.motion) applied to the tracks before a frame
  assign       yh_assign: batched maximum-weight assignment; `track(..., assign="optimal")` and
               `track_reid` likewise choose among an association's candidates with it (yh_track2)
  embed_quantize, embed_similarity   its two primitives, usable alone for gallery search
  Tracker      the state, the thresholds and the buffers of a set of streams; `update` for a
               caller's loop, `post` as the in-stream hook of a DetectPipeline

The rules are ByteTrack's with ultralytics' KalmanFilterXYWH (a first association of the high
scores with tracked and lost tracks, a second of the low scores with the tracks still unmatched,
a third of the remaining high scores with the tentative tracks; new tracks are tentative for a
frame), with two deliberate differences: by default the association is a greedy walk over the
pairs by IoU where ByteTrack solves an assignment (lapjv) - assign="optimal" solves it, with fixed
tie rules - and it only pairs equal classes unless class_aware is off. There
is no counterpart in the reference; the semantics are those stated in include/yolo_hip.h, pinned
by the numpy restatement in tests/_track_cases.py.
"""
import ctypes
from typing import NamedTuple

import torch

MAX_TRACKS = 1024   # YH_TRACK_MAX_TRACKS
MAX_DET = 1024      # YH_TRACK_MAX_DET
REID_MAX_DIM = 2048  # YH_REID_MAX_DIM
ASSIGN_MAX_WEIGHT = 1 << 16   # YH_ASSIGN_MAX_WEIGHT
ASSIGN_MAX_SIZE = 1024        # YH_ASSIGN_MAX_SIZE
ASSIGN_MODES = {"greedy": 0, "optimal": 1}   # YH_ASSIGN_GREEDY, YH_ASSIGN_OPTIMAL
_HDR, _FIELDS = 4, 24   # state words per stream: _HDR + _FIELDS * max_tracks (csrc/track_host.h)


class TrackParams(ctypes.Structure):
    """yh_track_params"""
    _fields_ = [("track_high", ctypes.c_float), ("track_low", ctypes.c_float), ("track_new", ctypes.c_float),
                ("iou_first", ctypes.c_float), ("iou_second", ctypes.c_float), ("iou_tentative", ctypes.c_float),
                ("max_age", ctypes.c_int), ("class_aware", ctypes.c_int)]


def params(track_high=0.25, track_low=0.1, track_new=0.25, iou_first=0.2, iou_second=0.5, iou_tentative=0.3,
           max_age=30, class_aware=True):
    """The thresholds of `track` (yh_track_params). IoU thresholds are minimum overlaps: ByteTrack's
    match_thresh 0.8 is a maximum cost 1 - IoU, i.e. iou_first = 0.2."""
    return TrackParams(track_high, track_low, track_new, iou_first, iou_second, iou_tentative, int(max_age),
                       1 if class_aware else 0)


class ReidParams(ctypes.Structure):
    """yh_reid_params"""
    _fields_ = [("cos_min", ctypes.c_float), ("iou_min", ctypes.c_float)]


class AssignParams(ctypes.Structure):
    """yh_assign_params"""
    _fields_ = [("mode", ctypes.c_int), ("reserved", ctypes.c_int * 3)]


def _assign_params(assign):
    if assign not in ASSIGN_MODES:
        raise ValueError(f"yolo_hip.track: assign must be 'greedy' or 'optimal', got {assign!r}")
    return AssignParams(ASSIGN_MODES[assign])


def _check_dim(dim, who="yolo_hip.track"):
    dim = int(dim)
    if dim % 64 or not 64 <= dim <= REID_MAX_DIM:
        raise ValueError(f"{who}: the feature length must be a multiple of 64 in [64, {REID_MAX_DIM}], got {dim}")
    return dim


def _reid_words(max_tracks, dim):
    return _HDR + _FIELDS * max_tracks + max_tracks * dim // 4


def track_state(streams, max_tracks=256, device="cpu", reid_dim=None):
    """The empty state of `streams` streams: (streams, 4 + 24 * max_tracks) int32 zeros. The words are
    opaque, hold no addresses and mean the same on host and device: .cpu() / .to(device) / a file
    carry a state over in the middle of a sequence. reid_dim: the state of `track_reid` for features
    of that length: each stream's words are followed by its gallery, max_tracks * reid_dim int8."""
    streams, max_tracks = int(streams), int(max_tracks)
    if streams < 0 or not 1 <= max_tracks <= MAX_TRACKS:
        raise ValueError(f"yolo_hip.track: streams must be >= 0 and max_tracks in [1, {MAX_TRACKS}]")
    words = _HDR + _FIELDS * max_tracks if reid_dim is None else _reid_words(max_tracks, _check_dim(reid_dim))
    return torch.zeros((streams, words), dtype=torch.int32, device=device)


class Tracks(NamedTuple):
    """Result of one tracker call: dets (B, max_out, 6) f32 = x1, y1, x2, y2 of the track's filtered
    box, then the score and class of the detection it was matched to; ids (B, max_out) i32 track
    ids (>= 1, unique within a stream); det_index (B, max_out) i32 the row of that detection in
    the input; counts (B,) i32. Rows beyond a count are 0."""
    dets: torch.Tensor
    ids: torch.Tensor
    det_index: torch.Tensor
    counts: torch.Tensor

    def tolist(self):
        """Per-stream (dets (k, 6), ids (k,), det_index (k,)) (reads counts on the host: synchronises
        the current stream)."""
        return [(self.dets[i, :k], self.ids[i, :k], self.det_index[i, :k]) for i, k in enumerate(self.counts.tolist())]


def _check(name, t, shape, dtype, device, who="yolo_hip.track"):
    if not isinstance(t, torch.Tensor):
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


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _frame_args(dets, counts, state, stream_ids, max_out, out):
    """The checks `track` and `track_reid` share -> (device, B, max_det, max_out, Tracks to write)."""
    if not isinstance(dets, torch.Tensor) or dets.dim() != 3:
        raise ValueError("yolo_hip.track: dets must be a (B, max_det, 6) tensor")
    dev = dets.device
    B, md = dets.shape[0], dets.shape[1]
    _check("dets", dets, (B, md, 6), torch.float32, dev)
    _check("counts", counts, (B,), torch.int32, dev)
    _check("state", state, (None, None), torch.int32, dev)
    if stream_ids is not None:
        _check("stream_ids", stream_ids, (B,), torch.int32, dev)
    max_out = md if max_out is None else int(max_out)
    if out is None:
        o = Tracks(torch.empty((B, max(max_out, 0), 6), dtype=torch.float32, device=dev),
                   torch.empty((B, max(max_out, 0)), dtype=torch.int32, device=dev),
                   torch.empty((B, max(max_out, 0)), dtype=torch.int32, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))
    else:
        o = Tracks(*out)
        _check("out dets", o.dets, (B, max_out, 6), torch.float32, dev)
        _check("out ids", o.ids, (B, max_out), torch.int32, dev)
        _check("out det_index", o.det_index, (B, max_out), torch.int32, dev)
        _check("out counts", o.counts, (B,), torch.int32, dev)
    return dev, B, md, max_out, o


def track(dets, counts, state, p=None, stream_ids=None, max_out=None, out=None, threads=0, assign="greedy"):
    """One frame of every stream of a batch, in one launch.

    dets (B, max_det, 6) f32 and counts (B,) i32 as `nms` or `Detector` return them (rows at or
    beyond counts[b] are never read); state: a `track_state` tensor, advanced in place; p: `params()`
    (default: its defaults); stream_ids (B,) i32 or None: row b is the next frame of stream
    stream_ids[b] (None: of stream b). The ids must be distinct; a row whose id is outside
    [0, streams) gets count 0 and touches no state. All on one device, all contiguous.
    -> Tracks of (B, max_out, ...) (max_out defaults to max_det); out=(dets, ids, det_index, counts)
    reuses buffers. Every byte is written.

    assign: "greedy" (the default: the sorted walk over the candidate pairs) or "optimal": each
    association takes, among the same candidate pairs, a matching of maximum total IoU (yh_assign's,
    deterministic). It keeps ids where tracks compete for the same detections and costs more time;
    the state is the same, so the mode may change between frames.

    cuda tensors run the HIP kernel (yh_track2) asynchronously on the current stream, CPU tensors
    the host twin (yh_track_host, `threads` <= 0: every hardware thread); both give the same bytes,
    state included. Frames of one stream must be submitted in order on one stream."""
    from ._lib import check, lib
    dev, B, md, max_out, o = _frame_args(dets, counts, state, stream_ids, max_out, out)
    S, words = state.shape
    if words < _HDR + _FIELDS or (words - _HDR) % _FIELDS:
        raise ValueError(f"yolo_hip.track: state has {words} words per stream, expected 4 + 24 * max_tracks")
    mt = (words - _HDR) // _FIELDS
    p = params() if p is None else p
    ptr = _ptr
    L = lib()
    if mt <= MAX_TRACKS and L.yh_track_state_bytes(S, mt) != state.numel() * 4:
        raise RuntimeError("yolo_hip.track: the library's state size differs from track_state's")
    ap = _assign_params(assign)
    args = (ptr(dets), ptr(counts), B, md, ptr(stream_ids), ptr(state), S, mt, ctypes.byref(p), max_out,
            ptr(o.dets), ptr(o.ids), ptr(o.det_index), ptr(o.counts), ctypes.byref(ap))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_track2(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "track")
    elif dev.type == "cpu":
        check(L.yh_track2_host(*args, int(threads)), "track_host")
    else:
        raise ValueError(f"yolo_hip.track: unsupported device {dev}")
    return o


def warp(state, motion, max_tracks, reid_dim=None, stream_ids=None, threads=0):
    """Move the tracks of a batch's streams by a camera motion, before the frame's `track` call
    (yh_track_warp). state: a `track_state` tensor (reid_dim: as it was made), changed in place;
    motion (B, 3) f32 rows of s, tx, ty - a `yolo_hip.motion.Motion` or its tensor: a track's centre
    becomes s * c + t, its size, velocities and covariances scale with s (s * s); stream_ids as
    `track`'s. A row with an id out of range, or a motion that is not finite or has s <= 0, changes
    nothing; with s == 1 only the centres change. cuda tensors run the kernel on the current stream,
    CPU tensors the host twin: the same bytes. -> state"""
    from ._lib import check, lib
    motion = getattr(motion, "motion", motion)
    if not isinstance(motion, torch.Tensor) or motion.dim() != 2:
        raise ValueError("yolo_hip.track: motion must be a (B, 3) tensor")
    dev = motion.device
    B = motion.shape[0]
    _check("motion", motion, (B, 3), torch.float32, dev)
    _check("state", state, (None, None), torch.int32, dev)
    if stream_ids is not None:
        _check("stream_ids", stream_ids, (B,), torch.int32, dev)
    mt = int(max_tracks)
    dim = 0 if reid_dim is None else _check_dim(reid_dim)
    S, words = state.shape
    want = _HDR + _FIELDS * mt if not dim else _reid_words(mt, dim)
    if not 1 <= mt <= MAX_TRACKS or words != want:
        raise ValueError(f"yolo_hip.track: state has {words} words per stream, expected {want} for max_tracks {mt}"
                         f"{'' if not dim else f' and reid_dim {dim}'}")
    L = lib()
    args = (_ptr(state), S, mt, dim, _ptr(motion), _ptr(stream_ids), B)
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_track_warp(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "track_warp")
    elif dev.type == "cpu":
        check(L.yh_track_warp_host(*args, int(threads)), "track_warp_host")
    else:
        raise ValueError(f"yolo_hip.track: unsupported device {dev}")
    return state


def reid_workspace(batch, max_det, max_tracks, dim, device="cpu"):
    """The scratch buffer of `track_reid` for these sizes (uint8; its contents mean nothing between
    calls)."""
    from ._lib import lib
    n = lib().yh_track_reid_workspace_bytes(int(batch), int(max_det), int(max_tracks), _check_dim(dim))
    return torch.empty((n,), dtype=torch.uint8, device=device)


def track_reid(dets, counts, state, embed=None, feat_counts=None, embed_total=None, dim=None, reid_cos=0.5,
               reid_iou=0.5, p=None, stream_ids=None, max_out=None, out=None, workspace=None, threads=0,
               assign="greedy"):
    """`track` with an appearance term in its first association (yh_track_reid): a track and a
    high-score row may also pair when their features agree (cosine >= reid_cos) and they overlap
    at least reid_iou, and such a pair is walked at the larger of its IoU and (1 + cosine) / 2.
    reid_iou = 0 re-identifies a lost track anywhere in the frame. BoT-SORT's values are the
    defaults.

    state: `track_state(..., reid_dim=dim)`; it also carries one int8 feature per track.
    embed (capacity, dim) f32 or None: the features of the rows, compacted as `crop_rois` compacts
    its crops: row r of batch row b has a feature iff r < n_b = clamp(feat_counts[b], 0, counts[b])
    (feat_counts None: the counts), at embed[n_0 + ... + n_(b-1) + r], as long as that index is
    below capacity and below embed_total[0] when given - `Classified.embed` of `Crops` cut with
    counts=feat_counts, and `Crops.total`, plug in as they lie. dim: the feature length when embed
    is None. workspace: a `reid_workspace` to reuse (None: allocated per call).
    Without features the result and the tracks are exactly `track`'s. assign: as `track`'s; in
    "optimal" mode the first association maximises the total of the pairs' values (the larger of
    IoU and (1 + cosine) / 2 where eligible).

    cuda tensors run the HIP kernels (quantise, the int8 MFMA similarity, the track kernel) on
    the current stream, CPU tensors the host twin; both give the same bytes, state included."""
    from ._lib import check, lib
    dev, B, md, max_out, o = _frame_args(dets, counts, state, stream_ids, max_out, out)
    if embed is not None:
        if not isinstance(embed, torch.Tensor) or embed.dim() != 2:
            raise ValueError("yolo_hip.track: embed must be a (capacity, dim) tensor")
        if dim is not None and int(dim) != embed.shape[1]:
            raise ValueError(f"yolo_hip.track: embed has {embed.shape[1]} columns, dim is {dim}")
        dim = embed.shape[1]
        _check("embed", embed, (None, dim), torch.float32, dev)
    elif dim is None:
        raise ValueError("yolo_hip.track: without embed, dim must be given")
    dim = _check_dim(dim)
    if feat_counts is not None:
        _check("feat_counts", feat_counts, (B,), torch.int32, dev)
    if embed_total is not None:
        _check("embed_total", embed_total, (1,), torch.int32, dev)
    S, words = state.shape
    per = _FIELDS + dim // 4
    if words < _HDR + per or (words - _HDR) % per:
        raise ValueError(f"yolo_hip.track: state has {words} words per stream, expected 4 + (24 + dim / 4) * max_tracks")
    mt = (words - _HDR) // per
    L = lib()
    if mt <= MAX_TRACKS and L.yh_track_reid_state_bytes(S, mt, dim) != state.numel() * 4:
        raise RuntimeError("yolo_hip.track: the library's state size differs from track_state's")
    need = L.yh_track_reid_workspace_bytes(B, md, mt, dim)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    else:
        _check("workspace", workspace, (None,), torch.uint8, dev)
    p = params() if p is None else p
    rp = ReidParams(float(reid_cos), float(reid_iou))
    ap = _assign_params(assign)
    args = (_ptr(dets), _ptr(counts), B, md, _ptr(stream_ids), _ptr(state), S, mt, ctypes.byref(p), max_out,
            _ptr(o.dets), _ptr(o.ids), _ptr(o.det_index), _ptr(o.counts), _ptr(embed),
            0 if embed is None else embed.shape[0], dim, _ptr(feat_counts), _ptr(embed_total), ctypes.byref(rp),
            _ptr(workspace), workspace.numel(), ctypes.byref(ap))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_track_reid2(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "track_reid")
    elif dev.type == "cpu":
        check(L.yh_track_reid2_host(*args, int(threads)), "track_reid_host")
    else:
        raise ValueError(f"yolo_hip.track: unsupported device {dev}")
    return o


def assign(weights, t_counts=None, d_counts=None, out=None, threads=0):
    """Batched maximum-weight assignment (yh_assign): weights (problems, T, D) int32, 0 = the pair is
    forbidden, 1 .. 65536 its weight (values outside are clamped into [0, 65536]); T, D <= 1024.
    t_counts / d_counts (problems,) int32 or None: only the leading slots / rows of a problem take
    part and nothing beyond them is read. -> (row_of_slot (problems, T), slot_of_row (problems, D))
    int32, -1 where unmatched; out=(row_of_slot, slot_of_row) reuses buffers, every element is
    written. The matching has the largest total weight over the allowed pairs (not the largest
    size); among equal totals the one the algorithm stated in include/yolo_hip.h finds.
    cuda tensors run the kernel on the current stream, CPU tensors the host twin: the same bytes."""
    from ._lib import check, lib
    who = "yolo_hip.assign"
    if not isinstance(weights, torch.Tensor) or weights.dim() != 3:
        raise ValueError(f"{who}: weights must be a (problems, T, D) tensor")
    dev = weights.device
    P, T, D = weights.shape
    _check("weights", weights, (P, T, D), torch.int32, dev, who)
    if t_counts is not None:
        _check("t_counts", t_counts, (P,), torch.int32, dev, who)
    if d_counts is not None:
        _check("d_counts", d_counts, (P,), torch.int32, dev, who)
    if out is None:
        out = (torch.empty((P, T), dtype=torch.int32, device=dev), torch.empty((P, D), dtype=torch.int32, device=dev))
    else:
        _check("out row_of_slot", out[0], (P, T), torch.int32, dev, who)
        _check("out slot_of_row", out[1], (P, D), torch.int32, dev, who)
    L = lib()
    args = (_ptr(weights), P, T, D, _ptr(t_counts), _ptr(d_counts), _ptr(out[0]), _ptr(out[1]))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_assign(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "assign")
    elif dev.type == "cpu":
        check(L.yh_assign_host(*args, int(threads)), "assign_host")
    else:
        raise ValueError(f"{who}: unsupported device {dev}")
    return out[0], out[1]


def embed_quantize(e, count=None, out=None, threads=0):
    """Unit int8 features (yh_embed_quantize): e (rows, dim) f32 -> (rows, dim) int8, each row scaled
    to length 127; a row of zeros, or with an element that is not finite, gives zeros ("no
    feature"). count (1,) i32 or None: rows at or beyond it give zeros. dim % 64 == 0, 64 <= dim <=
    2048. cuda tensors run the kernel on the current stream, CPU tensors the host twin: the same
    bytes."""
    from ._lib import check, lib
    if not isinstance(e, torch.Tensor) or e.dim() != 2:
        raise ValueError("yolo_hip.track: e must be a (rows, dim) tensor")
    dev = e.device
    rows, dim = e.shape
    _check("e", e, (rows, dim), torch.float32, dev)
    _check_dim(dim)
    if count is not None:
        _check("count", count, (1,), torch.int32, dev)
    if out is None:
        out = torch.empty((rows, dim), dtype=torch.int8, device=dev)
    else:
        _check("out", out, (rows, dim), torch.int8, dev)
    L = lib()
    args = (_ptr(e), rows, dim, _ptr(count), _ptr(out))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_embed_quantize(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "embed_quantize")
    elif dev.type == "cpu":
        check(L.yh_embed_quantize_host(*args, int(threads)), "embed_quantize_host")
    else:
        raise ValueError(f"yolo_hip.track: unsupported device {dev}")
    return out


def embed_similarity(a, b, a_index=None, out=None, threads=0):
    """Exact int32 products of int8 features (yh_embed_similarity): out[i] = A[i] @ b[i].T.
    a (nblocks, ra, dim) int8, whose blocks may be strided (a.stride(0) >= ra * dim, the rest
    contiguous); b (B, rb, dim) int8; a_index (B,) i32 or None: batch row i reads block
    a_index[i] (None: block i), a block out of range counts as zeros. -> (B, ra, rb) int32. Two
    `embed_quantize` rows give 16129 times their cosine. cuda tensors run the int8 MFMA kernel on
    the current stream, CPU tensors the host twin: the same numbers."""
    from ._lib import check, lib
    if not isinstance(a, torch.Tensor) or a.dim() != 3 or not isinstance(b, torch.Tensor) or b.dim() != 3:
        raise ValueError("yolo_hip.track: a must be (nblocks, ra, dim) and b (B, rb, dim)")
    dev = a.device
    nblocks, ra, dim = a.shape
    B, rb = b.shape[0], b.shape[1]
    _check_dim(dim)
    _check("b", b, (B, rb, dim), torch.int8, dev)
    if a.dtype != torch.int8 or a.device != dev:
        raise TypeError("yolo_hip.track: a must be int8 on b's device")
    if ra > 0 and nblocks > 0 and (a.stride(2) != 1 or a.stride(1) != dim or (nblocks > 1 and a.stride(0) < ra * dim)):
        raise ValueError("yolo_hip.track: the blocks of a must be contiguous and must not overlap")
    stride = a.stride(0) if nblocks > 1 else ra * dim
    if a_index is not None:
        _check("a_index", a_index, (B,), torch.int32, dev)
    if out is None:
        out = torch.empty((B, ra, rb), dtype=torch.int32, device=dev)
    else:
        _check("out", out, (B, ra, rb), torch.int32, dev)
    L = lib()
    args = (_ptr(a), stride, nblocks, _ptr(a_index), _ptr(b), B, ra, rb, dim, _ptr(out))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(L.yh_embed_similarity(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "embed_similarity")
    elif dev.type == "cpu":
        check(L.yh_embed_similarity_host(*args, int(threads)), "embed_similarity_host")
    else:
        raise ValueError(f"yolo_hip.track: unsupported device {dev}")
    return out


class Tracker:
    """The tracks of `streams` video streams on one device.

    update(dets, counts, stream_ids=None) (or update(detections) with a yolo_hip.Detections)
    advances the streams of the batch by one frame and returns Tracks. stream_ids: None (row b is
    stream b), a host sequence of ints (checked: distinct and inside [0, streams)) or an int32
    tensor on the device (not checked: reading it would synchronise; the kernel ignores rows with
    an id out of range, equal ids in one call are undefined).
    post(dets, counts) is the same with row b = stream b, shaped as DetectPipeline's `post` hook:
    it runs on the pipeline's NMS stream right behind each batch's NMS, and the batch's Tracks
    come back as the `extra` of submit(), valid after `done`.
    reset(streams=None) forgets every track (and optionally changes the number of streams);
    `state` is the state tensor (save it, move it, or assign one of the same shape).

    Order. Frames of one stream must reach the tracker in order, and the launches of one Tracker
    must run on one stream (they update the state in place). update() on the caller's stream does.
    Inside a DetectPipeline, the default configuration does: every batch's NMS, and with it post(),
    runs on the single NMS stream in submission order, whatever the number of lanes. nms_on_lane
    with several lanes does not: each lane's NMS runs on that lane's stream and batch k + 1 may
    pass batch k. post() raises when it is called on another stream than its first call (reset()
    clears that). A Tracker is constructed and reset on the current stream; submit() orders the
    pipeline's work after it.

    Re-identification. With reid_dim (the feature length) the tracker is `track_reid`'s: update()
    also takes embed, feat_counts and embed_total (see `track_reid`; reid_cos and reid_iou are its
    thresholds), the state carries a feature per track, and the tracker owns the workspace, sized
    at the first call and again when the batch shape grows. `feature_counts` says which rows to cut
    and embed. Without reid_dim a Tracker is the plain IoU tracker and takes no embeddings.

    assign: "greedy" (default) or "optimal", passed to every `track` / `track_reid` call (the
    attribute may be changed between frames).

    Camera motion. update(..., motion=m) with a (B, 3) tensor of s, tx, ty per batch row - or the
    `Motion` a `yolo_hip.motion.MotionEstimator` returns for the batch's frames - first moves the
    tracks of the batch's streams by it (`warp`, same stream_ids, same stream), so that a moving
    camera does not break the IoU association. post() takes none: the pipeline's hook has no frames.

    Nothing here reads a device value on the host. Outputs are allocated per call on the stream
    the call runs on (DetectPipeline marks its `extra` for the caller's stream)."""

    def __init__(self, streams, device, max_tracks=256, max_out=None, track_high=0.25, track_low=0.1, track_new=0.25,
                 iou_first=0.2, iou_second=0.5, iou_tentative=0.3, max_age=30, class_aware=True, reid_dim=None,
                 reid_cos=0.5, reid_iou=0.5, assign="greedy"):
        _assign_params(assign)
        self.assign = assign
        self.device = torch.device(device)
        self.max_tracks = int(max_tracks)
        self.max_out = None if max_out is None else int(max_out)
        if track_low > track_high:
            raise ValueError("yolo_hip.Tracker: track_low must be <= track_high")
        if max_age < 0:
            raise ValueError("yolo_hip.Tracker: max_age must be >= 0")
        self.params = params(track_high, track_low, track_new, iou_first, iou_second, iou_tentative, max_age,
                             class_aware)
        self.reid_dim = None if reid_dim is None else _check_dim(reid_dim)
        self.reid_cos, self.reid_iou = float(reid_cos), float(reid_iou)
        self._workspace = None
        self.state = track_state(streams, self.max_tracks, self.device, self.reid_dim)
        self._post_stream = None

    @property
    def streams(self):
        return self.state.shape[0]

    def reset(self, streams=None):
        if streams is None or int(streams) == self.streams:
            self.state.zero_()
        else:
            self.state = track_state(streams, self.max_tracks, self.device, self.reid_dim)
        self._post_stream = None

    def feature_counts(self, dets, counts):
        """(B,) int32: per batch row the number of leading rows with score >= track_high, clamped to
        the counts - the rows the first association and the births look at, hence the only rows whose
        feature is ever read. Cut and embed these (`crop_rois(..., counts=feature_counts)`) and
        pass the result to update() as feat_counts. Counting the leading rows is valid because
        `nms` (yh_nms) and `merge` (yh_merge) emit the rows of a frame by descending score, so the
        rows at or above the threshold are a prefix. Torch ops on the device; nothing is read on
        the host."""
        md = dets.shape[1]
        live = torch.arange(md, device=dets.device).unsqueeze(0) < counts.clamp(0, md).unsqueeze(1)
        high = (dets[:, :, 4] >= self.params.track_high) & live      # NaN padding compares false
        return torch.cumprod(high.to(torch.int32), dim=1).sum(dim=1).to(torch.int32)

    def update(self, dets, counts=None, stream_ids=None, threads=0, embed=None, feat_counts=None, embed_total=None,
               motion=None):
        if counts is None:                       # a Detections
            dets, counts = dets.dets, dets.counts
        if self.reid_dim is None and (embed is not None or feat_counts is not None or embed_total is not None):
            raise ValueError("yolo_hip.Tracker: embeddings need a Tracker made with reid_dim")
        if stream_ids is not None and not isinstance(stream_ids, torch.Tensor):
            host = [int(v) for v in stream_ids]
            if len(set(host)) != len(host):
                raise ValueError("yolo_hip.Tracker: stream_ids must be distinct")
            if any(not 0 <= v < self.streams for v in host):
                raise ValueError(f"yolo_hip.Tracker: stream_ids must lie in [0, {self.streams})")
            stream_ids = torch.tensor(host, dtype=torch.int32).to(self.device, non_blocking=True)
        elif stream_ids is None and isinstance(dets, torch.Tensor) and dets.dim() == 3 and dets.shape[0] > self.streams:
            raise ValueError(f"yolo_hip.Tracker: a batch of {dets.shape[0]} rows for {self.streams} streams")
        if motion is not None:                   # the camera's motion first, on the same stream
            warp(self.state, motion, self.max_tracks, reid_dim=self.reid_dim, stream_ids=stream_ids, threads=threads)
        if self.reid_dim is None:
            return track(dets, counts, self.state, self.params, stream_ids=stream_ids, max_out=self.max_out,
                         threads=threads, assign=self.assign)
        from ._lib import lib
        need = lib().yh_track_reid_workspace_bytes(dets.shape[0], dets.shape[1], self.max_tracks, self.reid_dim)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return track_reid(dets, counts, self.state, embed=embed, feat_counts=feat_counts, embed_total=embed_total,
                          dim=self.reid_dim, reid_cos=self.reid_cos, reid_iou=self.reid_iou, p=self.params,
                          stream_ids=stream_ids, max_out=self.max_out, workspace=self._workspace, threads=threads,
                          assign=self.assign)

    def post(self, dets, counts):
        if self.device.type == "cuda":
            cur = torch.cuda.current_stream(self.device)
            if self._post_stream is None:
                self._post_stream = cur
            elif cur != self._post_stream:
                raise RuntimeError("yolo_hip.Tracker.post: called on a second stream; frames are only in order on the "
                                   "pipeline's single NMS stream (nms_on_lane=False, or one lane)")
        return self.update(dets, counts)


class _CallableModule(type(ctypes)):
    """`yolo_hip.track` is this module as soon as it is imported, and the package also exports the
    function of that name: calling the module calls the function."""

    def __call__(self, *args, **kwargs):
        return track(*args, **kwargs)


import sys  # noqa: E402
sys.modules[__name__].__class__ = _CallableModule
