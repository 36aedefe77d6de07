"""The argument checks every handle-free wrapper makes before it calls the library, wrapper by
wrapper and tensor by tensor: not a tensor, wrong dtype, wrong device, wrong shape, not contiguous -
the exception type and the whole message; a call with every tensor on `meta`, which no wrapper
serves; and the rule for stream ids given on the host. The wrappers share one check, one device /
host fork and one stream-id rule (yolo_hip/_call.py); this table is what they have to keep saying.
CPU only: every case fails before the library is called, or runs the host twin on a tiny input.

Rows marked ADOPTED are the checks of `motion.estimate` that took the shared check's wording (and
TypeError for "not a tensor" and a wrong dtype) when the wrappers were folded; every other row also
holds for the wrappers as they were before, and so does all else here but the last test, the
refusal `letterbox_frames` got when it took the shared device branch.
"""
from collections import namedtuple

import pytest
import torch

import yolo_hip
from yolo_hip import gallery as yg
from yolo_hip import metrics
from yolo_hip import motion as ym
from yolo_hip import track as yt

f32, i32, u8, i8 = torch.float32, torch.int32, torch.uint8, torch.int8
KINDS = ("not a tensor", "dtype", "device", "shape", "contiguous")
ADOPTED = "adopted"


def z(*shape, dt=f32):
    return torch.zeros(shape, dtype=dt)


# key: the keyword, or (keyword, position) inside a tuple argument; want: the shape as the message
# prints it; over: kind -> (exception, message) where the wrapper answers before or instead of the
# shared check, or None where the malformation cannot be told from another legal call
Arg = namedtuple("Arg", "key name want dtype over note", defaults=({}, ""))
Wrapper = namedtuple("Wrapper", "id who call make args")


def lead(who, name, sentence, device_victim, **more):
    """The overrides of the tensor a wrapper takes its sizes and its device from: its own sentence when
    it is no tensor of the right rank; on another device, the next tensor is the one out of place."""
    own = (ValueError, f"{who}: {name} {sentence}")
    over = {"not a tensor": own, "shape": own,
            "device": (ValueError, f"{who}: {device_victim} is on cpu, expected meta")}
    over.update(more)
    return over


def _merge():
    return dict(dets=z(2, 2, 6), counts=z(2, dt=i32), tile_xf=z(2, 6), tile_offsets=torch.tensor([0, 1, 2], dtype=i32),
                image_wh=z(2, 2), max_tiles=1, max_out=2, out=(z(2, 2, 6), z(2, dt=i32)))


def _match():
    return dict(dets=z(2, 2, 6), counts=z(2, dt=i32), labels=z(2, 5), offsets=torch.tensor([0, 1, 2], dtype=i32),
                iou_v=z(2), out=z(2, 2, 2, dt=u8), score_cls=z(2, 2, 2), counts_out=z(2, dt=i32))


def _crop():
    return dict(frames=[z(8, 8, 3, dt=u8), z(8, 8, 3, dt=u8)], boxes=z(2, 2, 4), counts=z(2, dt=i32), size=(4, 4),
                out=(z(4, 3, 4, 4, dt=u8), z(4, 6, dt=i32), z(1, dt=i32)))


def _track(reid=False):
    kw = dict(dets=z(2, 2, 6), counts=z(2, dt=i32), state=yt.track_state(2, 2, reid_dim=64 if reid else None),
              stream_ids=torch.tensor([0, 1], dtype=i32), out=(z(2, 2, 6), z(2, 2, dt=i32), z(2, 2, dt=i32), z(2, dt=i32)))
    if reid:
        kw.update(embed=z(4, 64), feat_counts=z(2, dt=i32), embed_total=z(1, dt=i32),
                  workspace=yt.reid_workspace(2, 2, 2, 64))
    return kw


def _warp():
    return dict(state=yt.track_state(2, 2), motion=z(2, 3), max_tracks=2, stream_ids=torch.tensor([0, 1], dtype=i32))


def _assign():
    return dict(weights=z(2, 2, 2, dt=i32), t_counts=z(2, dt=i32), d_counts=z(2, dt=i32),
                out=(z(2, 2, dt=i32), z(2, 2, dt=i32)))


def _quantize():
    return dict(e=z(2, 64), count=z(1, dt=i32), out=z(2, 64, dt=i8))


def _similarity():
    return dict(a=z(2, 2, 64, dt=i8), b=z(2, 2, 64, dt=i8), a_index=z(2, dt=i32), out=z(2, 2, 2, dt=i32))


def _search():
    return dict(gallery=z(64, 64, dt=i8), q=z(2, 64, dt=i8), k=1, labels=z(64, dt=i32), size=z(1, dt=i32),
                count=z(1, dt=i32), out=(z(2, 1, dt=i32), z(2, 1, dt=i32)), workspace=yg.gallery_workspace(64, 2, 1))


def _enrol():
    return dict(gallery=z(64, 64, dt=i8), labels=z(64, dt=i32), size=z(1, dt=i32), q=z(2, 64, dt=i8),
                take=z(2, dt=i32), labels_in=z(2, dt=i32), next_label=z(1, dt=i32), count=z(1, dt=i32), out=z(2, dt=i32))


def _motion(model="translation"):
    kw = dict(frames=[z(24, 32, 3, dt=u8), z(24, 32, 3, dt=u8)], state=ym.motion_state(2, (12, 16)), thumb=(12, 16),
              radius=2, stream_ids=torch.tensor([0, 1], dtype=i32), out=(z(2, 3), z(2, 2, dt=i32)), model=model)
    if model == "similarity":
        kw.update(grid=(1, 1), min_blocks=2, field=z(2, 1, 4, dt=i32))
    return kw


TRACK, GALLERY, MOTION = "yolo_hip.track", "yolo_hip.gallery", "yolo_hip.motion"
_dets = "must be a (B, max_det, 6) tensor"
_frame_rows = [
    Arg("dets", "dets", (2, 2, 6), f32, lead(TRACK, "dets", _dets, "counts")),
    Arg("counts", "counts", (2,), i32),
    Arg("state", "state", ("*", "*"), i32),
    Arg("stream_ids", "stream_ids", (2,), i32),
    Arg(("out", 0), "out dets", (2, 2, 6), f32),
    Arg(("out", 1), "out ids", (2, 2), i32),
    Arg(("out", 2), "out det_index", (2, 2), i32),
    Arg(("out", 3), "out counts", (2,), i32),
]
_matrix = "must be a (rows, dim) tensor"
_gallery_rows = [
    Arg("gallery", "gallery", (64, 64), i8, lead(GALLERY, "gallery", _matrix, "q")),
    Arg("q", "q", (2, 64), i8, {k: (ValueError, f"{GALLERY}: q {_matrix}") for k in ("not a tensor", "shape")}),
    Arg("labels", "labels", (64,), i32),
    Arg("size", "size", (1,), i32),
    Arg("count", "count", (1,), i32),
]
_ab = (ValueError, f"{TRACK}: a must be (nblocks, ra, dim) and b (B, rb, dim)")
_motion_rows = [
    Arg("stream_ids", "stream_ids", (2,), i32, note=ADOPTED),
    Arg(("out", 0), "out motion", (2, 3), f32, note=ADOPTED),
    Arg(("out", 1), "out sad", (2, 2), i32, note=ADOPTED),
]

WRAPPERS = [
    Wrapper("merge", "yolo_hip.merge", yolo_hip.merge, _merge, [
        Arg("dets", "dets", (2, 2, 6), f32, lead("yolo_hip.merge", "dets", "must be a (T, max_det, 6) tensor", "counts")),
        Arg("counts", "counts", (2,), i32),
        Arg("tile_xf", "tile_xf", (2, 6), f32),
        Arg("tile_offsets", "tile_offsets", ("*",), i32),
        Arg("image_wh", "image_wh", (2, 2), f32),
        Arg(("out", 0), "out", (2, 2, 6), f32),
        Arg(("out", 1), "out_counts", (2,), i32)]),
    Wrapper("match_batch", "yolo_hip.match_batch", metrics.match_batch, _match, [
        Arg("dets", "dets", (2, 2, 6), f32, lead("yolo_hip.match_batch", "dets", _dets, "counts")),
        Arg("counts", "counts", (2,), i32),
        Arg("labels", "labels", ("*", 5), f32),
        Arg("offsets", "offsets", (3,), i32),
        Arg("iou_v", "iou_v", ("*",), f32),
        Arg("out", "out", (2, 2, 2), u8),
        Arg("score_cls", "score_cls", (2, 2, 2), f32),
        Arg("counts_out", "counts_out", (2,), i32)]),
    Wrapper("crop_rois", "yolo_hip.crop_rois", yolo_hip.crop_rois, _crop, [
        Arg("boxes", "boxes", (2, 2, 4), f32,
            lead("yolo_hip.crop_rois", "boxes", "must be a (B, max_rois, S) tensor", "counts")),
        Arg("counts", "counts", (2,), i32),
        Arg(("out", 0), "out data", (4, 3, 4, 4), u8),
        Arg(("out", 1), "out rois", (4, 6), i32),
        Arg(("out", 2), "out total", (1,), i32)]),
    Wrapper("track", TRACK, yolo_hip.track, _track, _frame_rows),
    Wrapper("track_reid", TRACK, yolo_hip.track_reid, lambda: _track(reid=True), _frame_rows + [
        Arg("embed", "embed", ("*", 64), f32,
            {k: (ValueError, f"{TRACK}: embed must be a (capacity, dim) tensor") for k in ("not a tensor", "shape")}),
        Arg("feat_counts", "feat_counts", (2,), i32),
        Arg("embed_total", "embed_total", (1,), i32),
        Arg("workspace", "workspace", ("*",), u8)]),
    Wrapper("warp", TRACK, yt.warp, _warp, [
        Arg("motion", "motion", (2, 3), f32, lead(TRACK, "motion", "must be a (B, 3) tensor", "state")),
        Arg("state", "state", ("*", "*"), i32),
        Arg("stream_ids", "stream_ids", (2,), i32)]),
    Wrapper("assign", "yolo_hip.assign", yolo_hip.assign, _assign, [
        Arg("weights", "weights", (2, 2, 2), i32,
            lead("yolo_hip.assign", "weights", "must be a (problems, T, D) tensor", "t_counts")),
        Arg("t_counts", "t_counts", (2,), i32),
        Arg("d_counts", "d_counts", (2,), i32),
        Arg(("out", 0), "out row_of_slot", (2, 2), i32),
        Arg(("out", 1), "out slot_of_row", (2, 2), i32)]),
    Wrapper("embed_quantize", TRACK, yolo_hip.embed_quantize, _quantize, [
        Arg("e", "e", (2, 64), f32, lead(TRACK, "e", _matrix, "count")),
        Arg("count", "count", (1,), i32),
        Arg("out", "out", (2, 64), i8)]),
    Wrapper("embed_similarity", TRACK, yolo_hip.embed_similarity, _similarity, [
        # a may be strided between its blocks: it has checks of its own; its device is the call's
        Arg("a", "a", (2, 2, 64), i8, {
            "not a tensor": _ab, "shape": _ab, "dtype": (TypeError, f"{TRACK}: a must be int8 on b's device"),
            "device": (ValueError, f"{TRACK}: b is on cpu, expected meta"),
            "contiguous": (ValueError, f"{TRACK}: the blocks of a must be contiguous and must not overlap")}),
        Arg("b", "b", (2, 2, 64), i8, {"not a tensor": _ab, "shape": _ab}),
        Arg("a_index", "a_index", (2,), i32),
        Arg("out", "out", (2, 2, 2), i32)]),
    Wrapper("gallery_search", GALLERY, yolo_hip.gallery_search, _search, _gallery_rows + [
        Arg(("out", 0), "out scores", (2, 1), i32),
        Arg(("out", 1), "out index", (2, 1), i32),
        Arg("workspace", "workspace", ("*",), u8)]),
    Wrapper("gallery_enrol", GALLERY, yolo_hip.gallery_enrol, _enrol, _gallery_rows + [
        Arg("take", "take", (2,), i32),
        Arg("labels_in", "labels_in", (2,), i32),
        Arg("next_label", "next_label", (1,), i32),
        Arg("out", "out", (2,), i32)]),
    # the state is motion's own to judge ("must be a motion_state tensor"); the device workspace of the
    # similarity model does not exist on the CPU
    Wrapper("motion", MOTION, ym.estimate, _motion, _motion_rows),
    Wrapper("motion_field", MOTION, ym.estimate, lambda: _motion("similarity"), _motion_rows + [
        Arg("field", "field", (2, 1, 4), i32, note=ADOPTED)]),
]


def malformed(t, kind):
    if kind == "not a tensor":
        return t.tolist()
    if kind == "dtype":
        return t.to(torch.float64)
    if kind == "device":
        return t.to("meta")
    if kind == "shape":
        return t.unsqueeze(-1)
    bad = t.new_zeros(tuple(t.shape) + (2,))[..., 0]     # the same shape over a stride of two
    assert not bad.is_contiguous()
    return bad


def expected(w, arg, kind, bad):
    if kind in arg.over:
        return arg.over[kind]
    head = f"{w.who}: {arg.name}"
    if kind == "shape":
        return ValueError, f"{head} has shape {tuple(bad.shape)}, expected {arg.want}"
    return {"not a tensor": (TypeError, f"{head} must be a tensor"),
            "dtype": (TypeError, f"{head} must be {arg.dtype}, got torch.float64"),
            "device": (ValueError, f"{head} is on meta, expected cpu"),
            "contiguous": (ValueError, f"{head} must be contiguous")}[kind]


def put(kw, key, value):
    if isinstance(key, tuple):
        seq = list(kw[key[0]])
        seq[key[1]] = value
        kw[key[0]] = tuple(seq)
    else:
        kw[key] = value


def get(kw, key):
    return kw[key[0]][key[1]] if isinstance(key, tuple) else kw[key]


def rows():
    for w in WRAPPERS:
        for arg in w.args:
            for kind in KINDS:
                if kind == "contiguous" and all(s == 1 for s in arg.want):
                    continue                             # one element is contiguous whatever its stride: no such case
                tag = f"{w.id}-{arg.name.replace(' ', '_')}-{kind.replace(' ', '_')}"
                yield pytest.param(w, arg, kind, id=tag + ("-" + arg.note if arg.note else ""))


@pytest.mark.parametrize("w", WRAPPERS, ids=[w.id for w in WRAPPERS])
def test_the_smallest_legal_call_runs_the_host_twin(w):
    """The table's arguments are legal as they stand: every malformed row differs from this call in
    one tensor only."""
    w.call(**w.make())


@pytest.mark.parametrize("w,arg,kind", rows())
def test_a_malformed_tensor_is_named_in_the_wrappers_words(w, arg, kind):
    kw = w.make()
    good = get(kw, arg.key)
    assert tuple(good.shape) == tuple(good.shape[i] if s == "*" else s for i, s in enumerate(arg.want)), "the table's shape"
    assert good.dtype == arg.dtype, "the table's dtype"
    bad = malformed(good, kind)
    put(kw, arg.key, bad)
    exc, message = expected(w, arg, kind, bad)
    with pytest.raises(exc) as info:
        w.call(**kw)
    assert type(info.value) is exc and str(info.value) == message


def to_meta(v):
    if isinstance(v, torch.Tensor):
        return v.to("meta")
    if isinstance(v, (tuple, list)) and v and isinstance(v[0], torch.Tensor):
        return type(v)(to_meta(t) for t in v)
    return v


@pytest.mark.parametrize("w", WRAPPERS, ids=[w.id for w in WRAPPERS])
def test_a_device_that_is_neither_cuda_nor_cpu_is_refused(w):
    kw = {k: to_meta(v) for k, v in w.make().items()}
    with pytest.raises(ValueError) as info:
        w.call(**kw)
    assert str(info.value) == f"{w.who}: unsupported device meta"


def _tracker_update(stream_ids, batch):
    yolo_hip.Tracker(2, "cpu", max_tracks=2).update(z(batch, 2, 6), z(batch, dt=i32), stream_ids=stream_ids)


def _estimator_estimate(stream_ids, batch):
    est = ym.MotionEstimator(2, "cpu", thumb=(12, 16), radius=2)
    est.estimate([z(24, 32, 3, dt=u8) for _ in range(batch)], stream_ids=stream_ids)


@pytest.mark.parametrize("who,call,noun", [("yolo_hip.Tracker", _tracker_update, "rows"),
                                           ("yolo_hip.MotionEstimator", _estimator_estimate, "frames")])
def test_stream_ids_given_on_the_host_are_checked_there(who, call, noun):
    for stream_ids, batch, message in (([0, 0], 2, "stream_ids must be distinct"),
                                       ([0, 2], 2, "stream_ids must lie in [0, 2)"),
                                       ((1, -1), 2, "stream_ids must lie in [0, 2)"),
                                       (None, 3, f"a batch of 3 {noun} for 2 streams")):
        with pytest.raises(ValueError) as info:
            call(stream_ids, batch)
        assert str(info.value) == f"{who}: {message}"
    call([1, 0], 2)                                   # a legal host sequence, and a tensor goes through unread
    call(torch.tensor([1, 0], dtype=i32), 2)
    call(None, 2)


def test_letterbox_frames_is_the_device_half_only():
    """It shares the frame walk and the device branch of the fork; its host twin takes one frame and
    has a function of its own (letterbox_frames_host), so a device that is no cuda device is refused
    before anything is walked."""
    from yolo_hip import preprocess as pre
    for device in ("cpu", "meta"):
        with pytest.raises(ValueError) as info:
            pre.letterbox_frames([z(8, 8, 3, dt=u8)], 32, device=device)
        assert str(info.value) == f"letterbox_frames: {device} is no cuda device (letterbox_frames_host is the host twin)"
