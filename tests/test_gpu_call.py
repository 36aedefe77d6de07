"""The device branch of the wrappers' one fork (yolo_hip/_call.py) hands the library the *current*
stream of the tensors' device. Every converted wrapper runs once inside `with torch.cuda.stream(s)`
and once on the default stream, on the smallest inputs, and must give the host twin's bytes, state
included.

What makes the first run a test of the stream: s first sleeps, and the inputs reach the device by
asynchronous copies from pinned memory queued on s behind the sleep. A kernel launched on s reads
them after they arrive; one launched on the default stream would not wait for s and would read
memory the copies have not filled yet. The rest of the suite runs on the default stream only and
cannot tell the two apart. What such a kernel would find there is whatever the side stream's pool
held before: fresh memory for the first case, and for the later ones the blocks of earlier cases,
whose inputs differ from case to case (other shapes, other values), so stale bytes do not pass for
this case's inputs. `torch.cuda._sleep` is private to torch; it is what holds the copies back.
"""
import numpy as np
import pytest
import torch

import yolo_hip
from yolo_hip import metrics
from yolo_hip import motion as ym
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu
f32, i32, u8, i8 = torch.float32, torch.int32, torch.uint8, torch.int8
SLEEP_CYCLES = 20_000_000   # some milliseconds to some tenths of a second, whatever clock the counter reads


def _rng():
    return np.random.default_rng(7)


def _dets():
    # 1 stream x 2 rows: two separate boxes above track_high, classes 0 and 1
    return dict(dets=torch.tensor([[[4, 4, 20, 24, 0.9, 0], [30, 8, 50, 40, 0.8, 1]]], dtype=f32),
                counts=torch.tensor([2], dtype=i32))


def _track():
    return dict(_dets(), state=yt.track_state(1, 2))


def _track_reid():
    e = torch.from_numpy(_rng().standard_normal((2, 64)).astype(np.float32))
    return dict(_dets(), state=yt.track_state(1, 2, reid_dim=64), embed=e)


def _warp():
    kw = _track()
    yolo_hip.track(**kw)                                   # a state with two tracks in it
    return dict(state=kw["state"], motion=torch.tensor([[1.25, 3.0, -2.0]], dtype=f32), max_tracks=2)


def _assign():
    return dict(weights=torch.tensor([[[5, 9], [7, 3]]], dtype=i32))


def _quantize():
    return dict(e=torch.from_numpy(_rng().standard_normal((2, 64)).astype(np.float32)))


def _int8(*shape):
    return torch.from_numpy(_rng().integers(-128, 128, shape, dtype=np.int8))


def _similarity():
    return dict(a=_int8(1, 1, 64), b=_int8(1, 1, 64).flip(-1))


def _search():
    g = _int8(64, 64)
    return dict(gallery=g, q=g[17:18].clone(), k=1, labels=torch.arange(64, dtype=i32), size=torch.tensor([64], dtype=i32))


def _enrol():
    return dict(gallery=torch.zeros((64, 64), dtype=i8), labels=torch.full((64,), -1, dtype=i32),
                size=torch.zeros((1,), dtype=i32), q=_int8(1, 64), next_label=torch.tensor([5], dtype=i32))


def _merge():
    xf = torch.tensor([[float(v) for v in yolo_hip.tile_transform((0, 0, 64, 48), 32)]], dtype=f32)
    return dict(_dets(), tile_xf=xf, tile_offsets=torch.tensor([0, 1], dtype=i32),
                image_wh=torch.tensor([[64.0, 48.0]], dtype=f32), max_tiles=1, max_out=2)


def _match():
    return dict(_dets(), labels=torch.tensor([[0, 5, 5, 20, 24]], dtype=f32), offsets=torch.tensor([0, 1], dtype=i32),
                iou_v=torch.tensor([0.5], dtype=f32))


def _crop():
    frame = torch.from_numpy(_rng().integers(0, 256, (8, 8, 3), dtype=np.uint8))
    return dict(frames=[frame], boxes=torch.tensor([[[1, 1, 7, 6]]], dtype=f32), counts=torch.tensor([1], dtype=i32),
                size=(4, 4))


def _motion(model):
    big = torch.from_numpy(_rng().integers(0, 256, (7, 9), dtype=np.uint8)).float()
    big = torch.nn.functional.interpolate(big[None, None], size=(28, 36), mode="bilinear")[0, 0].to(u8)
    first = big[2:26, 2:34, None].expand(24, 32, 3).contiguous()
    second = big[0:24, 4:36, None].expand(24, 32, 3).contiguous()     # the camera moved by (-2, 2)
    kw = dict(frames=[first, second], state=ym.motion_state(1, (12, 16)), thumb=(12, 16), radius=2, model=model)
    if model == "similarity":
        kw.update(grid=(1, 1), min_blocks=2, field=torch.zeros((1, 1, 4), dtype=i32))
    return kw


def _estimate_two(frames, **kw):
    """Two frames of one stream: the second call's motion is measured against the first's thumbnail."""
    ym.estimate(frames[:1], **kw)
    return ym.estimate(frames[1:], **kw)


CASES = [
    ("track", yolo_hip.track, _track),
    ("track_reid", yolo_hip.track_reid, _track_reid),
    ("warp", yt.warp, _warp),
    ("assign", yolo_hip.assign, _assign),
    ("embed_quantize", yolo_hip.embed_quantize, _quantize),
    ("embed_similarity", yolo_hip.embed_similarity, _similarity),
    ("gallery_search", yolo_hip.gallery_search, _search),
    ("gallery_enrol", yolo_hip.gallery_enrol, _enrol),
    ("merge", yolo_hip.merge, _merge),
    ("match_batch", metrics.match_batch, _match),
    ("crop_rois", yolo_hip.crop_rois, _crop),
    ("motion", _estimate_two, lambda: _motion("translation")),
    ("motion_field", _estimate_two, lambda: _motion("similarity")),
]
IDS = [c[0] for c in CASES]


def tensors(kw, ret):
    """Every tensor a call can have written: what it returned and, for the states it advances in place,
    what it was given."""
    out = [t for t in (ret if isinstance(ret, tuple) else (ret,)) if isinstance(t, torch.Tensor)]
    return out + [v for k, v in sorted(kw.items()) if isinstance(v, torch.Tensor)]


def host_result(call, make):
    kw = make()
    return tensors(kw, call(**kw))


def device_result(call, make, dev, stream):
    """The call with its inputs copied to the device on `stream`, behind a sleep when it is a side stream."""
    kw = {k: v.pin_memory() if isinstance(v, torch.Tensor) else v for k, v in make().items()}
    if "frames" in kw:                                   # host frames: the wrapper copies them itself
        kw["frames"] = [f.pin_memory() for f in kw["frames"]]
    with torch.cuda.stream(stream):
        if stream != torch.cuda.default_stream(dev):
            torch.cuda._sleep(SLEEP_CYCLES)
        kw = {k: v.to(dev, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
        ret = call(**kw)
    stream.synchronize()
    return [t.cpu() for t in tensors(kw, ret)]


@pytest.fixture(scope="module")
def side_stream(gpu):
    return torch.cuda.Stream(gpu)


@pytest.mark.parametrize("name,call,make", CASES, ids=IDS)
def test_a_wrapper_runs_on_the_current_stream_and_gives_the_host_twins_bytes(gpu, side_stream, name, call, make):
    want = host_result(call, make)
    assert any(t.any() for t in want[:1]) or name == "gallery_enrol", "the case's result is all zeros: no teeth"
    for stream in (side_stream, torch.cuda.default_stream(gpu)):
        got = device_result(call, make, gpu, stream)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (name, k, str(stream))


def test_the_device_workspace_of_the_similarity_model_takes_the_shared_check(gpu):
    """`motion.estimate` reads `workspace` on the device path only; like its other tensors it is
    judged by the wrappers' one check, and its size by motion's own sentence."""
    kw = _motion("similarity")
    kw = {k: v.to(gpu) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    frames = kw.pop("frames")[:1]
    with pytest.raises(TypeError) as info:
        ym.estimate(frames, workspace=torch.zeros((4096,), dtype=torch.int32, device=gpu), **kw)
    assert str(info.value) == "yolo_hip.motion: workspace must be torch.uint8, got torch.int32"
    need = ym.field_workspace(1, (1, 1), 2, gpu).numel()
    with pytest.raises(ValueError) as info:
        ym.estimate(frames, workspace=torch.zeros((need - 1,), dtype=u8, device=gpu), **kw)
    assert str(info.value) == (f"yolo_hip.motion: workspace must be a contiguous uint8 tensor of at least {need} bytes "
                               f"on {gpu}")
