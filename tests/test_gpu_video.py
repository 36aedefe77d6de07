"""Video front end on the device (yh_letterbox_frames; marked gpu): the kernel against its host
twin bit for bit on mixed BGR / NV12 batches larger than one launch, BGR on a square canvas
against yh_letterbox, and Detector(canvas=...) with NV12 frames against the hand composition
letterbox_frames -> Engine.forward -> nms -> merge. The host twin is pinned to the numpy
restatement in test_video_host.py.
"""
import numpy as np
import pytest
import torch

import _video_cases as vc
from yolo_hip import preprocess as pre
from yolo_hip import synth
from yolo_hip.detect import Detector, merge, tile_transform

pytestmark = pytest.mark.gpu

CONF, IOU, MAX_DET = 0.001, 0.65, 300


def _mixed_frames(n, gpu):
    """n frames over vc.SHAPES (+ two odd-sized BGR ones): BGR and NV12 of both matrices, tight and
    strided, host and device sources -> [(frame for the device call, the same frame on the host)]"""
    shapes = vc.SHAPES + ((17, 23), (33, 101))
    out = []
    for i in range(n):
        h, w = shapes[i % len(shapes)]
        kind = (i // len(shapes) + i) % 3
        on_device = i % 2 == 0
        if kind == 0 or h % 2 or w % 2:
            wide = np.zeros((h, w + 5 * (i // 2 % 2), 3), np.uint8)
            wide[:, :w] = vc.bgr_image(h, w, 100 + i)
            host = wide[:, :w]
            dev = torch.from_numpy(wide).to(gpu)[:, :w] if on_device else host
        else:
            y, uv = vc.nv12_planes(h, w, 200 + i, pad=4 * (i % 3))
            matrix = 601 if kind == 1 else 709
            host = pre.NV12(y, uv, matrix)
            if on_device:   # keep the row strides on the device: move the wide buffers, then slice
                yb = torch.from_numpy(np.ascontiguousarray(np.pad(y, ((0, 0), (0, 4 * (i % 3)))))).to(gpu)
                ub = torch.from_numpy(np.ascontiguousarray(np.pad(uv, ((0, 0), (0, 4 * (i % 3)))))).to(gpu)
                dev = pre.NV12(yb[:, :w], ub[:, :w], matrix)
                assert dev.y.stride(0) == w + 4 * (i % 3)
            else:
                dev = host
        out.append((dev, host))
    return out


@pytest.mark.parametrize("canvas", vc.CANVASES)
def test_device_frames_match_host_twin(gpu, canvas):
    frames = _mixed_frames(37, gpu)                       # two launches
    kinds = [isinstance(d, pre.NV12) for d, _ in frames]
    assert any(kinds) and not all(kinds)
    assert {d.matrix for d, _ in frames if isinstance(d, pre.NV12)} == {601, 709}
    want = np.stack([pre.letterbox_frames_host(h, canvas, threads=1 + k % 2 * 3) for k, (_, h) in enumerate(frames)])
    out = torch.full((37, 3) + canvas, 0xAB, dtype=torch.uint8, device=gpu)     # every byte is written
    got = pre.letterbox_frames([d for d, _ in frames], canvas, device=gpu, out=out)
    assert got is out
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    for k, (_, h) in enumerate(frames):                   # the border is zero
        nh, nw, top, left = pre.geometry(h.height if isinstance(h, pre.NV12) else h.shape[0],
                                         h.width if isinstance(h, pre.NV12) else h.shape[1], canvas)
        border = np.ones(canvas, bool)
        border[top:top + nh, left:left + nw] = False
        assert not got[k][:, border].any()
    # out= reuse with other frames overwrites everything, a fresh tensor gives the same bytes
    again = pre.letterbox_frames([d for d, _ in frames[::-1]], canvas, device=gpu, out=out)
    assert np.array_equal(again.cpu().numpy(), want[::-1])
    fresh = pre.letterbox_frames([d for d, _ in frames[:5]], canvas)
    assert fresh.shape == (5, 3) + canvas and np.array_equal(fresh.cpu().numpy(), want[:5])
    assert pre.letterbox_frames([], canvas, device=gpu).shape == (0, 3) + canvas


@pytest.mark.parametrize("size", [64, 320])
def test_bgr_on_a_square_canvas_is_letterbox(gpu, size):
    rng = np.random.default_rng(size)
    shapes = [(480, 640), (640, 427), (17, 23), (size, size), (2 * size, 2 * size), (33, 1000), (50, 70)]
    imgs = [torch.from_numpy(rng.integers(0, 256, s + (3,), dtype=np.uint8)).to(gpu) for s in shapes]
    want = pre.letterbox(imgs, size)
    assert torch.equal(pre.letterbox_frames(imgs, size), want)
    assert torch.equal(pre.letterbox_frames(imgs, (size, size)), want)
    assert np.array_equal(want[2].cpu().numpy(), pre.letterbox_host(imgs[2].cpu().numpy(), size))


@pytest.fixture(scope="module")
def engine(gpu):
    from nets import nn
    from yolo_hip.engine import Engine
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    eng = Engine(*model._yh_arch, gpu, torch.bfloat16)
    eng.load_module(model.eval())
    return eng


def _scene_bgr(h, w, seed):
    x = synth.synth_scenes(1, h, w, seed=seed)[0]                                 # (3, h, w) RGB in [0, 1]
    return (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()


def _scene_nv12(h, w, seed):
    """A synthetic scene as limited-range NV12 (BT.601 forward transform in float; only a plausible
    input is needed, the conversion under test is the library's)."""
    bgr = _scene_bgr(h, w, seed).numpy().astype(np.float64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    uv = np.stack((u[0::2, 0::2], v[0::2, 0::2]), -1).reshape(h // 2, w)
    return pre.NV12(np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8))


def _compose(engine, gpu, x, xfs, whs, batch):
    """x (n, 3, H, W) uint8 canvases -> merge(nms(forward)) with one tile per image, padded to `batch`."""
    from yolo_hip.engine import nms
    n = x.shape[0]
    xp = torch.zeros((batch,) + tuple(x.shape[1:]), dtype=torch.uint8, device=gpu)
    xp[:n] = x
    d, c = nms(engine.forward(xp), confidence_threshold=CONF, iou_threshold=IOU, max_det=MAX_DET)
    xf = torch.zeros((batch, 6), dtype=torch.float32)
    xf[:n] = torch.from_numpy(np.asarray(xfs, np.float32))
    off = torch.arange(n + 1, dtype=torch.int32)
    wh = torch.tensor(whs, dtype=torch.float32)
    return merge(d.contiguous(), c.contiguous(), xf.to(gpu), off.to(gpu), wh.to(gpu), 1, iou=IOU, max_out=MAX_DET)


def test_detector_on_a_rectangular_canvas_with_nv12(gpu, engine):
    canvas = (256, 384)
    nv = _scene_nv12(324, 576, 61)
    bgr = _scene_bgr(432, 768, 62)
    assert pre.geometry(324, 576, canvas) == (216, 384, 20, 0)
    assert pre.geometry(432, 768, canvas) == (216, 384, 20, 0)                    # exact 2x
    det = Detector(engine, batch=4, canvas=canvas, conf=CONF, iou=IOU, max_det=MAX_DET)
    res = det.predict([nv, bgr])
    x = pre.letterbox_frames([nv, bgr], canvas, device=gpu)
    want, wcnt = _compose(engine, gpu, x, [tile_transform((0, 0, 576, 324), canvas), tile_transform((0, 0, 768, 432), canvas)],
                          [[576, 324], [768, 432]], 4)
    assert res.dets.shape == (2, MAX_DET, 6) and int(wcnt.sum()) > 0
    assert torch.equal(res.counts, wcnt) and res.dets.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    d0 = res.dets[0, :int(res.counts[0])].cpu().numpy()                           # source pixels of the NV12 frame
    assert (d0[:, :2] >= 0).all() and (d0[:, 2] <= 576).all() and (d0[:, 3] <= 324).all()
    # the NV12 frame == the BGR frame the host conversion makes of it
    as_bgr = det.predict([pre.nv12_to_bgr_host(nv), bgr])
    assert torch.equal(as_bgr.counts, res.counts) and torch.equal(as_bgr.dets, res.dets)
    with pytest.raises(ValueError, match="NV12"):
        Detector(engine, batch=4, canvas=canvas, tile=256).predict([nv])
    with pytest.raises(ValueError, match="32"):
        Detector(engine, batch=4, canvas=(250, 384))


def test_detector_without_canvas_is_unchanged(gpu, engine):
    size = 320
    shapes = ((416, 544), (320, 320), (200, 300))
    images = [_scene_bgr(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    res = Detector(engine, size=size, batch=4, conf=CONF, iou=IOU, max_det=MAX_DET).predict(images)
    x = pre.letterbox([im.to(gpu) for im in images], size)
    want, wcnt = _compose(engine, gpu, x, [tile_transform((0, 0, w, h), size) for h, w in shapes],
                          [[w, h] for h, w in shapes], 4)
    assert int(wcnt.sum()) > 0
    assert torch.equal(res.counts, wcnt) and res.dets.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # an NV12 frame on the square canvas goes through letterbox_frames at (size, size)
    nv = _scene_nv12(200, 300, 63)
    r2 = Detector(engine, size=size, batch=4, conf=CONF, iou=IOU, max_det=MAX_DET).predict([nv])
    r3 = Detector(engine, size=size, batch=4, conf=CONF, iou=IOU, max_det=MAX_DET).predict([pre.nv12_to_bgr_host(nv)])
    assert torch.equal(r2.counts, r3.counts) and torch.equal(r2.dets, r3.dets)
