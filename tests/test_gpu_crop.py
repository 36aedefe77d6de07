"""yh_crop_rois on the device (marked gpu): the kernel against its host twin bit for bit on the
cases of _crop_cases.py - mixed BGR / NV12 batches larger than one launch, host- and
device-resident frames, boxes as they lie in a (B, max_det, 6) tensor - the sweep of rectangle
sizes (the device's double-precision geometry), out= reuse, empty calls, and
Detector.predict(keep_frames=True) -> crop_rois end to end. The host twin is pinned to the numpy
restatement in test_crop_host.py.
"""
import numpy as np
import pytest
import torch

import _crop_cases as cc
from yolo_hip import preprocess as pre
from yolo_hip import synth
from yolo_hip.detect import Detector

pytestmark = pytest.mark.gpu

SIZES = ((32, 16), (24, 40), (16, 8))


def _host(case, size, keep_aspect, pad, capacity=None, frames=None):
    c = pre.crop_rois(frames or cc.lib_frames(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["counts"]),
                      size, keep_aspect=keep_aspect, pad=pad, capacity=capacity, threads=4)
    return c.data.numpy(), c.rois.numpy(), c.total.numpy()


def _mixed(case, gpu):
    """The case's frames, every second one already on the device."""
    host, dev = cc.lib_frames(case), cc.lib_frames(case, gpu)
    return [d if k % 2 == 0 else h for k, (h, d) in enumerate(zip(host, dev))]


def _same(c, want):
    got = (c.data.cpu().numpy(), c.rois.cpu().numpy(), c.total.cpu().numpy())
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("keep_aspect", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_device_crops_match_host_twin(gpu, size, keep_aspect):
    case = cc.build(*size, batch=37, max_rois=8)          # two launches
    cc.assert_coverage(case, *size, want_area=size == (32, 16))
    frames = _mixed(case, gpu)
    assert any(isinstance(f, np.ndarray) for f in frames) and any(isinstance(f, torch.Tensor) for f in frames)
    assert {f.device.type for f in frames if isinstance(f, pre.NV12)} == {"cpu", "cuda"}
    boxes, counts = torch.from_numpy(case["boxes"]).to(gpu), torch.from_numpy(case["counts"]).to(gpu)
    assert boxes.shape == (37, 8, 6)                      # box_stride 6: the rows of Detections.dets
    for pad in (0.0, 0.1, 0.5):
        want = _host(case, size, keep_aspect, pad)
        out = (torch.full((37 * 8, 3) + size, 0xAB, dtype=torch.uint8, device=gpu),      # every byte is written
               torch.full((37 * 8, 6), -1, dtype=torch.int32, device=gpu), torch.full((1,), -1, dtype=torch.int32, device=gpu))
        c = pre.crop_rois(frames, boxes, counts, size, keep_aspect=keep_aspect, pad=pad, out=out)
        assert c.data is out[0]
        assert 0 < int(want[2][0]) < 37 * 8
        assert _same(c, want), (size, keep_aspect, pad)
    # a capacity below the total drops the last rows; at 100 the frames of the second launch own none
    for capacity in (int(want[2][0]) - 3, 100):
        fresh = pre.crop_rois(frames, boxes, counts, size, keep_aspect=keep_aspect, pad=0.5, capacity=capacity)
        assert fresh.data.shape == (capacity, 3) + size
        assert _same(fresh, _host(case, size, keep_aspect, 0.5, capacity=capacity))


@pytest.mark.parametrize("size", [(64, 64), (32, 16), (72, 68)])    # (72, 68): 1224 groups, the fifth chunk partly filled
def test_sixteen_rois_per_frame_on_device_frames(gpu, size):
    case = cc.build(*size)                                # batch 8, max_rois 16
    boxes, counts = torch.from_numpy(case["boxes"]).to(gpu), torch.from_numpy(case["counts"]).to(gpu)
    for keep_aspect in (False, True):
        c = pre.crop_rois(cc.lib_frames(case, gpu), boxes, counts, size, keep_aspect=keep_aspect, pad=0.1)
        assert _same(c, _host(case, size, keep_aspect, 0.1))


@pytest.mark.parametrize("keep_aspect", [False, True])
def test_sweep_of_rectangle_sizes(gpu, keep_aspect):
    """200 integer rectangle sizes: lb_geometry / lb_finish in the device's fp64 give the host's bits."""
    case = cc.sweep()
    boxes, counts = torch.from_numpy(case["boxes"]).to(gpu), torch.from_numpy(case["counts"]).to(gpu)
    for size in ((32, 16), (24, 40), (20, 28)):
        c = pre.crop_rois(cc.lib_frames(case, gpu), boxes, counts, size, keep_aspect=keep_aspect)
        want = _host(case, size, keep_aspect, 0.0)
        assert want[2][0] == 200 and _same(c, want), size


def test_out_reuse_with_fewer_rois_zeroes_the_tail(gpu):
    size = (24, 40)
    case = cc.build(*size, batch=6, max_rois=8)
    frames = cc.lib_frames(case, gpu)
    boxes = torch.from_numpy(case["boxes"]).to(gpu)
    c = pre.crop_rois(frames, boxes, torch.from_numpy(case["counts"]).to(gpu), size)
    n = int(c.total[0])
    assert c.data[:n].any() and c.rois[n - 1].any()
    fewer = dict(case, counts=np.array([2, 0, 1, 0, 3, 0], np.int32))
    again = pre.crop_rois(frames, boxes, torch.from_numpy(fewer["counts"]).to(gpu), size, out=tuple(c))
    assert again.data is c.data and int(again.total[0]) == 6 < n
    assert _same(again, _host(fewer, size, False, 0.0))
    assert not again.data[6:].any() and not again.rois[6:].any()


def test_empty_calls(gpu):
    size = (16, 8)
    case = cc.build(*size, batch=3, max_rois=4)
    frames = cc.lib_frames(case, gpu)
    boxes, counts = torch.from_numpy(case["boxes"]).to(gpu), torch.from_numpy(case["counts"]).to(gpu)
    c = pre.crop_rois(frames, boxes, counts, size, capacity=0)
    assert c.data.shape == (0, 3, 16, 8) and c.rois.shape == (0, 6) and int(c.total[0]) == 0
    out = (torch.full((5, 3, 16, 8), 0xAB, dtype=torch.uint8, device=gpu),
           torch.full((5, 6), -1, dtype=torch.int32, device=gpu), torch.full((1,), -1, dtype=torch.int32, device=gpu))
    c = pre.crop_rois([], boxes[:0], counts[:0], size, capacity=5, out=out)
    assert int(c.total[0]) == 0 and not c.data.any() and not c.rois.any()
    c = pre.crop_rois([], boxes[:0], counts[:0], size)
    assert c.data.shape == (0, 3, 16, 8) and int(c.total[0]) == 0
    assert c.gather(boxes[:0, :, 5]).shape == (0,)


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
    input is needed)."""
    bgr = _scene_bgr(h, w, seed).numpy().astype(np.float64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    uv = np.stack((u[0::2, 0::2], v[0::2, 0::2]), -1).reshape(h // 2, w)
    return pre.NV12(np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8))


def test_detector_keep_frames_then_crop(gpu, engine):
    canvas, max_det = (256, 384), 20
    nv, bgr = _scene_nv12(324, 576, 61), _scene_bgr(432, 768, 62)
    det = Detector(engine, batch=4, canvas=canvas, conf=0.001, iou=0.65, max_det=max_det)
    plain = det.predict([nv, bgr])
    assert plain.frames is None
    res = det.predict([nv, bgr], keep_frames=True)
    assert torch.equal(res.dets, plain.dets) and torch.equal(res.counts, plain.counts)    # the default is unchanged
    assert isinstance(res.frames[0], pre.NV12) and res.frames[0].device == gpu and res.frames[1].device == gpu
    counts = res.counts.cpu()
    assert int(counts.sum()) > 0
    for size, keep_aspect, pad in (((32, 16), False, 0.0), ((64, 64), True, 0.1)):
        c = pre.crop_rois(res.frames, res.dets, res.counts, size, keep_aspect=keep_aspect, pad=pad)
        host = pre.crop_rois([nv, bgr.numpy()], res.dets.cpu(), counts, size, keep_aspect=keep_aspect, pad=pad)
        assert _same(c, (host.data.numpy(), host.rois.numpy(), host.total.numpy()))
        n = int(c.total[0])
        assert n == int(counts.sum()) and c.data[:n].any()
        want = torch.cat([res.dets[i, :k, 5] for i, k in enumerate(counts.tolist())])
        assert torch.equal(c.gather(res.dets[..., 5])[:n], want)
        assert [(crop.shape, roi[:2]) for crop, roi in c.tolist()[:1]] == [((3,) + size, (int(c.rois[0, 0]), 0))]
