"""yh_crop_rois_host (the twin of the kernel, same per-pixel and geometry code) against the numpy
restatement in _crop_cases.py, bit for bit; the composition with the already pinned
letterbox_frames_host / resize_linear_host / nv12_to_bgr_host; capacity, threads, the argument
errors and Crops.gather. The device kernel is pinned to the host twin in test_gpu_crop.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import _crop_cases as cc
from oracle import preprocess as opre
from yolo_hip import _lib
from yolo_hip import preprocess as pre

# (32, 16): a 48-byte row, all vector (vtail 48), and the area path from a 64 x 32 rectangle;
# (24, 40): wider than high, a 120-byte row with an 8-byte scalar tail; (64, 64): square, larger
# than most frames; (16, 8): a 24-byte row, vector up to byte 16 and scalar after it
SIZES = ((32, 16), (24, 40), (64, 64), (16, 8))


def twin(case, size, keep_aspect, pad, capacity=None, threads=1, out=None):
    c = pre.crop_rois(cc.lib_frames(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["counts"]), size,
                      keep_aspect=keep_aspect, pad=pad, capacity=capacity, threads=threads, out=out)
    assert isinstance(c, pre.Crops)
    return c.data.numpy(), c.rois.numpy(), c.total.numpy()


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def test_tail_rule_of_the_sizes():
    assert opre.vtail(3 * 16) == 48 and opre.vtail(3 * 8) == 16 and opre.vtail(3 * 40) == 112


@pytest.mark.parametrize("size", SIZES)
def test_cases_cover_every_branch(size):
    cc.assert_coverage(cc.build(*size), *size, want_area=size == (32, 16))


@pytest.mark.parametrize("pad", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("keep_aspect", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_host_twin_bit_exact_vs_restatement(size, keep_aspect, pad):
    case = cc.build(*size)
    want = cc.expected(case, *size, keep_aspect, pad)
    got = twin(case, size, keep_aspect, pad)
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert same(got, want)
    M = case["boxes"].shape[1]
    assert want[2][0] == sum(min(max(int(n), 0), M) for n in case["counts"])
    live = want[1][:want[2][0], 4] > 0
    assert live.any() and not live.all()
    if pad == 0.0 and keep_aspect:    # a 60 x 1 (120 x 1) rectangle has no geometry: it keeps its slot, empty
        rects = [rc for _, rc, _ in cc.valid_rects(case, 0.0)]
        ks = [i for i, rc in enumerate(rects) if rc is not None and cc.geometry_fails(rc[3], rc[2], *size)]
        assert any(rects[k][3] == 1 and rects[k][2] in (60, 120) for k in ks)
        assert all(tuple(got[1][k, 2:]) == (0, 0, 0, 0) and not got[0][k].any() for k in ks)


@pytest.mark.parametrize("keep_aspect", [False, True])
def test_sweep_of_rectangle_sizes(keep_aspect):
    case = cc.sweep()
    assert case["counts"][0] == 200
    for size in ((32, 16), (24, 40)):
        assert same(twin(case, size, keep_aspect, 0.0, threads=0), cc.expected(case, *size, keep_aspect, 0.0))


@pytest.mark.parametrize("size", [(32, 16), (24, 40)])
def test_capacity_and_every_byte_written(size):
    case = cc.build(*size)
    total = int(cc.expected(case, *size, False, 0.1)[2][0])
    for capacity in (total - 9, total, total + 5, 0):
        for keep_aspect in (False, True):
            want = cc.expected(case, *size, keep_aspect, 0.1, capacity)
            assert want[2][0] == min(total, capacity)
            out = (torch.full((capacity, 3) + size, 0xAB, dtype=torch.uint8),
                   torch.full((capacity, 6), 0x2B2B2B2B, dtype=torch.int32), torch.full((1,), -7, dtype=torch.int32))
            got = twin(case, size, keep_aspect, 0.1, capacity=capacity, out=out)
            assert got[0].ctypes.data == out[0].numpy().ctypes.data or capacity == 0
            assert same(got, want)
            if capacity > total:
                assert not got[0][total:].any() and not got[1][total:].any()


@pytest.mark.parametrize("size", [(32, 16), (24, 40), (16, 8)])
def test_threads_do_not_change_the_result(size):
    case = cc.build(*size, batch=11, max_rois=8)
    for keep_aspect in (False, True):
        one = twin(case, size, keep_aspect, 0.1, threads=1)
        assert same(twin(case, size, keep_aspect, 0.1, threads=4), one)
        assert same(twin(case, size, keep_aspect, 0.1, threads=0), one)
        assert same(twin(case, size, keep_aspect, 0.1, threads=1000), one)


@pytest.mark.parametrize("size", [(32, 16), (24, 40), (16, 8)])
def test_composition_through_the_pinned_host_calls(size):
    """Step 3 through the library's own letterbox, resize and conversion, run on the view."""
    case = cc.build(*size)
    frames = cc.lib_frames(case)
    bgr = [pre.nv12_to_bgr_host(f) if isinstance(f, pre.NV12) else np.ascontiguousarray(f) for f in frames]
    for b, img in enumerate(bgr):
        assert np.array_equal(img, case["bgr"][b])
    for keep_aspect in (False, True):
        data, rois, total = twin(case, size, keep_aspect, 0.0)
        seen = 0
        for s in range(int(total[0])):
            b, r, x0, y0, w, h = (int(v) for v in rois[s])
            if w == 0:
                assert h == 0 and not data[s].any()
                continue
            view = np.ascontiguousarray(bgr[b][y0:y0 + h, x0:x0 + w])
            if keep_aspect:
                want = pre.letterbox_frames_host(view, size)
            else:
                want = np.ascontiguousarray(pre.resize_linear_host(view, *size).transpose(2, 0, 1)[::-1])
            assert np.array_equal(data[s], want), (s, b, r, x0, y0, w, h)
            seen += 1
        assert seen > 20


def _raw(**kw):
    """Arguments of yh_crop_rois_host for one 4 x 8 NV12 frame and one box, with overrides."""
    y, uv = np.zeros((4, 8), np.uint8), np.zeros((2, 8), np.uint8)
    f = dict(plane0=y.ctypes.data, plane1=uv.ctypes.data, height=4, width=8, stride0=0, stride1=0,
             format=_lib.YH_PIX_NV12, matrix=_lib.YH_YUV_BT601)
    f.update(kw.pop("frame", {}))
    frame = _lib.YhFrame(**f)
    boxes = np.array([[[1, 1, 5, 3]]], np.float32)
    counts = np.array([1], np.int32)
    crops = np.full((2, 3, 8, 8), 0xAB, np.uint8)
    rois = np.full((2, 6), -1, np.int32)
    total = np.full((1,), -1, np.int32)
    a = dict(frames=ctypes.pointer(frame), batch=1, boxes=boxes.ctypes.data, box_stride=4, counts=counts.ctypes.data,
             max_rois=1, out_h=8, out_w=8, keep_aspect=0, pad=0.0, capacity=2, crops=crops.ctypes.data,
             rois=rois.ctypes.data, total=total.ctypes.data)
    a.update(kw)
    return list(a.values()), (y, uv, frame, boxes, counts, crops, rois, total)


@pytest.mark.parametrize("kw,msg", [
    (dict(batch=-1), "negative"), (dict(max_rois=-1), "negative"), (dict(capacity=-1), "negative"),
    (dict(out_h=0), "out_h"), (dict(out_h=-3), "out_h"),
    (dict(out_w=0), "out_w"), (dict(out_w=2), "out_w"), (dict(out_w=10), "multiple of 4"), (dict(out_w=-4), "out_w"),
    (dict(box_stride=3), "box_stride"), (dict(box_stride=0), "box_stride"),
    (dict(pad=-0.1), "pad"), (dict(pad=float("nan")), "pad"), (dict(pad=float("inf")), "pad"),
    (dict(keep_aspect=2), "keep_aspect"), (dict(keep_aspect=-1), "keep_aspect"),
    (dict(frames=None), "NULL"), (dict(boxes=None), "NULL"), (dict(counts=None), "NULL"),
    (dict(crops=None), "NULL"), (dict(rois=None), "NULL"), (dict(total=None), "NULL"),
    (dict(frame=dict(height=3)), "even"), (dict(frame=dict(stride0=7)), "stride"),
    (dict(frame=dict(plane0=None)), "plane0"), (dict(frame=dict(plane1=None)), "plane1"),
    (dict(frame=dict(format=2)), "format"), (dict(frame=dict(matrix=2)), "matrix"),
    (dict(frame=dict(format=_lib.YH_PIX_BGR, height=0)), "positive"),
])
def test_error_returns(kw, msg):
    L = _lib.lib()
    args, keep = _raw(**kw)
    crops, rois, total = keep[5:]
    rc = L.yh_crop_rois_host(*args, 1)
    assert rc == -1 and msg in L.yh_last_error().decode(), L.yh_last_error().decode()
    # the device entry point validates before it touches the device: same code without a GPU
    rc = L.yh_crop_rois(*args, None)
    assert rc == -1 and msg in L.yh_last_error().decode()
    assert (crops == 0xAB).all() and (rois == -1).all() and total[0] == -1


def test_valid_edge_arguments():
    L = _lib.lib()
    args, keep = _raw()
    crops, rois, total = keep[5:]
    assert L.yh_crop_rois_host(*args, 1) == 0
    assert total[0] == 1 and tuple(rois[0]) == (0, 0, 1, 1, 4, 2) and not rois[1].any() and not crops[1].any()
    args, keep = _raw(batch=0, frames=None, boxes=None, counts=None)
    crops, rois, total = keep[5:]
    assert L.yh_crop_rois_host(*args, 1) == 0
    assert total[0] == 0 and not crops.any() and not rois.any()
    args, keep = _raw(capacity=0, crops=None, rois=None)
    assert L.yh_crop_rois_host(*args, 1) == 0 and keep[7][0] == 0
    assert L.yh_abi_version() == 7


def test_python_checks():
    case = cc.build(32, 16, batch=3, max_rois=4)
    frames, boxes, counts = cc.lib_frames(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["counts"])
    with pytest.raises(TypeError, match="counts"):
        pre.crop_rois(frames, boxes, counts.long(), (32, 16))
    with pytest.raises(TypeError, match="boxes"):
        pre.crop_rois(frames, boxes.double(), counts, (32, 16))
    with pytest.raises(ValueError, match="contiguous"):
        pre.crop_rois(frames, boxes[:, :, :5], counts, (32, 16))
    with pytest.raises(ValueError, match="frames"):
        pre.crop_rois(frames[:2], boxes, counts, (32, 16))
    with pytest.raises(ValueError, match="counts"):
        pre.crop_rois(frames, boxes, counts[:2], (32, 16))
    with pytest.raises(ValueError, match="out data"):
        pre.crop_rois(frames, boxes, counts, (32, 16), out=(torch.zeros((12, 3, 32, 32), dtype=torch.uint8),
                                                            torch.zeros((12, 6), dtype=torch.int32),
                                                            torch.zeros((1,), dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        pre.crop_rois(frames, boxes, counts, (32, 18))
    import yolo_hip
    assert yolo_hip.crop_rois is pre.crop_rois and yolo_hip.Crops is pre.Crops
    c = pre.crop_rois(frames, boxes, counts, 16)     # an int is a square crop
    assert tuple(c.data.shape) == (12, 3, 16, 16)


def test_gather_and_tolist():
    case = cc.build(24, 40, batch=5, max_rois=4)
    boxes = torch.from_numpy(case["boxes"])
    c = pre.crop_rois(cc.lib_frames(case), boxes, torch.from_numpy(case["counts"]), (24, 40))
    n = int(c.total[0])
    assert 0 < n < c.rois.shape[0]
    cls = c.gather(boxes[..., 5])
    assert cls.shape == (c.rois.shape[0],)
    want = [case["boxes"][b, r, 5] for b, r in c.rois[:n, :2].tolist()]
    assert cls[:n].tolist() == want
    assert (cls[n:] == boxes[0, 0, 5]).all()
    assert torch.equal(c.gather(boxes)[:n, :4], torch.stack([boxes[b, r, :4] for b, r in c.rois[:n, :2].tolist()]))
    lst = c.tolist()
    assert len(lst) == n and lst[0][1] == tuple(c.rois[0].tolist()) and torch.equal(lst[-1][0], c.data[n - 1])
    assert c.gather(torch.zeros((0, 4, 6))).shape == (c.rois.shape[0], 6)
