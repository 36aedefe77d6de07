"""Video front end on the host: yh_letterbox_geometry2, yh_nv12_to_bgr_host and
yh_letterbox_frames_host (the twin of the kernel, same per-pixel code) against the numpy
restatement in _video_cases.py, bit for bit; the argument errors; rect_canvas, tile_transform on
a rectangular canvas and NV12.from_packed. The device kernel is pinned to the host twin in
test_gpu_video.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import _video_cases as vc
from oracle import preprocess as opre
from yolo_hip import _lib
from yolo_hip import preprocess as pre
from yolo_hip.detect import tile_transform


def test_square_geometry_is_the_old_geometry():
    """The grid of test_preprocess.py::test_geometry_matches_restatement: (s, s) == s == the restatement."""
    for h in (1, 2, 31, 320, 427, 479, 480, 481, 639, 640, 641, 1000, 1279, 4000):
        for w in (1, 3, 64, 333, 640, 853, 1280, 3000):
            for s in (32, 320, 640, 1280):
                want = opre.geometry(h, w, s)
                if min(want[:2]) < 1:
                    with pytest.raises(RuntimeError):
                        pre.geometry(h, w, (s, s))
                    continue
                assert pre.geometry(h, w, (s, s)) == want == pre.geometry(h, w, s), (h, w, s)
                old = [ctypes.c_int() for _ in range(4)]
                assert _lib.lib().yh_letterbox_geometry(h, w, s, *[ctypes.byref(v) for v in old]) == 0
                assert tuple(v.value for v in old) == want


def test_rectangular_geometry_matches_restatement():
    assert pre.geometry(1080, 1920, (384, 640)) == (360, 640, 12, 0)
    assert pre.geometry(720, 1280, (384, 640)) == (360, 640, 12, 0)      # the exact 2x path
    assert pre.geometry(1920, 1080, (640, 384)) == (640, 360, 0, 12)     # portrait
    for h in (2, 31, 360, 479, 480, 720, 1080, 1081, 1920, 4000):
        for w in (3, 64, 333, 640, 853, 1280, 1920, 3000):
            for c in ((384, 640), (640, 384), (32, 64), (256, 384), (640, 640), (1280, 736)):
                want = vc.geometry(h, w, *c)
                if min(want[:2]) < 1:
                    with pytest.raises(RuntimeError, match="below 1"):
                        pre.geometry(h, w, c)
                    continue
                assert pre.geometry(h, w, c) == want, (h, w, c)


@pytest.mark.parametrize("matrix", [601, 709])
def test_nv12_to_bgr_host_bit_exact_vs_restatement(matrix):
    cases = [vc.corner_planes(), vc.nv12_planes(36, 64, 1), vc.nv12_planes(50, 70, 2, pad=6), vc.nv12_planes(2, 2, 3)]
    sweep = np.zeros((32, 512), np.uint8)           # every Y against a sweep of U (per column pair) and V (per row)
    sweep[:, 0::2] = np.arange(256)[None, :]
    sweep[:, 1::2] = (np.arange(32) * 8 + 3)[:, None]
    cases.append((np.tile(np.repeat(np.arange(256), 2).astype(np.uint8), (64, 1)), sweep))
    for y, uv in cases:
        got = pre.nv12_to_bgr_host(pre.NV12(y, uv, matrix))
        assert got.shape == y.shape + (3,) and got.dtype == np.uint8
        assert np.array_equal(got, vc.nv12_to_bgr(y, uv, matrix))
        # 2^-20 coefficient rounding moves a sum of at most three products of |factor| <= 239 by
        # 3 * 239 * 2^-21 < 4e-4 of a level: at most one level after rounding, never more
        assert np.abs(got.astype(np.float64) - vc.nv12_to_bgr_float(y, uv, matrix)).max() <= 1


def test_nv12_corner_values():
    y, uv = vc.corner_planes()
    got = pre.nv12_to_bgr_host(pre.NV12(y, uv, 601))
    assert (got[:, 0:2, 0] == 0).all()                       # Y 0, U 0: blue saturates low
    k = 2 * (1 * 9 + 1 * 3 + 1)                              # Y 16, U 128, V 128: black
    assert (got[:, k:k + 2] == 0).all()
    k = 2 * (2 * 9 + 1 * 3 + 1)                              # Y 235, neutral chroma: white
    assert (got[:, k:k + 2] == 255).all()


def _frames(h, w, seed):
    """name -> (frame for the library, its BGR image for the restatement)"""
    out = {}
    img = vc.bgr_image(h, w, seed)
    out["bgr"] = (img, img)
    wide = np.zeros((h, w + 5, 3), dtype=np.uint8)
    wide[:, :w] = img
    out["bgr_strided"] = (wide[:, :w], img)
    if h % 2 == 0 and w % 2 == 0:
        for matrix, pad in ((601, 0), (709, 3)):
            y, uv = vc.nv12_planes(h, w, seed + matrix, pad)
            out[f"nv12_{matrix}"] = (pre.NV12(y, uv, matrix), vc.nv12_to_bgr(y, uv, matrix))
    return out


@pytest.mark.parametrize("canvas", vc.CANVASES)
@pytest.mark.parametrize("h,w", vc.SHAPES)
def test_letterbox_frames_host_bit_exact_vs_restatement(h, w, canvas):
    nh, nw, top, left = vc.geometry(h, w, *canvas)
    if (h, w, canvas) == (50, 70, (64, 96)):
        assert (nw, left) == (89, 3)
    if (h, w, canvas) == (128, 192, (64, 96)):
        assert (nh, nw) == (64, 96)
    for name, (frame, bgr) in _frames(h, w, 7 * h + w).items():
        want = vc.letterbox(bgr, *canvas)
        for threads in (1, 4):
            got = pre.letterbox_frames_host(frame, canvas, threads=threads)
            assert got.shape == (3,) + canvas and got.dtype == np.uint8
            assert np.array_equal(got, want), (name, h, w, canvas, threads)
        if name.startswith("nv12"):     # the composition rule, through the library's own conversion
            assert np.array_equal(pre.letterbox_frames_host(pre.nv12_to_bgr_host(frame), canvas), want)


def test_square_canvas_is_letterbox_host():
    for h, w in vc.SHAPES + ((17, 23), (33, 100)):
        img = vc.bgr_image(h, w, 5)
        assert np.array_equal(pre.letterbox_frames_host(img, 64), pre.letterbox_host(img, 64))
        assert np.array_equal(pre.letterbox_frames_host(img, (64, 64)), opre.letterbox(img, 64))


def _frame(**kw):
    y = np.zeros((4, 8), np.uint8)
    uv = np.zeros((2, 8), np.uint8)
    f = dict(plane0=y.ctypes.data, plane1=uv.ctypes.data, height=4, width=8, stride0=0, stride1=0,
             format=_lib.YH_PIX_NV12, matrix=_lib.YH_YUV_BT601)
    f.update(kw)
    return _lib.YhFrame(**f), (y, uv)


@pytest.mark.parametrize("kw,msg", [
    (dict(height=3), "even"), (dict(width=7), "even"),
    (dict(stride0=7), "stride"), (dict(stride1=6), "stride"),
    (dict(format=_lib.YH_PIX_BGR, stride0=23), "stride"),
    (dict(plane0=None), "plane0"), (dict(plane1=None), "plane1"),
    (dict(format=2), "format"), (dict(matrix=2), "matrix"), (dict(format=-1), "format"),
    (dict(height=4000, width=2), "below 1"),
])
def test_error_returns(kw, msg):
    L = _lib.lib()
    f, keep = _frame(**kw)
    dst = np.zeros((3, 32, 32), np.uint8)
    rc = L.yh_letterbox_frames_host(ctypes.byref(f), 32, 32, dst.ctypes.data, 1)
    assert rc == -1 and msg in L.yh_last_error().decode()
    # the device entry point validates before it touches the device: same code without a GPU
    rc = L.yh_letterbox_frames(ctypes.byref(f), 1, 32, 32, dst.ctypes.data, None)
    assert rc == -1 and msg in L.yh_last_error().decode()
    if kw.get("format", _lib.YH_PIX_NV12) == _lib.YH_PIX_NV12 and "below" not in msg:
        out = np.zeros((4, 8, 3), np.uint8)
        assert L.yh_nv12_to_bgr_host(ctypes.byref(f), out.ctypes.data) == -1
    assert not dst.any()


def test_more_error_returns():
    L = _lib.lib()
    f, keep = _frame()
    dst = np.zeros((3, 32, 32), np.uint8)
    assert L.yh_letterbox_frames_host(ctypes.byref(f), 32, 32, dst.ctypes.data, 1) == 0
    assert L.yh_letterbox_frames(ctypes.byref(f), 1, 32, 30, dst.ctypes.data, None) == -1
    assert "multiple of 4" in L.yh_last_error().decode()
    assert L.yh_letterbox_frames(ctypes.byref(f), 1, 0, 32, dst.ctypes.data, None) == -1
    assert L.yh_letterbox_frames(None, 1, 32, 32, dst.ctypes.data, None) == -1
    assert L.yh_letterbox_frames_host(None, 32, 32, dst.ctypes.data, 1) == -1
    assert L.yh_letterbox_frames_host(ctypes.byref(f), 32, 32, None, 1) == -1
    bgr, _ = _frame(format=_lib.YH_PIX_BGR)
    assert L.yh_nv12_to_bgr_host(ctypes.byref(bgr), dst.ctypes.data) == -1
    assert L.yh_abi_version() == 7
    with pytest.raises(ValueError):
        pre.NV12(np.zeros((3, 4), np.uint8), np.zeros((1, 4), np.uint8))
    with pytest.raises(ValueError):
        pre.NV12(np.zeros((4, 4), np.uint8), np.zeros((2, 4), np.uint8), matrix=2020)


def test_rect_canvas():
    assert pre.rect_canvas(1080, 1920) == (384, 640)
    assert pre.rect_canvas(720, 1280) == (384, 640)
    assert pre.rect_canvas(1920, 1080) == (640, 384)
    assert pre.rect_canvas(640, 640) == (640, 640)
    assert pre.rect_canvas(480, 640, size=320) == (256, 320)
    assert pre.rect_canvas(1080, 1920, size=1280, stride=64) == (768, 1280)
    assert pre.rect_canvas(10, 4000) == (32, 640)
    for h, w in ((1080, 1920), (480, 640), (333, 1000), (1000, 333), (17, 23)):
        c = pre.rect_canvas(h, w)
        nh, nw, top, left = pre.geometry(h, w, c)
        assert (nh, nw) == opre.geometry(h, w, 640)[:2]      # the square canvas's resize, fewer border rows
        assert c[0] % 32 == 0 and c[1] % 32 == 0 and c[0] - nh < 32 and c[1] - nw < 32
    with pytest.raises(ValueError):
        pre.rect_canvas(0, 10)


def test_tile_transform_on_a_rectangular_canvas():
    xf = tile_transform((5, 7, 1920, 1080), (384, 640))
    assert all(isinstance(v, np.float32) for v in xf)
    assert xf == (np.float32(3.0), np.float32(3.0), np.float32(0), np.float32(12), np.float32(5), np.float32(7))
    assert tile_transform((0, 0, 300, 200), (320, 320)) == tile_transform((0, 0, 300, 200), 320)
    nh, nw, top, left = vc.geometry(90, 40, 64, 96)
    assert tile_transform((0, 0, 40, 90), (64, 96)) == (np.float32(40) / np.float32(nw), np.float32(90) / np.float32(nh),
                                                        np.float32(left), np.float32(top), np.float32(0), np.float32(0))


def test_nv12_from_packed():
    rng = np.random.default_rng(0)
    buf = rng.integers(0, 256, (54, 64), dtype=np.uint8)       # 36 Y rows + 18 UV rows
    f = pre.NV12.from_packed(buf, 36, 64, matrix=709)
    assert (f.height, f.width, f.matrix) == (36, 64, 709)
    assert f.y.data_ptr() == buf.ctypes.data and f.uv.data_ptr() == buf.ctypes.data + 36 * 64   # views
    assert np.array_equal(pre.nv12_to_bgr_host(f), vc.nv12_to_bgr(buf[:36], buf[36:], 709))
    g = pre.NV12.from_packed(torch.from_numpy(buf), 36, 64)
    assert np.array_equal(pre.letterbox_frames_host(g, (64, 96)),
                          vc.letterbox(vc.nv12_to_bgr(buf[:36], buf[36:], 601), 64, 96))
    with pytest.raises(ValueError):
        pre.NV12.from_packed(buf, 36, 62)
    with pytest.raises(ValueError):
        pre.NV12.from_packed(buf[:53], 35, 64)
