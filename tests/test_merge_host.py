"""yh_merge_host (csrc/merge_host.cpp) through yolo_hip.detect.merge on CPU tensors: the map-back
and the cross-tile merge against the numpy restatement (tests/_merge_cases.py), exactly, on the
whole `out` and `out_counts`; the round trip through the letterbox transform; the argument errors.
"""
import ctypes

import numpy as np
import pytest
import torch

import _merge_cases as mc
from yolo_hip import _lib
from yolo_hip.detect import merge, tile_transform
from yolo_hip.preprocess import geometry


def run_host(c, threads=0):
    N = c["image_wh"].shape[0]
    out = torch.full((N, c["max_out"], 6), -7.0)                   # reused buffers: every byte is written
    cnt = torch.full((N,), -7, dtype=torch.int32)
    got = merge(c["dets"], c["counts"], c["tile_xf"], c["tile_offsets"], c["image_wh"], c["max_tiles"], iou=c["iou"],
                max_out=c["max_out"], out=(out, cnt), threads=threads)
    assert got[0] is out and got[1] is cnt
    return out.numpy(), cnt.numpy()


@pytest.mark.parametrize("name", mc.ALL)
def test_merge_host_equals_restatement(name):
    c = mc.case(name)
    out, cnt = run_host(c)
    assert np.isfinite(out).all()                                   # the NaN padding rows were never read
    assert np.array_equal(cnt, c["want"][1])
    assert np.array_equal(out, c["want"][0])


def test_single_tile_is_the_clipped_inverse_letterbox():
    c = mc.case("single")
    out, cnt = run_host(c)
    assert cnt.tolist() == [23, 23, 23]                             # 25 rows, 2 dropped (border padding, zero width)
    for i, (W, H) in enumerate(c["image_wh"].tolist()):
        k = cnt[i]
        b = out[i, :k]
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= W).all() and (b[:, 3] <= H).all()
        assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
        assert b[1, 0] == 0 and b[1, 1] == 0 and b[2, 2] == W and b[2, 3] == H      # the two clipped rows
        assert np.array_equal(b[:3, 4], np.float32([0.9, 0.8, 0.95]))               # input order, not score order
        assert not out[i, k:].any()
    # 480 x 640 on a 320 canvas: scale 2, top border 40
    assert np.array_equal(out[0, 0, :4], np.float32([20.5, 41.0, 201.5, 180.0]))
    # 320 x 320 on a 320 canvas: the identity
    assert np.array_equal(out[1, 0, :4], c["dets"][1, 0, :4].numpy())


def test_object_in_the_overlap_comes_out_once():
    c = mc.case("overlap_once")
    assert c["tile_offsets"].tolist() == [0, 4] and c["counts"].tolist() == [3, 2, 1, 1]   # seen 2, 4 and 1 times
    out, cnt = run_host(c)
    assert cnt.tolist() == [3]
    assert sorted(out[0, :3, 5].tolist()) == [0.0, 1.0, 2.0]


def test_chain_suppressed_box_does_not_suppress():
    out, cnt = run_host(mc.case("chain"))
    assert cnt.tolist() == [2]
    assert np.array_equal(out[0, :2, 0], np.float32([0, 60]))       # A and C; B was killed by A


def test_equal_boxes_of_other_classes_survive():
    out, cnt = run_host(mc.case("classes"))
    assert cnt.tolist() == [3]
    assert out[0, :3, 4:].tolist() == [[np.float32(0.9), 0.0], [np.float32(0.8), 1.0], [np.float32(0.6), 2.0]]


def test_equal_scores_keep_the_lower_position():
    """All scores equal: the walk order is the input order, so the kept rows are a subsequence of
    the mapped input rows."""
    c = mc.case("ties")
    out, cnt = run_host(c)
    md = c["dets"].shape[1]
    for i in range(2):
        lo, hi = c["tile_offsets"][i:i + 2].tolist()
        rows = np.concatenate([mc.map_rows(c["dets"][t, :int(c["counts"][t])].numpy(), c["tile_xf"][t].numpy(),
                                           *c["image_wh"][i].tolist())[0] for t in range(lo, hi)], 0)
        at = 0
        for r in out[i, :cnt[i]]:
            while not np.array_equal(rows[at], r):
                at += 1
            at += 1
        assert 0 < cnt[i] < len(rows) and md == 64


def test_round_trip_through_the_letterbox_transform():
    """Source boxes pushed through the forward letterbox transform in float64 and mapped back return
    within 4 * 2**-24 * max(W, H): one rounding each for the subtract, the multiply, sx itself and
    the add, each at most half an ulp of a value no larger than max(W, H). (The canvas coordinates
    are multiples of 1/64, so their own cast to fp32 is exact.)"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for (H, W, crop, size) in ((333, 500, (0, 0, 500, 333), 320), (480, 640, (0, 0, 640, 480), 320),
                               (2160, 3840, (3200, 1520, 640, 640), 640), (2160, 3840, (0, 0, 3840, 2160), 640),
                               (700, 1000, (477, 211, 517, 489), 640)):
        f = tile_transform(crop, size)
        x0, y0, w, h = crop
        nh, nw, top, left = geometry(h, w, size)
        k = 200
        # canvas points on a 1/64 grid inside the resized crop; the source box is their preimage
        # under the exact scale w / nw (float64), so the forward transform lands back on the grid
        cx = np.sort(np.round(rng.uniform(left + 0.1, left + nw - 0.1, size=(k, 2)) * 64) / 64, 1)
        cy = np.sort(np.round(rng.uniform(top + 0.1, top + nh - 0.1, size=(k, 2)) * 64) / 64, 1)
        ok = (cx[:, 1] - cx[:, 0] > 1) & (cy[:, 1] - cy[:, 0] > 1)
        cx, cy = cx[ok], cy[ok]
        src = np.stack(((cx[:, 0] - left) * (w / nw) + x0, (cy[:, 0] - top) * (h / nh) + y0,
                        (cx[:, 1] - left) * (w / nw) + x0, (cy[:, 1] - top) * (h / nh) + y0), 1)     # float64
        assert (src >= 0).all() and (src[:, [0, 2]] <= W).all() and (src[:, [1, 3]] <= H).all()
        canvas = np.stack(((src[:, 0] - x0) * (nw / w) + left, (src[:, 1] - y0) * (nh / h) + top,
                           (src[:, 2] - x0) * (nw / w) + left, (src[:, 3] - y0) * (nh / h) + top), 1)  # forward
        rows = np.concatenate([canvas, np.full((len(src), 1), 0.5), np.zeros((len(src), 1))], 1)
        c = mc.pack([(W, H, [(f, rows)])], len(src), max_out=len(src))
        assert np.abs(c["dets"][0, :, :4].numpy().astype(np.float64) - canvas).max() < 1e-9   # the fp32 cast is exact
        out, cnt = run_host(c)
        assert cnt[0] == len(src)
        err = np.abs(out[0, :, :4].astype(np.float64) - src).max()
        worst = max(worst, err / max(W, H))
        assert err <= 4 * 2.0 ** -24 * max(W, H), (crop, err)
    assert worst > 0


def test_threads_give_the_same_bytes():
    for name in ("mixed", "ties", "total_257"):
        a, ac = run_host(mc.case(name), threads=1)
        b, bc = run_host(mc.case(name), threads=4)
        assert a.tobytes() == b.tobytes() and ac.tobytes() == bc.tobytes()


def test_default_buffers_and_max_out_zero():
    c = mc.case("mixed")
    out, cnt = merge(c["dets"], c["counts"], c["tile_xf"], c["tile_offsets"], c["image_wh"], c["max_tiles"],
                     iou=c["iou"], max_out=c["max_out"])
    assert np.array_equal(out.numpy(), c["want"][0]) and np.array_equal(cnt.numpy(), c["want"][1])
    out, cnt = merge(c["dets"], c["counts"], c["tile_xf"], c["tile_offsets"], c["image_wh"], c["max_tiles"], max_out=0)
    assert out.shape == (4, 0, 6) and cnt.tolist() == [0, 0, 0, 0]


def test_bad_arguments_are_einval():
    lib = _lib.lib()
    t = torch.zeros((64,))
    p = ctypes.c_void_p(t.data_ptr())
    cap = _lib.MERGE_MAX_CAND

    def call(dets=p, counts=p, tiles=1, md=4, xf=p, off=p, wh=p, images=1, max_tiles=1, max_out=2, out=p, oc=p):
        return lib.yh_merge_host(dets, counts, tiles, md, xf, off, wh, images, max_tiles, 0.5, max_out, out, oc, 1)

    assert call() == 0
    for kw, word in ((dict(tiles=-1), b"tiles"), (dict(md=-1), b"max_det"), (dict(images=-1), b"images"),
                     (dict(max_out=-1), b"max_out"), (dict(max_tiles=0), b"max_tiles"),
                     (dict(max_tiles=cap // 4 + 1), b"YH_MERGE_MAX_CAND"), (dict(md=cap + 1), b"YH_MERGE_MAX_CAND"),
                     (dict(dets=None), b"null"), (dict(counts=None), b"null"), (dict(xf=None), b"null"),
                     (dict(off=None), b"null"), (dict(wh=None), b"null"), (dict(out=None), b"null"),
                     (dict(oc=None), b"null")):
        assert call(**kw) == -1, kw                                 # YH_EINVAL
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())
    assert call(max_tiles=cap // 4) == 0                            # exactly at the cap
    with pytest.raises(RuntimeError, match="YH_MERGE_MAX_CAND"):
        c = mc.case("chain")
        merge(c["dets"], c["counts"], c["tile_xf"], c["tile_offsets"], c["image_wh"], cap)


def test_merge_rejects_mistyped_misplaced_and_strided_tensors():
    c = mc.case("total_256")
    names = ("dets", "counts", "tile_xf", "tile_offsets", "image_wh")
    args = [c[k] for k in names]
    T, md = c["dets"].shape[:2]
    strided = [torch.zeros((T, md, 12))[:, :, ::2], torch.zeros((2 * T,), dtype=torch.int32)[::2],
               torch.zeros((T, 12))[:, ::2], torch.zeros((4,), dtype=torch.int32)[::2], torch.zeros((1, 4))[:, ::2]]
    for i, bad in enumerate(strided):
        assert bad.shape == args[i].shape and not bad.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            merge(*args[:i], bad, *args[i + 1:], c["max_tiles"])
    wrong = [args[0].double(), args[1].long(), args[2].half(), args[3].long(), args[4].double()]
    for i, bad in enumerate(wrong):
        with pytest.raises(TypeError, match=names[i]):
            merge(*args[:i], bad, *args[i + 1:], c["max_tiles"])
    for i in range(1, 5):                                            # a tensor on another device than dets
        with pytest.raises(ValueError, match="expected cpu"):
            merge(*args[:i], args[i].to("meta"), *args[i + 1:], c["max_tiles"])
    with pytest.raises(ValueError, match="shape"):
        merge(args[0], args[1][:-1].contiguous(), *args[2:], c["max_tiles"])
    with pytest.raises(ValueError, match="shape"):
        merge(*args, c["max_tiles"], out=(torch.zeros((1, 5, 6)), torch.zeros((1,), dtype=torch.int32)), max_out=4)
    with pytest.raises(ValueError, match="contiguous"):
        merge(*args, c["max_tiles"], out=(torch.zeros((1, 4, 12))[:, :, ::2], torch.zeros((1,), dtype=torch.int32)),
              max_out=4)
