"""yh_match_host (csrc/match_host.cpp) through yolo_hip.metrics.match_batch on CPU tensors:
the whole-batch matching against compute_metric per image, exactly, on the reference's
golden set and on tie-heavy random cases (tests/_match_cases.py), plus the argument errors.
"""
import ctypes

import numpy as np
import pytest
import torch

import _match_cases as mc
from yolo_hip import _lib
from yolo_hip.metrics import match_batch


def _run_host(c, threads=0):
    B, md = c["dets"].shape[:2]
    T = c["iou_v"].shape[0]
    tp = torch.full((B, md, T), 0xFF, dtype=torch.uint8)           # the buffer is reused: every byte is written
    sc = torch.full((B, md, 2), -7.0)
    co = torch.full((B,), -7, dtype=torch.int32)
    got = match_batch(c["dets"], c["counts"], c["labels"], c["offsets"], c["iou_v"], out=tp, score_cls=sc,
                      counts_out=co, threads=threads)
    assert got is tp
    return tp, sc, co


def _check_side_outputs(c, sc, co):
    md = c["dets"].shape[1]
    cnt = c["counts"].clamp(0, md)
    assert torch.equal(co, cnt)
    valid = torch.arange(md)[None, :] < cnt[:, None]
    want = torch.where(valid[..., None], c["dets"][:, :, 4:6], torch.zeros(()))
    assert torch.equal(sc, want)


@pytest.mark.parametrize("name", mc.ALL)
def test_match_host_equals_compute_metric(name):
    c = mc.case(name)
    tp, sc, co = _run_host(c)
    assert np.array_equal(tp.numpy(), c["want"].numpy())
    _check_side_outputs(c, sc, co)


def test_golden_is_the_references_answer():
    """tp[b, :D_b] is the reference's `correct_b`, everything beyond is 0."""
    g = mc.load_golden("metrics_synth.npz")
    c = mc.case("golden")
    tp, _, _ = _run_host(c, threads=3)
    for i in range(int(g["n_img"])):
        d = g[f"out_{i}"].shape[0]
        assert np.array_equal(tp[i, :d].numpy().astype(bool), g[f"correct_{i}"]), i
        assert not tp[i, d:].any()


def test_one_label_many_detections_only_first_is_tp():
    c = mc.case("full_one_label")
    tp, _, _ = _run_host(c)
    assert tp[0, 0].all() and not tp[0, 1:].any()


def test_counts_are_clamped_and_optional_outputs_optional():
    c = dict(mc.case("t10_b33_float"))
    md = c["dets"].shape[1]
    c["counts"] = c["counts"].clone()
    c["counts"][0], c["counts"][1] = md + 5, -3
    tp, sc, co = _run_host(c)
    assert co[0] == md and co[1] == 0 and not tp[1].any()
    _check_side_outputs(c, sc, co)
    plain = match_batch(c["dets"], c["counts"], c["labels"], c["offsets"], c["iou_v"])
    assert torch.equal(plain, tp)


def test_single_thread_equals_threaded():
    c = mc.case("t32_b33_grid")
    assert torch.equal(_run_host(c, threads=1)[0], _run_host(c, threads=5)[0])


@pytest.mark.parametrize("num_iou", [0, 33])
def test_num_iou_out_of_range_is_einval(num_iou):
    lib = _lib.lib()
    dets = torch.zeros((1, 4, 6))
    counts = torch.zeros((1,), dtype=torch.int32)
    labels = torch.zeros((0, 5))
    off = torch.zeros((2,), dtype=torch.int32)
    thr = torch.zeros((40,))
    tp = torch.zeros((1, 4, 40), dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.yh_match_host(p(dets), p(counts), 1, 4, p(labels), p(off), p(thr), num_iou, p(tp), None, None, 1)
    assert rc == -1                                                # YH_EINVAL
    assert b"num_iou" in lib.yh_last_error()
    with pytest.raises(RuntimeError, match="num_iou"):
        match_batch(dets, counts, labels, off, thr[:num_iou], out=tp[:, :, :num_iou].contiguous())


def test_bad_sizes_are_einval():
    lib = _lib.lib()
    t = torch.zeros((8,))
    p = ctypes.c_void_p(t.data_ptr())
    for batch, md in ((-1, 4), (1, -1), (1, 4097)):
        assert lib.yh_match_host(p, p, batch, md, p, p, p, 1, p, None, None, 1) == -1
        assert lib.yh_last_error()


def test_non_contiguous_and_mistyped_tensors_raise():
    c = mc.case("t10_b33_float")
    B, md = c["dets"].shape[:2]
    T = c["iou_v"].shape[0]
    args = [c["dets"], c["counts"], c["labels"], c["offsets"], c["iou_v"]]
    strided = [torch.zeros((B, md, 12))[:, :, ::2], torch.zeros((2 * B,), dtype=torch.int32)[::2],
               torch.zeros((c["labels"].shape[0], 10))[:, ::2], torch.zeros((2 * B + 2,), dtype=torch.int32)[::2],
               torch.zeros((2 * T,))[::2]]
    for i, bad in enumerate(strided):
        assert bad.shape == args[i].shape and not bad.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            match_batch(*args[:i], bad, *args[i + 1:])
    for kw, bad in (("out", torch.zeros((B, md, 2 * T), dtype=torch.uint8)[:, :, ::2]),
                    ("score_cls", torch.zeros((B, md, 4))[:, :, ::2]),
                    ("counts_out", torch.zeros((2 * B,), dtype=torch.int32)[::2])):
        with pytest.raises(ValueError, match="contiguous"):
            match_batch(*args, **{kw: bad})
    with pytest.raises(TypeError):
        match_batch(args[0], args[1].long(), *args[2:])
    with pytest.raises(ValueError):
        match_batch(args[0], args[1], args[2], args[3][:-1].contiguous(), args[4])
