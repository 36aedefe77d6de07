"""yh_hota_eval_host against TrackEval's float64 HOTA (tests/_hota_cases.py). No GPU.

Bars. TP, FP, FN and the row counts are integers on both sides and must be equal. With equal matchings
the integer rules differ from float64 only by their truncations:
  LocA   each matched similarity is truncated by less than 2^-16, so is their mean;
  AssA, AssRe, AssPr   each identity pair's term is floored by less than 2^-20, there are PAIRS of them
         and the sum is divided by TP: e_A = 2^-20 PAIRS / TP;
  HOTA(a) = sqrt(DetA AssA) with DetA exact: |sqrt(D A) - sqrt(D A')| = D |A - A'| / (sqrt(D A) +
         sqrt(D A')) <= D e_A / sqrt(D A_ref) = e_A sqrt(D / A_ref); the mean over the thresholds is
         held to the mean of these bounds.
The association bars and what follows from them get 8 float64 ulps of the value on top for the
reference's own roundings; the LocA bar is strict.
"""
import numpy as np
import pytest
import torch

import _hota_cases as hc

ULPS = 8 * np.finfo(np.float64).eps


@pytest.mark.parametrize("name", list(hc.cases()))
def test_host_twin_meets_the_float64_reference(name):
    from yolo_hip.mot import hota_ratios
    c = hc.cases()[name]
    ref, rows, ign = hc.reference(name)
    out, got_rows, got_ign = hc.run_lib(c, "cpu", 1)
    again = hc.run_lib(c, "cpu", 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((out, got_rows, got_ign), again)), "threads differ"
    assert np.array_equal(got_rows, rows) and np.array_equal(got_ign, ign)
    r = hota_ratios(out)
    for s, want in enumerate(ref):
        tp, fp, fn, pairs = out[s, :, 0], out[s, :, 1], out[s, :, 2], out[s, :, 7]
        assert np.array_equal(tp, want["tp"]) and np.array_equal(fp, want["fp"]) and np.array_equal(fn, want["fn"])
        assert np.array_equal(pairs, want["pairs"])
        live = tp > 0
        assert np.isnan(r["hota_alpha"][s][~live]).all()
        assert np.isnan(r["hota"][s]) == (not live.all())      # the mean is a number iff every threshold is
        if not live.any():
            continue
        e_a = 2.0 ** -20 * pairs[live] / tp[live]
        err = lambda k: np.abs(r[k][s][live] - want[k][live])
        assert (err("loca") < 2.0 ** -16).all()
        for k in ("assa", "assre", "asspr"):
            assert (err(k) <= e_a + ULPS * want[k][live]).all(), k
        e_h = e_a * np.sqrt(want["deta"][live] / want["assa"][live]) + ULPS
        assert (err("hota_alpha") <= e_h).all()
        # the mean over the thresholds that matched something (all of them where "hota" is a number)
        assert abs(np.nanmean(r["hota_alpha"][s]) - want["hota_alpha"][live].mean()) <= e_h.mean()
        if live.all():
            assert abs(r["hota"][s] - want["hota_alpha"].mean()) <= e_h.mean()


def test_bad_arguments_are_refused():
    from yolo_hip import _lib
    lib = _lib.lib()
    z = lambda *s, dtype=torch.int32: torch.zeros(s, dtype=dtype)
    tr, ti, tc, gt, gi, gc = z(1, 1, 4, 6, dtype=torch.float32), z(1, 1, 4), z(1, 1), z(1, 1, 4, 5, dtype=torch.float32), z(1, 1, 4), z(1, 1)
    thr, out, rows, ign = torch.tensor([0.5]), z(1, 1, 8, dtype=torch.int64), z(1, 2, dtype=torch.int64), z(1, 2)
    p = lambda t: None if t is None else t.data_ptr()

    def call(max_out=4, max_gt=4, S=1, F=1, num_thr=1, ng=4, nt=4, ca=1, thr=thr, out=out, rows=rows, tr=tr):
        return lib.yh_hota_eval_host(p(tr), p(ti), p(tc), max_out, p(gt), p(gi), p(gc), max_gt, S, F, None, p(thr), num_thr,
                                     ng, nt, ca, p(out), p(rows), p(ign), 1)

    assert call() == 0
    for bad in (dict(max_out=257), dict(max_gt=257), dict(ng=1025), dict(nt=1025), dict(F=65536), dict(num_thr=0),
                dict(num_thr=33), dict(S=-1), dict(max_gt=-1), dict(ca=2), dict(thr=None), dict(out=None), dict(rows=None),
                dict(tr=None)):
        assert call(**bad) == -1 and b"hota_eval" in lib.yh_last_error(), bad
    # per sequence: P, n_g, n_t, the levels, 8 (6 num_thr + 4) bytes of counters and the ticket, each padded to 16
    assert lib.yh_hota_workspace_bytes(2, 3, 5, 7) == 2 * (144 + 32 + 32 + 432 + 192)
    assert lib.yh_hota_workspace_bytes(1, 19, 64, 64) == 329152 and lib.yh_hota_workspace_bytes(1, 32, 1024, 1024) == 138421808
    assert lib.yh_hota_workspace_bytes(1, 33, 5, 7) == 0
    # the device entry checks its workspace before anything is launched
    args = (p(tr), p(ti), p(tc), 4, p(gt), p(gi), p(gc), 4, 1, 1, None, p(thr), 1, 4, 4, 1, p(out), p(rows), p(ign))
    assert lib.yh_hota_eval(*args, p(gt), 16, None) == -1 and b"workspace too small" in lib.yh_last_error()
    assert lib.yh_hota_eval(*args, p(gt) + 4, 1 << 20, None) == -1 and b"aligned" in lib.yh_last_error()
