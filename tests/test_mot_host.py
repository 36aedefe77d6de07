"""yh_mot_eval_host against the rules restated in tests/_mot_cases.py: every output is an integer, so
the comparison is byte for byte. No GPU."""
import numpy as np
import pytest
import torch

import _mot_cases as mc


@pytest.mark.parametrize("name", list(mc.cases()))
def test_host_twin_equals_the_rules(name):
    want = mc.reference(name)
    for threads in (1, 3):
        got = mc.run_lib(mc.cases()[name], "cpu", threads)
        assert got[0].tobytes() == want[0].tobytes(), f"{name}: counts\n{got[0]}\n{want[0]}"
        assert got[1].tobytes() == want[1].tobytes(), f"{name}: ignored"


def test_perfect_tracker():
    c = mc.scene(9, [[40, 64, 0, 17]], [[0, 0, 0, 0]], 64, 64, [0.5, 0.9], 64, 64)
    c["tr"][..., :4], c["tr"][..., 5], c["tr"][..., 4] = c["gt"][..., :4], c["gt"][..., 4], 0.9
    inside = (c["gt_ids"] >= 0) & (c["gt_ids"] < 64)
    c["tr_ids"], c["tr_counts"] = np.where(inside, (c["gt_ids"] + 7) % 64, -1).astype(np.int32), c["gt_counts"]
    out, ign = mc.run_lib(c)
    tp, fp, fn, idsw, siou, idtp, gt, hyp = out[0].T
    assert ign[0, 0] == ign[0, 1] > 0 and (gt == 121 - ign[0, 0]).all()
    assert (fp == 0).all() and (fn == 0).all() and (idsw == 0).all() and (idtp == gt).all() and (tp == hyp).all()
    assert (siou == 65535 * tp).all()


def test_id_swap():
    F, k = 10, 6
    out, _ = mc.run_lib(mc.swap_case(F, k))
    tp, fp, fn, idsw, siou, idtp, gt, hyp = out[0, 0]
    assert (tp, fp, fn, idsw, gt, hyp) == (2 * F, 0, 0, 2, 2 * F, 2 * F)
    assert idtp == 2 * max(k, F - k)           # each identity keeps the longer half of its track
    from yolo_hip.mot import ratios
    r = ratios(out)
    assert r["idf1"][0, 0] == 2 * idtp / (gt + hyp) == 0.6 and r["mota"][0, 0] == 1 - 2 / 20 and r["motp"][0, 0] == 1.0


def test_carry_keeps_the_pair_the_assignment_would_drop():
    out, _ = mc.run_lib(mc.carry_case())
    assert out[0, :, 0].tolist() == [3, 3] and out[0, :, 3].tolist() == [0, 1]   # TP; IDSW at 0.4 (carried), 0.5
    assert out[0, 0, 4] < out[0, 1, 4]         # the carried pair overlaps less than the best one


def test_bad_arguments_are_refused():
    from yolo_hip import _lib
    lib = _lib.lib()
    z = lambda *s, dtype=torch.int32: torch.zeros(s, dtype=dtype)
    tr, ti, tc, gt, gi, gc = z(1, 1, 4, 6, dtype=torch.float32), z(1, 1, 4), z(1, 1), z(1, 1, 4, 5, dtype=torch.float32), z(1, 1, 4), z(1, 1)
    thr, out, ign = torch.tensor([0.5]), z(1, 1, 8, dtype=torch.int64), z(1, 2)
    p = lambda t: None if t is None else t.data_ptr()

    def call(max_out=4, max_gt=4, S=1, F=1, num_thr=1, ng=4, nt=4, ca=1, thr=thr, out=out, tr=tr):
        return lib.yh_mot_eval_host(p(tr), p(ti), p(tc), max_out, p(gt), p(gi), p(gc), max_gt, S, F, None, p(thr), num_thr,
                                    ng, nt, ca, p(out), p(ign), 1)

    assert call() == 0
    for bad in (dict(max_out=257), dict(max_gt=257), dict(ng=1025), dict(nt=1025), dict(F=65536), dict(num_thr=0),
                dict(num_thr=17), dict(S=-1), dict(max_gt=-1), dict(ca=2), dict(thr=None), dict(out=None), dict(tr=None)):
        assert call(**bad) == -1 and b"mot_eval" in lib.yh_last_error(), bad
    assert lib.yh_mot_workspace_bytes(2, 3, 5, 7) == 2 * 3 * 80 and lib.yh_mot_workspace_bytes(1, 17, 5, 7) == 0
    # the device entry checks its workspace before anything is launched
    assert lib.yh_mot_eval(p(tr), p(ti), p(tc), 4, p(gt), p(gi), p(gc), 4, 1, 1, None, p(thr), 1, 4, 4, 1, p(out), p(ign),
                           p(gt), 16, None) == -1 and b"workspace too small" in lib.yh_last_error()
