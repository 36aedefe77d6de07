"""yh_assign_host (csrc/assign_host.cpp) against the numpy restatement of the normative algorithm
(tests/_assign_cases.py): the same bytes on every case; the matching is valid; its total weight is
exactly scipy's optimum and never below the greedy walk's; thread counts do not matter; every
YH_EINVAL is raised. CPU only.
"""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import _assign_cases as ac
import yolo_hip
from yolo_hip import _lib

CASES = ac.solver_cases()


_REF = {}


def ref(name):
    """The restatement's answer, computed once per case."""
    if name not in _REF:
        _REF[name] = ac.solve_batch(*CASES[name])
    return _REF[name]


def total(w, ros):
    return sum(int(w[t, d]) for t, d in enumerate(ros[:w.shape[0]]) if d >= 0)


@pytest.mark.parametrize("name", list(CASES))
def test_twin_equals_the_restatement(name):
    got = ac.run_lib(CASES[name])
    want = ref(name)
    assert got[0].tobytes() == want[0].tobytes(), "row_of_slot"
    assert got[1].tobytes() == want[1].tobytes(), "slot_of_row"


@pytest.mark.parametrize("name", list(CASES))
def test_matching_is_valid_and_optimal(name):
    weights, tcnt, dcnt = CASES[name]
    ros, sor = ac.run_lib(CASES[name])
    for p in range(weights.shape[0]):
        w = ac.live(weights, tcnt, dcnt, p)
        nt, nd = w.shape
        assert (ros[p, nt:] == -1).all() and (sor[p, nd:] == -1).all()
        used = ros[p][ros[p] >= 0]
        assert len(set(used.tolist())) == len(used) and (used < nd).all(), "not injective"
        for t, d in enumerate(ros[p]):
            if d >= 0:
                assert w[t, d] > 0, "a forbidden pair"
                assert sor[p, d] == t
        for d, t in enumerate(sor[p]):
            if t >= 0:
                assert ros[p, t] == d
        got = total(w, ros[p])
        if nt and nd:
            r, c = linear_sum_assignment(w, maximize=True)
            assert got == int(w[r, c].sum()), "not the maximum weight"
        else:
            assert got == 0
        assert got >= ac.greedy_total(w)


def test_band_beats_the_greedy_walk():
    weights, _, _ = CASES["band_64"]
    ros, _ = ac.run_lib(CASES["band_64"])
    w = ac.live(weights, None, None, 0)
    assert (ros[0] == np.arange(64)).all()                     # the last slot's path moved every slot
    assert total(w, ros[0]) == 64 * 1000 > ac.greedy_total(w) == 63 * 1001


def test_weight_is_not_cardinality():
    """One heavy pair beats two light ones, and a constant matrix pins the tie rules: slot i takes row i."""
    w = torch.tensor([[[10, 100], [0, 10]]], dtype=torch.int32)
    ros, sor = yolo_hip.assign(w)
    assert ros.tolist() == [[1, -1]] and sor.tolist() == [[-1, 0]]
    ros, _ = ac.run_lib(CASES["constant"])
    assert (ros == np.arange(12)).all()


@pytest.mark.parametrize("name", ["counts", "sparse_256x300", "ties_128"])
def test_threads_do_not_matter(name):
    one = ac.run_lib(CASES[name], threads=1)
    three = ac.run_lib(CASES[name], threads=3)
    assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes()


def test_clamp_is_the_stated_one():
    weights, _, _ = CASES["clamp"]
    assert weights.max() > ac.M and weights.min() < 0
    clamped = np.clip(weights, 0, ac.M).astype(np.int32)
    a, b = ac.run_lib(CASES["clamp"]), ac.run_lib((clamped, None, None))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_bad_arguments():
    L = _lib.lib()
    w = torch.ones((1, 4, 4), dtype=torch.int32)
    ros, sor = torch.empty((1, 4), dtype=torch.int32), torch.empty((1, 4), dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    msg = lambda: L.yh_last_error().decode()
    assert L.yh_assign_host(p(w), 1, 4, 4, None, None, p(ros), p(sor), 1) == 0
    assert L.yh_assign_host(p(w), 1, 1025, 4, None, None, p(ros), p(sor), 1) == -1 and "YH_ASSIGN_MAX_SIZE" in msg()
    assert L.yh_assign_host(p(w), 1, 4, 1025, None, None, p(ros), p(sor), 1) == -1 and "YH_ASSIGN_MAX_SIZE" in msg()
    assert L.yh_assign_host(p(w), -1, 4, 4, None, None, p(ros), p(sor), 1) == -1 and "problems" in msg()
    assert L.yh_assign_host(p(w), 1, -4, 4, None, None, p(ros), p(sor), 1) == -1 and ">= 0" in msg()
    assert L.yh_assign_host(p(w), 1, 4, -4, None, None, p(ros), p(sor), 1) == -1 and ">= 0" in msg()
    assert L.yh_assign_host(None, 1, 4, 4, None, None, p(ros), p(sor), 1) == -1 and "weights" in msg()
    assert L.yh_assign_host(p(w), 1, 4, 4, None, None, None, p(sor), 1) == -1 and "row_of_slot" in msg()
    assert L.yh_assign_host(p(w), 1, 4, 4, None, None, p(ros), None, 1) == -1 and "slot_of_row" in msg()
    with pytest.raises(RuntimeError, match="YH_ASSIGN_MAX_SIZE"):
        yolo_hip.assign(torch.zeros((1, 1025, 2), dtype=torch.int32))
    with pytest.raises(TypeError, match="int32"):
        yolo_hip.assign(torch.zeros((1, 2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="problems, T, D"):
        yolo_hip.assign(torch.zeros((2, 2), dtype=torch.int32))
    # nothing to do is not an error, and every byte is still written
    ros, sor = yolo_hip.assign(torch.zeros((2, 0, 3), dtype=torch.int32))
    assert ros.shape == (2, 0) and sor.tolist() == [[-1] * 3] * 2
