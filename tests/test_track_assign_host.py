"""The tracker's assign mode on the host (yh_track2_host / yh_track_reid2_host): "greedy" is the
existing functions byte for byte, "optimal" equals the numpy restatement extended with the optimal
association (tests/_assign_cases.py), outputs and whole state after every frame; the two-person
scene keeps its ids only in optimal mode; without competition both modes agree; the mode may
change in mid-sequence. CPU only.
"""
import numpy as np
import pytest
import torch

import _assign_cases as ac
import _reid_cases as rc
import _track_cases as tc
from yolo_hip import track as yt

CASES = ac.tracker_cases()


@pytest.mark.parametrize("name", ["crowd_classes", "crowd_full_table"])
def test_greedy_is_the_existing_tracker(name):
    frames, mt, kw = CASES[name]
    old, _ = ac.run_track(frames, mt, assign=None, **kw)
    new, _ = ac.run_track(frames, mt, assign="greedy", threads=3, **kw)
    ac.same(new, old, name)
    want = tc.run_ref(frames, mt, **kw)
    tc.same(old, want, name)


def test_greedy_is_the_existing_reid_tracker():
    frames, mt = ac.reid_case()
    old, _ = ac.run_track(frames, mt, assign=None, dim=ac.REID_DIM)
    new, _ = ac.run_track(frames, mt, assign="greedy", dim=ac.REID_DIM)
    ac.same(new, old, "reid")
    plain, _ = rc.run_lib(frames, mt, ac.REID_DIM)
    rc.same(old, plain, "reid")


@pytest.mark.parametrize("name", list(CASES))
def test_optimal_equals_the_restatement(name):
    frames, mt, kw = CASES[name]
    got, _ = ac.run_track(frames, mt, assign="optimal", **kw)
    want = ac.run_ref(frames, mt, "optimal", **kw)
    ac.same(got, want, name)
    three, _ = ac.run_track(frames, mt, assign="optimal", threads=3, **kw)
    ac.same(three, got, name + " threads")


@pytest.mark.parametrize("kw", [{}, {"iou_min": 0.0, "cos_min": 0.2}])
def test_optimal_reid_equals_the_restatement(kw):
    frames, mt = ac.reid_case()
    got, _ = ac.run_track(frames, mt, assign="optimal", dim=ac.REID_DIM, **kw)
    want = ac.run_ref(frames, mt, "optimal", dim=ac.REID_DIM, **kw)
    ac.same(got, want, "reid")
    greedy, _ = ac.run_track(frames, mt, assign="greedy", dim=ac.REID_DIM, **kw)
    assert any(g[1].tobytes() != o[1].tobytes() for g, o in zip(greedy, got)), "the case never makes the modes differ"


def test_crowds_make_the_modes_differ():
    frames, mt, kw = CASES["crowd"]
    a, _ = ac.run_track(frames, mt, assign="greedy", **kw)
    b, _ = ac.run_track(frames, mt, assign="optimal", **kw)
    assert any(x[4].tobytes() != y[4].tobytes() for x, y in zip(a, b))


def test_two_people_keep_their_ids_only_in_optimal_mode():
    """Frame 2: IoU (t0, d0) = 65/135, (t1, d0) = 75/125, (t1, d1) = 50/150. The walk takes (t1, d0),
    loses track 1 and starts id 3 on the second person; the assignment takes (t0, d0) + (t1, d1)."""
    frames, mt, _ = CASES["two_person"]
    greedy, gs = ac.run_track(frames, mt, assign="greedy")
    optimal, os_ = ac.run_track(frames, mt, assign="optimal")
    for out in (greedy, optimal):
        assert out[0][3].tolist() == [2] and out[0][1][0, :2].tolist() == [1, 2]
    # greedy: id 2 jumps to the first person, the second is tentative in frame 2 and comes back as id 3
    assert greedy[1][3].tolist() == [1] and greedy[1][1][0, 0] == 2 and greedy[1][2][0, 0] == 0
    assert greedy[-1][1][0, :2].tolist() == [2, 3] and greedy[-1][3].tolist() == [2]
    status, ids = gs[0, 4:4 + mt].tolist(), gs[0, 4 + mt:4 + 2 * mt].tolist()
    assert status[ids.index(1)] == 3 and gs[0, 1] == 3            # track 1 is lost, three ids handed out
    # optimal: both ids stay on their people in every frame, nothing is born or lost
    for out in optimal:
        assert out[3].tolist() == [2] and out[1][0, :2].tolist() == [1, 2] and out[2][0, :2].tolist() == [0, 1]
    assert os_[0, 1] == 2 and sorted(os_[0, 4:4 + mt].tolist())[-2:] == [2, 2]
    assert sorted(os_[0, 4:4 + mt].tolist())[:-2] == [0] * (mt - 2)


def test_without_competition_both_modes_agree():
    frames = ac.separated()
    a, _ = ac.run_track(frames, 16, assign="greedy")
    b, _ = ac.run_track(frames, 16, assign="optimal")
    ac.same(b, a, "separated")
    assert sum(int(x[3].sum()) for x in a) > 40


def test_switching_modes_in_mid_sequence():
    frames, mt, kw = CASES["crowd"]
    modes = ["optimal", "greedy", "greedy", "optimal", "optimal", "greedy", "optimal", "greedy"]
    got, _ = ac.run_track(frames, mt, assign=modes, **kw)
    want = ac.run_ref(frames, mt, modes, **kw)
    ac.same(got, want, "switching")
    # the same through a Tracker whose attribute changes, from the state bytes of the run so far
    trk = yt.Tracker(2, "cpu", max_tracks=mt, assign="optimal")
    for i, ((dets, counts), mode) in enumerate(zip(frames, modes)):
        trk.assign = mode
        res = trk.update(dets, counts, threads=1)
        assert res.ids.numpy().tobytes() == got[i][1].tobytes()
        assert trk.state.numpy().tobytes() == got[i][4].tobytes()


def test_bad_modes_raise():
    dets, counts = CASES["two_person"][0][0]
    state = yt.track_state(1, 8)
    with pytest.raises(ValueError, match="assign"):
        yt.track(dets, counts, state, assign="hungarian")
    with pytest.raises(ValueError, match="assign"):
        yt.Tracker(1, "cpu", assign="best")
    import ctypes
    from yolo_hip import _lib
    L = _lib.lib()
    p = yt.params()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = (torch.empty((1, 8, 6)), torch.empty((1, 8), dtype=torch.int32), torch.empty((1, 8), dtype=torch.int32),
           torch.empty((1,), dtype=torch.int32))
    args = (ptr(dets), ptr(counts), 1, 8, None, ptr(state), 1, 8, ctypes.byref(p), 8, *(ptr(t) for t in out))
    assert L.yh_track2_host(*args, None, 1) == -1 and "assign" in L.yh_last_error().decode()
    bad = yt.AssignParams(2)
    assert L.yh_track2_host(*args, ctypes.byref(bad), 1) == -1 and "mode" in L.yh_last_error().decode()
    assert state.abs().sum() == 0
