"""yh_motion_field on the host (yh_motion_field_host; CPU only): the twin against the numpy restatement of
tests/_motion_field_cases.py byte for byte - motion, sad, field and the state after every frame -, the
fallback rows against yh_motion on the same state, the accuracy under zoom, the tracker over a zoom
sequence, and the argument errors. tests/test_gpu_motion_field.py holds the kernels to the same cases.
"""
import ctypes

import numpy as np
import pytest
import torch

import _motion_cases as mc
import _motion_field_cases as fc
from yolo_hip import _lib
from yolo_hip import motion as ym
from yolo_hip import track as yt


@pytest.mark.parametrize("name", list(fc.CASES))
def test_host_twin_matches_restatement(name):
    _, _, thumb, R, grid, _ = fc.CASES[name]
    steps = [("similarity", [f], None) for f in fc.case_frames(name)]
    want = fc.ref(steps, 1, thumb, R, grid)
    fc.assert_same(fc.run(steps, 1, thumb, R, grid), want, name)
    if grid == (1, 1):                                     # always the fallback: yh_motion's bytes
        plain = fc.run([("translation", fr, ids) for _, fr, ids in steps], 1, thumb, R, grid)
        assert all(w[0].tobytes() == p[0].tobytes() and np.array_equal(w[3], p[3]) for w, p in zip(want, plain))
    else:
        assert all((w[2][0, :, 3] & 2).any() and w[0][0, 0] != 1 for w in want[2:]), "the zoom steps must be fitted"


def test_mixed_batch_and_fallback_rows():
    steps, S, thumb, R, grid = fc.mixed_steps(), 35, (24, 32), 2, (2, 2)
    want = fc.ref(steps, S, thumb, R, grid, max_mad=10)
    got = fc.run(steps, S, thumb, R, grid, max_mad=10)
    fc.assert_same(got, want, "mixed")
    # rule 5: a row that is not the fit's is yh_motion's on the same state, and every kind occurs
    plain = fc.run([("translation", fr, ids) for _, fr, ids in steps], S, thumb, R, grid, max_mad=10)
    for t in (0, 1):                                       # the states agree up to here whichever call advanced them
        fell = ~(got[t][2][:, :, 3] & 2).any(1)
        assert got[t][0][fell].tobytes() == plain[t][0][fell].tobytes() and np.array_equal(got[t][1], plain[t][1])
    fitted = (got[1][2][:, :, 3] & 2).any(1)
    cut = got[1][1][:, 0] > 10 * 20 * 28
    assert fitted.any() and cut.any() and not (fitted & cut).any()
    assert not fitted[::5].any() and (got[1][2][::5, :, 3] == 0).all(), "flat rows: no votes"
    assert (got[3][2][:, :, 3] & 2).any(), "a fit after yh_motion advanced the state"


@pytest.mark.parametrize("s", [0.96, 1.0, 1.05])
def test_accuracy_under_zoom(s):
    """Corner displacement error of the fit, 240 x 320 frames resampled in fp64 about (200, 90) plus a shift
    of (6, -4). The restatement measured 1.72, 0.62 and 1.95 px for s = 0.96, 1, 1.05 (translation only:
    8.54, 0.02, 10.67 px); the bound is twice that."""
    H, W, thumb, R, grid, c, sh = 240, 320, (60, 80), 4, (4, 6), (200.0, 90.0), (6.0, -4.0)
    wd = mc.world(11, H + 160, W + 160)
    pair = [fc.zoomed(wd, H, W, 1.0, c, (0, 0)), fc.zoomed(wd, H, W, s, c, sh)]
    err = {}
    for model in ("similarity", "translation"):
        got = fc.run([(model, [f], None) for f in pair], 1, thumb, R, grid, min_blocks=6)
        err[model] = fc.corner_error(got[1][0][0], s, c, sh, H, W)
    print(f"s {s}: corner error {err['similarity']:.3f} px, translation only {err['translation']:.3f} px")
    assert err["similarity"] <= 2 * {0.96: 1.72, 1.0: 0.62, 1.05: 1.95}[s]
    if s != 1.0:
        assert err["translation"] >= 4 * err["similarity"]      # measured: 4.97 and 5.49 times


def test_field_keeps_the_ids_over_a_zoom():
    h, w = mc.SHAKE_HW
    wd = mc.world(103, h + 240, w + 240)
    cc, s_tot, frames, boxes = np.array([w / 2, h / 2]), 1.0, [], []
    base = np.array([[cx - 20, cy - 40, cx + 20, cy + 40] for cx, cy in
                     ((100, 150), (300, 60), (420, 200), (200, 260), (540, 120))], np.float32)
    for z in (1.0, 1.14, 1 / 1.14, 1.14, 1 / 1.14, 1.12):   # in and out: the velocity model cannot follow
        s_tot *= z
        frames.append(fc.zoomed(wd, h, w, s_tot, cc, (0, 0)))
        boxes.append(((base.reshape(-1, 2, 2) - cc) * s_tot + cc).reshape(-1, 4).astype(np.float32))
    ids = {}
    for model in (None, "translation", "similarity"):
        est = model and ym.MotionEstimator(1, "cpu", thumb=mc.SHAKE_THUMB, radius=mc.SHAKE_R, model=model, grid=(4, 6))
        trk = yt.Tracker(1, "cpu", max_tracks=16)
        for f, bx in zip(frames, boxes):
            d = torch.full((1, 8, 6), float("nan"))
            d[0, :5] = torch.from_numpy(np.concatenate([bx, np.full((5, 1), 0.9, np.float32), np.zeros((5, 1), np.float32)], 1))
            r = trk.update(d, torch.tensor([5], dtype=torch.int32), motion=est.estimate([f]) if est else None)
        ids[model] = int(trk.state[0, 1])
    assert ids[None] > 5 and ids["translation"] > 5, ids
    assert ids["similarity"] == 5 and sorted(r.ids[0, :5].tolist()) == [1, 2, 3, 4, 5], ids


def test_abi_and_argument_errors():
    L = _lib.lib()
    assert L.yh_abi_version() == 7
    assert L.yh_motion_field_workspace_bytes(40, 6, 10, 8) == 32 * (60 * 16 + 6 * 17 * 17 * 4)
    assert L.yh_motion_field_workspace_bytes(1, 0, 10, 8) == 0 and L.yh_motion_field_workspace_bytes(1, 17, 16, 8) == 0
    img = np.zeros((72, 128, 3), np.uint8)
    state = ym.motion_state(1, (24, 32))
    state.fill_(0x5A)
    keep = state.numpy().copy()
    good = dict(grid_h=2, grid_w=2, radius=2, max_mad=24, min_contrast=4, tol=1, min_blocks=2)
    for bad in (dict(grid_h=0), dict(grid_w=0), dict(grid_h=6), dict(grid_w=8), dict(radius=0), dict(min_contrast=-1),
                dict(tol=-1), dict(tol=65), dict(min_blocks=1), None):
        p = None if bad is None else _lib.YhMotionFieldParams(*{**good, **bad}.values(), 0)
        motion, sad, field = np.full((1, 3), -7, np.float32), np.full((1, 2), -7, np.int32), np.full((1, 64, 4), -7, np.int32)
        d = _lib.YhFrame(img.ctypes.data, None, 72, 128, 0, 0, 0, 0)
        rc = L.yh_motion_field_host(ctypes.byref(d), 1, None, state.data_ptr(), 1, 24, 32, p and ctypes.byref(p),
                                    motion.ctypes.data, sad.ctypes.data, field.ctypes.data, 1)
        assert rc == -1 and L.yh_last_error(), bad
        assert (motion == -7).all() and (sad == -7).all() and (field == -7).all() and np.array_equal(state.numpy(), keep), bad
    with pytest.raises(ValueError):
        ym.estimate([img], ym.motion_state(1, (24, 32)), (24, 32), 2, model="affine")
