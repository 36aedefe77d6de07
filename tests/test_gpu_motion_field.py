"""yh_motion_field on the device (marked gpu): motion_field_search and motion_field_fit against the numpy
restatement of tests/_motion_field_cases.py byte for byte - motion, sad, field and the whole state after
every frame - on the cases tests/test_motion_field_host.py holds the host twin to, and MotionEstimator
with its own workspace against the host twin.
"""
import numpy as np
import pytest
import torch

import _motion_field_cases as fc
from yolo_hip import motion as ym

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(fc.CASES))
def test_device_matches_restatement(gpu, name):
    _, _, thumb, R, grid, _ = fc.CASES[name]
    steps = [("similarity", [f], None) for f in fc.case_frames(name)]
    want = fc.ref(steps, 1, thumb, R, grid)
    fc.assert_same(fc.run(steps, 1, thumb, R, grid, device=gpu), want, name)
    assert grid == (1, 1) or all((w[2][0, :, 3] & 2).any() for w in want[2:])


def test_mixed_batch_two_launches(gpu):
    """33 rows, shuffled ids, an invalid id, first frames, flat rows, a scene cut, yh_motion in between."""
    steps, S, thumb, R, grid = fc.mixed_steps(), 35, (24, 32), 2, (2, 2)
    want = fc.ref(steps, S, thumb, R, grid, max_mad=10)
    fc.assert_same(fc.run(steps, S, thumb, R, grid, device=gpu, max_mad=10), want, "mixed")


def test_estimator_owns_the_workspace(gpu):
    name = "40x52-r3-g3x4"
    _, _, thumb, R, grid, _ = fc.CASES[name]
    kw = dict(thumb=thumb, radius=R, model="similarity", grid=grid, min_blocks=2)
    host, dev = ym.MotionEstimator(1, "cpu", **kw), ym.MotionEstimator(1, gpu, **kw)
    assert dev.workspace is not None and dev.workspace.is_cuda
    for f in fc.case_frames(name):
        want, got = host.estimate([f]), dev.estimate([torch.from_numpy(f).to(gpu)])
        assert got.motion.cpu().numpy().tobytes() == want.motion.numpy().tobytes() and torch.equal(got.sad.cpu(), want.sad)
        assert torch.equal(dev.state.cpu(), host.state)
    assert want.motion[0, 0] != 1
