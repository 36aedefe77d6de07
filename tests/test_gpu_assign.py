"""yh_assign (csrc/assign.hip) on the device against yh_assign_host: the same bytes on every solver
case of tests/_assign_cases.py, on the current and on a side stream. Marked gpu.

The host twin itself is pinned to the numpy restatement and to scipy by tests/test_assign_host.py.
"""
import pytest
import torch

import _assign_cases as ac
import yolo_hip

pytestmark = pytest.mark.gpu

CASES = ac.solver_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host(gpu, name):
    got = ac.run_lib(CASES[name], device=gpu)
    want = ac.run_lib(CASES[name])
    assert got[0].tobytes() == want[0].tobytes(), "row_of_slot"
    assert got[1].tobytes() == want[1].tobytes(), "slot_of_row"


def test_side_stream_and_fresh_outputs(gpu):
    """Correct after stream.synchronize() alone, with outputs the call allocates."""
    w, _, _ = CASES["sparse_256x300"]
    want = ac.run_lib(CASES["sparse_256x300"])
    on = torch.from_numpy(w).to(gpu)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        ros, sor = yolo_hip.assign(on)
    s.synchronize()
    assert ros.cpu().numpy().tobytes() == want[0].tobytes() and sor.cpu().numpy().tobytes() == want[1].tobytes()


def test_bad_arguments_raise_on_the_device_path(gpu):
    with pytest.raises(RuntimeError, match="YH_ASSIGN_MAX_SIZE"):
        yolo_hip.assign(torch.zeros((1, 2, 1025), dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match="expected cuda"):
        yolo_hip.assign(torch.zeros((1, 2, 2), dtype=torch.int32, device=gpu), t_counts=torch.zeros(1, dtype=torch.int32))
