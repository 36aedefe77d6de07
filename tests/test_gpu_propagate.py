"""Track propagation on the device (yh_propagate_remember, yh_propagate; marked gpu): the kernels
against their host twin bit for bit on the case list of tests/_propagate_cases.py - outputs and the
state after every step -, a state carried from the host to the device in the middle of a sequence,
and the public loop (Detections-shaped rows -> Tracker -> Propagator -> Tracker) without a host read.
The twin is pinned to the numpy restatement in tests/test_propagate_host.py.
"""
import pytest
import torch

import _propagate_cases as pc
from yolo_hip import propagate as yp
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(pc.CASES))
def test_device_matches_host_twin(gpu, name):
    pc.same(pc.run(name, gpu), pc.run(name), name)


@pytest.mark.parametrize("name,at", [("geometry-nv12", 2), ("batch-over", 1), ("batch70", 4)])
def test_state_moves_from_host_to_device_mid_sequence(gpu, name, at):
    pc.same(pc.run(name, gpu, move_at=at), pc.run(name), name)


def test_public_loop_on_the_device(gpu):
    """The README snippet on device tensors, against the same loop on the host."""
    c = pc.case("batch70")
    frames = [s[1] for s in c["steps"][:3]]
    dets, _, counts = (torch.from_numpy(a) for a in c["steps"][0][2])
    dets = torch.nan_to_num(dets, nan=0.0)
    res = []
    for dev in ("cpu", gpu):
        trk, prop = yt.Tracker(3, dev, max_tracks=80), yp.Propagator(3, dev, max_tracks=80, radius=2, max_mad=12)
        tracks = trk.update(dets.to(dev), counts.to(dev))
        prop.remember(frames[0], tracks)
        out = [tracks]
        for f in frames[1:]:
            p = prop.propagate(f)
            out += [p, trk.update(p.dets, p.counts)]
        res.append([[t.cpu() for t in o] for o in out] + [[prop.state.cpu(), trk.state.cpu()]])
    for i, (h, d) in enumerate(zip(*res)):
        for a, b in zip(h, d):
            assert a.numpy().tobytes() == b.numpy().tobytes(), f"call {i}"
    assert int(res[0][1][3].max()) > 0
