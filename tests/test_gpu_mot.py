"""yh_mot_eval on the device: byte-equal to the host twin (which tests/test_mot_host.py holds to the
rules) on the shared case list, on the default stream and on a side stream; and a tracker scene run
through `Tracker` and `TrackEvaluator` on the device against the same on the host."""
import numpy as np
import pytest
import torch

import _assign_cases as ac
import _mot_cases as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(mc.cases()))
def test_kernel_equals_host_twin(name):
    c = mc.cases()[name]
    want = mc.run_lib(c, "cpu", 0)
    got = mc.run_lib(c, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = mc.run_lib(c, "cuda")
    for g in (got, again):
        assert g[0].tobytes() == want[0].tobytes(), f"{name}: counts\n{g[0]}\n{want[0]}"
        assert g[1].tobytes() == want[1].tobytes(), f"{name}: ignored"


@pytest.mark.parametrize("scene", ["two_person", "crowd_classes"])
@pytest.mark.parametrize("assign", ["greedy", "optimal"])
def test_tracker_to_evaluator(scene, assign):
    import yolo_hip
    frames, max_tracks, params = ac.tracker_cases()[scene]
    B, md = frames[0][0].shape[:2]
    res = {}
    for device in ("cpu", "cuda"):
        trk = yolo_hip.Tracker(B, device, max_tracks=max_tracks, assign=assign, **params)
        ev = yolo_hip.TrackEvaluator(B, len(frames), thr=(0.3, 0.5, 0.7), max_out=md, max_gt=md, n_gt_ids=md,
                                     n_tr_ids=256, device=device)
        for fr in frames:
            dets, counts = fr[0].to(device), fr[1].to(device)
            gt = dets[:, :, [0, 1, 2, 3, 5]].contiguous()          # the detections are the truth, row r is identity r
            ids = torch.arange(md, dtype=torch.int32, device=device).repeat(B, 1)
            ev.update(trk.update(dets, counts), gt, ids, counts)
        res[device] = ev.compute()
    for k, v in res["cpu"].items():
        assert np.array_equal(v, res["cuda"][k], equal_nan=True), k
    assert res["cuda"]["tp"].sum() > 0
    if scene == "two_person":       # the optimal assignment keeps both ids, the greedy walk trades them
        assert (res["cuda"]["idsw"][0, 1] == 0) == (assign == "optimal")
