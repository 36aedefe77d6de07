"""yh_hota_eval on the device: byte-equal to the host twin (which tests/test_hota_host.py holds to the
float64 reference) on the shared case list and with `frames` cut short; and a tracker scene run
through `Tracker` and `TrackEvaluator(hota=True)` on the device against the same on the host."""
import numpy as np
import pytest
import torch

import _assign_cases as ac
import _hota_cases as hc

pytestmark = pytest.mark.gpu


def _same(c):
    want = hc.run_lib(c, "cpu", 0)
    got = hc.run_lib(c, "cuda")
    for g, w, what in zip(got, want, ("counts", "rows", "ignored")):
        assert g.tobytes() == w.tobytes(), f"{what}\n{g}\n{w}"
    return got


@pytest.mark.parametrize("name", list(hc.cases()) + list(hc.dense_cases()))
def test_kernels_equal_host_twin(name):
    got = _same({**hc.cases(), **hc.dense_cases()}[name])
    if name not in ("empty_sides", "no_rows"):
        assert got[0][..., 0].sum() > 0


def test_frames_shorter_than_the_buffers():
    c = dict(hc.cases()["recipe"], frames=np.asarray([5, 0, 39], np.int32))
    _same(c)
    _same(dict(c, frames=None))


def test_tracker_to_evaluator():
    import yolo_hip
    frames, max_tracks, params = ac.tracker_cases()["crowd_classes"]
    B, md = frames[0][0].shape[:2]
    res = {}
    for device in ("cpu", "cuda"):
        trk = yolo_hip.Tracker(B, device, max_tracks=max_tracks, assign="optimal", **params)
        ev = yolo_hip.TrackEvaluator(B, len(frames), thr=(0.5,), max_out=md, max_gt=md, n_gt_ids=md, n_tr_ids=256,
                                     device=device, hota=True)
        for fr in frames:
            dets, counts = fr[0].to(device), fr[1].to(device)
            gt = dets[:, :, [0, 1, 2, 3, 5]].contiguous()          # the detections are the truth, row r is identity r
            ids = torch.arange(md, dtype=torch.int32, device=device).repeat(B, 1)
            ev.update(trk.update(dets, counts), gt, ids, counts)
        res[device] = ev.compute()
    assert res["cuda"]["hota_alpha"].shape == (B, 19) and res["cuda"]["hota"].shape == (B,)
    for k, v in res["cpu"].items():
        assert np.array_equal(v, res["cuda"][k], equal_nan=True), k
    assert res["cuda"]["hota_tp"].sum() > 0
