"""The tracker's optimal mode on the device (the OPT instances of csrc/track.hip) against the host
twins: the same bytes, outputs and whole state, after every frame, for the plain and the
appearance tracker; the greedy mode through the new entry points against the host; a state handed
to the host and back in mid-sequence; a change of mode in mid-sequence; Tracker(assign="optimal")
as the in-stream hook of a DetectPipeline. Marked gpu.

The host twins are pinned to the numpy restatement by tests/test_track_assign_host.py.
"""
import pytest
import torch

import _assign_cases as ac
import _track_cases as tc
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu

CASES = ac.tracker_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_optimal_device_equals_host_after_every_frame(gpu, name):
    frames, mt, kw = CASES[name]
    got, _ = ac.run_track(frames, mt, assign="optimal", device=gpu, **kw)
    want, _ = ac.run_track(frames, mt, assign="optimal", **kw)
    ac.same(got, want, name)


def test_greedy_through_the_new_entry_point(gpu):
    frames, mt, kw = CASES["crowd"]
    got, _ = ac.run_track(frames, mt, assign="greedy", device=gpu, **kw)
    want, _ = ac.run_track(frames, mt, assign=None, **kw)
    ac.same(got, want, "greedy")


def test_optimal_at_the_pipeline_shape(gpu):
    """256 slots x 300 rows with 120 crowded objects of one class: five columns per lane, long paths."""
    frames = tc.sequence(8, streams=2, frames=4, max_det=300, objects=120, classes=1)
    got, _ = ac.run_track(frames, 256, assign="optimal", device=gpu)
    want, _ = ac.run_track(frames, 256, assign="optimal")
    ac.same(got, want, "256 x 300")
    assert min(int(w[3].min()) for w in want[2:]) > 40


@pytest.mark.parametrize("kw", [{}, {"iou_min": 0.0, "cos_min": 0.2}])
def test_optimal_reid_device_equals_host(gpu, kw):
    frames, mt = ac.reid_case()
    got, _ = ac.run_track(frames, mt, assign="optimal", dim=ac.REID_DIM, device=gpu, **kw)
    want, _ = ac.run_track(frames, mt, assign="optimal", dim=ac.REID_DIM, **kw)
    ac.same(got, want, "reid")


def test_state_handed_to_the_host_and_back_and_modes_switched(gpu):
    frames, mt, kw = CASES["crowd"]
    modes = ["optimal", "greedy", "optimal", "optimal", "greedy", "optimal", "greedy", "optimal"]
    want, _ = ac.run_track(frames, mt, assign=modes, **kw)
    got, _ = ac.run_track(frames, mt, assign=modes, device=gpu, handover=4, **kw)
    ac.same(got, want, "handover")
    # the second half on the host from the device's state
    first, state = ac.run_track(frames[:4], mt, assign=modes[:4], device=gpu, **kw)
    rest, _ = ac.run_track(frames[4:], mt, assign=modes[4:], state=state.cpu(), **kw)
    ac.same(first + rest, want, "device then host")


def test_optimal_tracker_post_in_a_pipeline_equals_sequential_updates(gpu):
    """3 batches through a DetectPipeline with Tracker(assign="optimal").post on its NMS stream,
    against Tracker.update over the same detections, and against the host twin."""
    from nets import nn
    from yolo_hip import synth
    from yolo_hip.engine import Engine, nms
    from yolo_hip.pipeline import DetectPipeline
    B, S = 2, 320
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    eng = Engine(*model._yh_arch, gpu, torch.bfloat16)
    eng.load_module(model)
    base = synth.synth_scenes(B, S, S, seed=300)
    xs = [torch.roll(base, shifts=3 * i, dims=3).to(gpu, torch.bfloat16) for i in range(3)]
    d0, c0 = nms(eng.forward(xs[0]))
    scores = torch.cat([d0[i, :k, 4] for i, k in enumerate(c0.tolist())])
    assert scores.numel() >= 8
    high = float(scores.median())
    kw = dict(max_tracks=256, track_high=high, track_low=high / 2, track_new=high, assign="optimal")
    trk = yt.Tracker(B, gpu, **kw)
    pipe = DetectPipeline([eng], B, S, S, post=trk.post)
    got = [pipe.submit(x) for x in xs]
    pipe.drain()
    torch.cuda.synchronize()
    seq, host = yt.Tracker(B, gpu, **kw), yt.Tracker(B, "cpu", **kw)
    total = 0
    for i, (dets, counts, extra, _) in enumerate(got):
        assert isinstance(extra, yt.Tracks)
        want = seq.update(dets, counts)
        on_host = host.update(dets.cpu(), counts.cpu(), threads=1)
        for a, b, c in zip(extra, want, on_host):
            assert torch.equal(a, b) and torch.equal(a.cpu(), c), f"batch {i}"
        total += int(want.counts.sum())
    assert torch.equal(trk.state, seq.state) and torch.equal(trk.state.cpu(), host.state) and total > 0
