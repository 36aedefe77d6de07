"""yh_track (csrc/track.hip) on the device against yh_track_host: the same bytes, outputs and state,
after every frame; at the caps; a state handed from the device to the host in mid-sequence; the
Tracker as the in-stream hook of a DetectPipeline; a launch on a side stream. Marked gpu.

The host twin itself is pinned to the numpy restatement by tests/test_track_host.py.
"""
import numpy as np
import pytest
import torch

import _track_cases as tc
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu


def same_states(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[4].tobytes() == w[4].tobytes(), f"{what} frame {i}: state"


@pytest.mark.parametrize("max_det", [8, 70])
@pytest.mark.parametrize("max_tracks", [5, 64, 65, 130])
def test_device_equals_host_after_every_frame(gpu, max_det, max_tracks):
    """3 streams, 12 frames; every launch is queued before the first download."""
    frames = tc.sequence(7, max_det=max_det)
    assert len(frames) == 12 and frames[0][0].shape == (3, max_det, 6)
    got, _ = tc.run_lib(frames, max_tracks, device=gpu, keep_state=True)
    want, _ = tc.run_lib(frames, max_tracks, keep_state=True)
    tc.same(got, want, f"{max_tracks} x {max_det}")
    same_states(got, want, f"{max_tracks} x {max_det}")
    assert sum(int(w[3].sum()) for w in want) > 30


def test_device_equals_host_at_the_pipeline_shape(gpu):
    """256 slots x 300 rows with 120 crowded objects: lanes share a slot's (a row's) scan, and an
    association takes several rounds."""
    frames = tc.sequence(8, frames=6, max_det=300, objects=120)
    got, _ = tc.run_lib(frames, 256, device=gpu, keep_state=True)
    want, _ = tc.run_lib(frames, 256, keep_state=True)
    tc.same(got, want, "256 x 300")
    same_states(got, want, "256 x 300")
    assert min(int(w[3].min()) for w in want[2:]) > 40


def test_device_equals_host_with_other_thresholds_and_stream_ids(gpu):
    frames = tc.sequence(7)
    sids = [[2, 7, 0] if i % 2 else [1, 0, 2] for i in range(len(frames))]      # 7: no such stream
    kw = dict(class_aware=False, max_age=2, iou_first=0.3, track_new=0.5, max_out=9, stream_ids=sids, keep_state=True)
    got, _ = tc.run_lib(frames, 40, device=gpu, **kw)
    want, _ = tc.run_lib(frames, 40, **kw)
    tc.same(got, want)
    same_states(got, want, "stream_ids")


def test_at_the_caps(gpu):
    """One stream, 1024 slots x 1024 rows, two frames: a 32 x 32 grid of boxes that moves a little,
    every slot taken in frame 1 and matched in frame 2."""
    g = np.arange(32, dtype=np.float32)
    cx, cy = np.meshgrid(40 + 60 * g, 40 + 60 * g)
    rng = np.random.default_rng(0)
    frames = []
    for f in range(2):
        order = rng.permutation(1024)
        rows = np.stack([cx.ravel() - 20 + 3 * f, cy.ravel() - 25, cx.ravel() + 20 + 3 * f, cy.ravel() + 25,
                         rng.uniform(0.3, 0.9, 1024), (np.arange(1024) % 3)], 1)[order]
        frames.append(tc.pack([rows], 1024))
    got, _ = tc.run_lib(frames, 1024, device=gpu, keep_state=True)
    want, _ = tc.run_lib(frames, 1024, keep_state=True)
    tc.same(got, want, "caps")
    same_states(got, want, "caps")
    assert want[0][3].tolist() == [1024] and want[1][3].tolist() == [1024]
    assert sorted(want[1][1][0].tolist()) == list(range(1, 1025))


def test_state_handed_from_device_to_host(gpu):
    frames = tc.sequence(7)
    want, want_state = tc.run_lib(frames, 64)
    first, state = tc.run_lib(frames[:6], 64, device=gpu)
    rest, state = tc.run_lib(frames[6:], 64, state=state.cpu())
    tc.same(first + rest, want)
    assert state.numpy().tobytes() == want_state.numpy().tobytes()


def test_side_stream_launch(gpu):
    """Correct after stream.synchronize() alone: the launch ran on that stream."""
    frames = tc.sequence(7)[:2]
    want, _ = tc.run_lib(frames, 64)
    on = [(d.to(gpu), c.to(gpu)) for d, c in frames]
    state = yt.track_state(3, 64, gpu)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        got = [yt.track(d, c, state) for d, c in on]
    s.synchronize()
    tc.same([tuple(t.cpu().numpy() for t in g) for g in got], want)


def test_bad_arguments_raise_on_the_device_path(gpu):
    dets, counts = (t.to(gpu) for t in tc.sequence(7)[0])
    with pytest.raises(RuntimeError, match="track_low"):
        yt.track(dets, counts, yt.track_state(3, 8, gpu), yt.params(track_low=0.9))
    with pytest.raises(ValueError, match="expected cuda"):
        yt.track(dets, counts, yt.track_state(3, 8))


def test_tracker_post_in_a_pipeline_equals_sequential_updates(gpu):
    """4 batches through a two-lane DetectPipeline with Tracker.post on its NMS stream, against
    Tracker.update over the same detections one after the other."""
    from nets import nn
    from yolo_hip import synth
    from yolo_hip.engine import Engine
    from yolo_hip.pipeline import DetectPipeline
    B, S = 4, 320
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    engs = []
    for _ in range(2):
        e = Engine(*model._yh_arch, gpu, torch.bfloat16)
        e.load_module(model)
        engs.append(e)
    base = synth.synth_scenes(B, S, S, seed=300)
    xs = [torch.roll(base, shifts=3 * i, dims=3).to(gpu, torch.bfloat16) for i in range(4)]     # a slow pan
    # the bands are laid over the scores these weights give: half of the first frame's rows are high
    from yolo_hip.engine import nms
    d0, c0 = nms(engs[0].forward(xs[0]))
    scores = torch.cat([d0[i, :k, 4] for i, k in enumerate(c0.tolist())])
    assert scores.numel() >= 8
    high = float(scores.median())
    kw = dict(max_tracks=256, track_high=high, track_low=high / 2, track_new=high)
    trk = yt.Tracker(B, gpu, **kw)
    pipe = DetectPipeline(engs, B, S, S, post=trk.post)
    got = [pipe.submit(x) for x in xs]
    pipe.drain()
    torch.cuda.synchronize()
    seq = yt.Tracker(B, gpu, **kw)
    total = 0
    for i, (dets, counts, extra, _) in enumerate(got):
        assert isinstance(extra, yt.Tracks)
        want = seq.update(dets, counts)
        for a, b in zip(extra, want):
            assert torch.equal(a, b), f"batch {i}"
        total += int(want.counts.sum())
    assert torch.equal(trk.state, seq.state) and total > 0
    assert int(want.ids.max()) >= 1
    # per-lane NMS runs the frames of a stream on several streams: refused
    trk2 = yt.Tracker(B, gpu, **kw)
    lanes = DetectPipeline(engs, B, S, S, post=trk2.post, nms_on_lane=True)
    lanes.submit(xs[0])
    with pytest.raises(RuntimeError, match="second stream"):
        lanes.submit(xs[1])
    lanes.drain()
    torch.cuda.synchronize()
