"""The appearance stage on the device (csrc/reid.hip, the appearance instance of csrc/track.hip)
against its host twins: the same bytes - quantised features, int32 similarities (which also pins
the lane map of v_mfma_i32_32x32x32_i8 with exact integer data), tracker outputs and whole
states, galleries included. Marked gpu.

The host twins themselves are pinned to the numpy restatement by tests/test_reid_host.py.
"""
import numpy as np
import pytest
import torch

import _reid_cases as rc
import _track_cases as tc
import yolo_hip
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim", [64, 1280])
def test_quantize_device_equals_host(gpu, dim):
    e = torch.from_numpy(rc.quantize_cases(dim))
    want = yolo_hip.embed_quantize(e)
    got = yolo_hip.embed_quantize(e.to(gpu), out=torch.full(e.shape, 55, dtype=torch.int8, device=gpu))
    assert torch.equal(got.cpu(), want)
    assert want[6].any() and want[7, 3] == 127                         # the subnormal rows are features
    for count in (0, 9, 24, 99, -3):
        c = torch.tensor([count], dtype=torch.int32)
        bad = e.clone()
        bad[min(max(count, 0), 24):] = float("nan")                   # never read
        got = yolo_hip.embed_quantize(bad.to(gpu), count=c.to(gpu),
                                      out=torch.full(e.shape, 55, dtype=torch.int8, device=gpu))
        assert torch.equal(got.cpu(), yolo_hip.embed_quantize(e, count=c)), count


@pytest.mark.parametrize("dim", [64, 128, 1280])
def test_similarity_device_is_the_exact_int32_matmul(gpu, dim):
    """Every pair of ra, rb in {1, 31, 32, 33, 70}: partial tiles on either side, strided blocks, a
    permuted index with one entry out of range. The outputs lie inside a poisoned buffer whose
    margins must stay untouched."""
    for ra in (1, 31, 32, 33, 70):
        for rb in (1, 31, 32, 33, 70):
            a, b, index = rc.similarity_case(ra, rb, dim)
            want = rc.similarity(a.numpy(), b.numpy(), index.numpy())
            buf = torch.full((5, ra, rb), -9, dtype=torch.int32, device=gpu)
            da = a.to(gpu)                                             # .to() keeps the strides of the view
            if da.is_contiguous():
                big = torch.zeros((5, ra + 3, dim), dtype=torch.int8, device=gpu)
                big[:, :ra] = da
                da = big[:, :ra]
            assert da.stride(0) == (ra + 3) * dim
            got = yolo_hip.embed_similarity(da, b.to(gpu), index.to(gpu), out=buf[1:4])
            assert got.data_ptr() == buf[1:4].data_ptr()
            res = buf.cpu().numpy()
            assert np.array_equal(res[1:4], want), (ra, rb)
            assert (res[0] == -9).all() and (res[4] == -9).all(), (ra, rb)
            got = yolo_hip.embed_similarity(da[:3], b.to(gpu))         # no index: block b
            assert np.array_equal(got.cpu().numpy(), rc.similarity(a[:3].numpy(), b.numpy())), (ra, rb)


def test_similarity_device_with_more_batch_rows_than_xcds(gpu):
    """The kernel deals the batch rows out in groups of 8: 11 rows make a full and a partial group."""
    rng = np.random.default_rng(11)
    a = torch.from_numpy(rng.integers(-128, 128, (11, 33, 64), dtype=np.int8))
    b = torch.from_numpy(rng.integers(-128, 128, (11, 70, 64), dtype=np.int8))
    got = yolo_hip.embed_similarity(a.to(gpu), b.to(gpu))
    assert np.array_equal(got.cpu().numpy(), rc.similarity(a.numpy(), b.numpy()))
    index = torch.tensor([10, 3, -1, 0, 11, 5, 5, 9, 1, 2, 8], dtype=torch.int32)
    got = yolo_hip.embed_similarity(a.to(gpu), b.to(gpu), index.to(gpu))
    assert np.array_equal(got.cpu().numpy(), rc.similarity(a.numpy(), b.numpy(), index.numpy()))


def both(frames, max_tracks, dim, gpu, **kw):
    got, gstate = rc.run_lib(frames, max_tracks, dim, device=gpu, **kw)
    want, wstate = rc.run_lib(frames, max_tracks, dim, **kw)
    rc.same(got, want, f"{max_tracks} x {frames[0][0].shape[1]} x {dim}")
    assert torch.equal(gstate.cpu(), wstate), "state"
    return want, wstate


@pytest.mark.parametrize("dim", [64, 1280])
@pytest.mark.parametrize("max_tracks,max_det", [(1, 1), (33, 31), (256, 70)])
def test_track_reid_device_equals_host(gpu, max_tracks, max_det, dim):
    """3 streams, 12 frames; outputs after every frame, the whole state at the end."""
    frames = rc.reid_sequence(2, dim=dim, max_det=max_det)
    want, state = both(frames, max_tracks, dim, gpu, cos_min=0.3, iou_min=0.0)
    if max_tracks > 1:
        assert state.numpy()[:, 4 + 24 * max_tracks:].any()            # galleries were written
        plain, _ = tc.run_lib([f[:2] for f in frames], max_tracks)
        assert any(not np.array_equal(g[1], w[1]) for g, w in zip(want, plain)), "appearance changed no match"


def test_track_reid_device_equals_host_at_the_pipeline_shape(gpu):
    frames = rc.reid_sequence(8, dim=1280, frames=6, max_det=300, objects=120)
    want, _ = both(frames, 256, 1280, gpu)
    assert min(int(w[3].min()) for w in want[2:]) > 40


def test_track_reid_single_stream_and_stream_ids(gpu):
    frames = rc.reid_sequence(1)
    sids = [[2, 7, 0] if i % 2 else [1, 0, 2] for i in range(len(frames))]      # 7: no such stream
    both(frames, 40, 64, gpu, stream_ids=sids, iou_min=0.0, class_aware=False, max_out=9)
    one = rc.reid_sequence(3, streams=1)
    both(one, 64, 64, gpu, cos_min=0.2, iou_min=0.2)
    nine = rc.reid_sequence(5, streams=9, frames=5, max_det=31)                 # more streams than XCDs
    both(nine, 33, 64, gpu, cos_min=0.3, iou_min=0.0)


def test_a_state_moved_between_host_and_device_continues_with_the_same_bytes(gpu):
    frames = rc.reid_sequence(4)
    want, wstate = rc.run_lib(frames, 64, 64, iou_min=0.0)
    a, state = rc.run_lib(frames[:4], 64, 64, device=gpu, iou_min=0.0)
    b, state = rc.run_lib(frames[4:8], 64, 64, state=state.cpu(), iou_min=0.0)
    c, state = rc.run_lib(frames[8:], 64, 64, device=gpu, state=state.to(gpu), iou_min=0.0)
    rc.same(a + b + c, want)
    assert torch.equal(state.cpu(), wstate)


def test_without_features_it_is_yh_track_on_the_device(gpu):
    frames = tc.sequence(7)
    want, wstate = tc.run_lib(frames, 64, device=gpu)
    none = [(d, c, None, None, None) for d, c in frames]
    zero = [(d, c, torch.ones((200, 64)), torch.zeros(3, dtype=torch.int32), None) for d, c in frames]
    for name, seq in (("embed=None", none), ("feat_counts=0", zero)):
        got, state = rc.run_lib(seq, 64, 64, device=gpu, cos_min=-1.0, iou_min=0.0)
        tc.same(got, want, name)
        assert np.array_equal(rc.base_words(state, 64), wstate.cpu().numpy()), name
        assert not state.cpu().numpy()[:, 4 + 24 * 64:].any(), name


def test_classifier_embeddings_feed_the_tracker_on_the_device(gpu):
    """Frames -> feature_counts -> crop_rois -> Classifier.predict(embed=True) -> Tracker.update,
    nothing read back in between; the host twin fed the same embeddings gives the same bytes."""
    import _cls_cases as cc
    from yolo_hip import preprocess as pre, synth
    from yolo_hip.classify import Classifier

    def frame(seed):
        x = synth.synth_scenes(1, 240, 320, seed=seed)[0]
        return (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()   # BGR HWC

    cls = Classifier(cc.make_model("n", 10), gpu, torch.bfloat16, max_batch=16)
    trk = yolo_hip.Tracker(2, gpu, max_tracks=8, reid_dim=1280, reid_iou=0.0)
    host = yolo_hip.Tracker(2, "cpu", max_tracks=8, reid_dim=1280, reid_iou=0.0)
    frames = [frame(71), frame(72)]
    for step in range(3):
        rows = [[tc.box(60 + 9 * step, 80, 50, 90, 0.9), tc.box(200 - 7 * step, 120, 60, 100, 0.8),
                 tc.box(150, 60, 40, 40, 0.15)],
                [tc.box(100, 100 + 5 * step, 70, 70, 0.7), tc.box(250, 150, 40, 60, 0.2)]]
        dets, counts = tc.pack(rows, 4)
        d, c = dets.to(gpu), counts.to(gpu)
        fc = trk.feature_counts(d, c)
        crops = pre.crop_rois(frames, d, fc, (64, 32))
        got = cls.predict(crops, embed=True)
        t = trk.update(d, c, embed=got.embed, feat_counts=fc, embed_total=crops.total)
        assert fc.tolist() == [2, 1] and got.embed.shape == (8, 1280) and int(crops.total[0]) == 3
        w = host.update(dets, counts, embed=got.embed.float().cpu(), feat_counts=fc.cpu(), embed_total=crops.total.cpu(),
                        threads=1)
        for g, h in zip(t, w):
            assert torch.equal(g.cpu(), h), step
    assert torch.equal(trk.state.cpu(), host.state)
    assert t.counts.tolist() == [2, 1] and trk.state.cpu().numpy()[:, 4 + 24 * 8:].any()
