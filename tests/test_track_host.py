"""yh_track_host (csrc/track_host.cpp) through yolo_hip.track on CPU tensors: bit for bit the numpy
restatement (tests/_track_cases.py) on random sequences, the behaviours a tracker is used for
(each first confirmed on the restatement), stream_ids, empty and clamped inputs, argument errors.
"""
import ctypes

import numpy as np
import pytest
import torch

import _track_cases as tc
import yolo_hip
from yolo_hip import _lib
from yolo_hip import track as yt


def both(frames, max_tracks, **kw):
    """Restatement and host twin over a sequence, equal bit for bit -> the (shared) results."""
    want = tc.run_ref(frames, max_tracks, **kw)
    got, _ = tc.run_lib(frames, max_tracks, **kw)
    tc.same(got, want)
    return got


def ids_of(res, b=0):
    """Per frame the emitted {det_index: id} of batch row b."""
    return [{int(d): int(i) for d, i in zip(r[2][b, :r[3][b]], r[1][b, :r[3][b]])} for r in res]


@pytest.mark.parametrize("seed,max_tracks,max_det,kw", [
    (1, 64, 70, {}),
    (2, 20, 70, {}),                                     # fewer slots than objects: births are dropped
    (3, 64, 24, {}),                                     # fewer rows than detections: the frame is cut
    (4, 64, 70, dict(class_aware=False)),
    (5, 64, 70, dict(max_age=2, iou_first=0.3, track_new=0.5)),
    (6, 40, 70, dict(max_out=9)),
])
def test_host_equals_restatement_on_random_sequences(seed, max_tracks, max_det, kw):
    frames = tc.sequence(seed, max_det=max_det)
    res = both(frames, max_tracks, **kw)
    assert sum(int(r[3].sum()) for r in res) > 100       # the sequences do track something
    ids = [i for r in res for b in range(3) for i in r[1][b, :r[3][b]]]
    assert len(set(ids)) > 10 and len(ids) > 3 * len(set(ids))     # ids are born and kept


def test_the_random_sequences_contain_exact_ties_and_every_band():
    frames = tc.sequence(1)
    dup = low = 0
    for dets, counts in frames:
        for b in range(dets.shape[0]):
            r = dets[b, :counts[b]].numpy()
            dup += len(r) - len(np.unique(r[:, :4], axis=0))
            low += int(((r[:, 4] >= 0.1) & (r[:, 4] < 0.25)).sum())
            assert torch.isnan(dets[b, counts[b]:]).all()
    assert dup > 5 and low > 20


def test_threads_give_the_same_bytes():
    frames = tc.sequence(1)
    a, sa = tc.run_lib(frames, 64, threads=1)
    b, sb = tc.run_lib(frames, 64, threads=3)
    tc.same(a, b)
    assert sa.numpy().tobytes() == sb.numpy().tobytes()


def _occlusion(hidden):
    rows = []
    for f in range(12 + hidden + 6):
        vis = f < 12 or f >= 12 + hidden
        rows.append([tc.box(100 + 5 * f, 200, 80, 120)] if vis else [])
    return tc.single(rows)


def test_occlusion_of_30_frames_keeps_the_id_31_frames_do_not():
    res = ids_of(both(_occlusion(30), 8, max_age=30))
    assert all(r == {0: 1} for r in res[:12]) and all(r == {} for r in res[12:42])
    assert all(r == {0: 1} for r in res[42:])            # back on frame 43, matched at once
    res = ids_of(both(_occlusion(31), 8, max_age=30))
    assert all(r == {} for r in res[12:44])              # hidden, then one tentative frame
    assert all(r == {0: 2} for r in res[44:])            # a new track


def test_crossing_boxes_keep_their_ids():
    rows = [[tc.box(100 + 10 * f, 200, 80, 120), tc.box(420 - 10 * f, 290, 80, 120)] for f in range(33)]
    res = ids_of(both(tc.single(rows), 8))
    assert all(r == {0: 1, 1: 2} for r in res)


def test_a_single_frame_false_positive_is_never_output():
    rows = [[tc.box(100, 100, 50, 50)] for _ in range(8)]
    rows[3] = rows[3] + [tc.box(400, 300, 60, 60, score=0.95)]
    res = both(tc.single(rows), 8)
    assert all(r == {0: 1} for r in ids_of(res))
    # it did take a slot and an id for a frame: the next birth is id 3
    more = rows + [[tc.box(100, 100, 50, 50), tc.box(300, 100, 40, 40)]] * 2
    assert ids_of(both(tc.single(more), 8))[-1] == {0: 1, 1: 3}


def test_low_scores_keep_a_track_alive_but_never_start_one():
    rows = [[tc.box(100 + 2 * f, 100, 50, 50, score=0.9 if f < 4 else 0.15), tc.box(400, 300, 60, 60, score=0.2)]
            for f in range(10)]
    res = both(tc.single(rows), 8)
    assert all(r == {0: 1} for r in ids_of(res))
    assert res[-1][0][0, 0, 4] == np.float32(0.15)       # the row's score comes out


def test_more_births_than_slots_the_lowest_rows_win_and_freed_slots_are_reused():
    five = [tc.box(60 + 100 * i, 100, 40, 40, cls=float(i)) for i in range(5)]
    res = both(tc.single([five, five, []] + [list(reversed(five))] * 2, max_det=8), 3, max_age=0)
    ids = ids_of(res)
    assert ids[0] == {0: 1, 1: 2, 2: 3} and ids[1] == ids[0]      # rows 3 and 4 found no slot
    assert ids[2] == {}                                           # all lost and, with max_age 0, freed
    assert ids[3] == {}                                           # three tentative births in the reused slots
    assert ids[4] == {0: 4, 1: 5, 2: 6}                           # of the reversed frame's first rows
    # slots freed in a frame are taken in the same frame: the lost track goes, a new box is born
    a, b = tc.box(100, 100, 40, 40), tc.box(300, 100, 40, 40)
    res = both(tc.single([[a], [], [b], [b]]), 1, max_age=1)
    assert ids_of(res) == [{0: 1}, {}, {}, {0: 2}]


def test_class_aware_decides_whether_a_class_change_keeps_the_id():
    rows = [[tc.box(100, 100, 50, 50, cls=1.0 if f < 4 else 2.0)] for f in range(8)]
    res = both(tc.single(rows), 4, class_aware=False)
    assert all(r == {0: 1} for r in ids_of(res)) and res[-1][0][0, 0, 5] == 2.0
    res = ids_of(both(tc.single(rows), 4, class_aware=True))
    assert res[3] == {0: 1} and res[4] == {} and res[5] == {0: 2}


def test_stream_ids_permutations_and_subsets_equal_per_stream_runs():
    frames = tc.sequence(1)
    plain, plain_state = tc.run_lib(frames, 64)
    rng = np.random.default_rng(0)
    sids, sub = [], []
    for dets, counts in frames:
        rows = [int(v) for v in rng.permutation(3)[:rng.integers(1, 4)]]     # batch row j carries stream rows[j]
        sids.append(rows)
        sub.append((dets[rows].contiguous(), counts[rows].contiguous()))
    # each stream seen alone, on the frames it takes part in
    alone = {s: iter(tc.run_lib([(d[r.index(s):r.index(s) + 1], c[r.index(s):r.index(s) + 1])
                                 for (d, c), r in zip(sub, sids) if s in r], 64, streams=1)[0]) for s in range(3)}
    got, _ = tc.run_lib(sub, 64, streams=3, stream_ids=sids)
    tc.same(got, tc.run_ref(sub, 64, streams=3, stream_ids=sids))
    for g, r in zip(got, sids):
        for j, s in enumerate(r):
            w = next(alone[s])
            assert all(np.array_equal(g[i][j], w[i][0]) for i in range(4))
    # a full permutation every frame is the plain run with the rows permuted
    perm = [[2, 0, 1]] * len(frames)
    got, state = tc.run_lib([(d[[2, 0, 1]].contiguous(), c[[2, 0, 1]].contiguous()) for d, c in frames], 64,
                            stream_ids=perm)
    for g, w in zip(got, plain):
        assert all(np.array_equal(g[i], w[i][[2, 0, 1]]) for i in range(4))
    assert state.numpy().tobytes() == plain_state.numpy().tobytes()


def test_an_out_of_range_stream_id_touches_nothing():
    frames = tc.sequence(1)[:3]
    for bad in (-1, 3, 2 ** 30):
        sids = [[0, bad, 2]] * 3
        got, state = tc.run_lib(frames, 64, stream_ids=sids)
        tc.same(got, tc.run_ref(frames, 64, stream_ids=sids))
        assert all(g[3][1] == 0 and not g[0][1].any() and not g[1][1].any() and not g[2][1].any() for g in got)
        assert not state[1].any() and state[0].any() and state[2].any()


def test_empty_inputs_and_clamped_counts():
    frames = tc.sequence(1)[:4]
    md = frames[0][0].shape[1]
    # zero rows in a frame: tracks are lost, nothing comes out, the frame counter still advances
    empty = [frames[0], (frames[1][0], torch.zeros(3, dtype=torch.int32)), frames[2]]
    res = both(empty, 64)
    assert not res[1][3].any() and res[2][3].all()
    # counts are clamped on both sides: a negative count is 0 rows, a huge one max_det rows
    full = torch.from_numpy(np.nan_to_num(frames[0][0].numpy(), nan=0.0))
    full[:, :, 2:4] += 1.0                               # the former padding becomes small boxes
    wild = [(full, torch.tensor([-5, md + 1000, 2 ** 30], dtype=torch.int32))]
    want = tc.run_ref([(full, torch.tensor([0, md, md], dtype=torch.int32))], 64)
    got, _ = tc.run_lib(wild, 64)
    tc.same(got, want)
    assert got[0][3][0] == 0 and got[0][3][1] > 0
    # max_out 0, max_det 0, zero streams, an empty batch
    got, state = tc.run_lib(frames, 64, max_out=0)
    assert all(g[0].shape == (3, 0, 6) and not g[3].any() for g in got)
    assert state.numpy().tobytes() == tc.run_lib(frames, 64)[1].numpy().tobytes()     # the tracks are kept all the same
    t = yt.track(torch.zeros((2, 0, 6)), torch.zeros(2, dtype=torch.int32), yt.track_state(2, 4))
    assert t.dets.shape == (2, 0, 6) and t.counts.tolist() == [0, 0]
    t = yt.track(frames[0][0], frames[0][1], yt.track_state(0, 4))
    assert t.counts.tolist() == [0, 0, 0] and not t.dets.any() and not t.ids.any()
    t = yt.track(torch.zeros((0, 5, 6)), torch.zeros(0, dtype=torch.int32), yt.track_state(3, 4))
    assert t.dets.shape == (0, 5, 6)


def test_all_zero_bytes_are_the_empty_state_and_the_size_is_exported():
    lib = _lib.lib()
    assert lib.yh_track_state_bytes(3, 64) == yt.track_state(3, 64).numel() * 4 == 3 * (16 + 96 * 64)
    assert lib.yh_track_state_bytes(0, 64) == 0
    state = yt.track_state(1, 4)
    dets, counts = tc.pack([[tc.box(50, 50, 20, 20), tc.box(150, 50, 20, 20)]], 4)
    t = yt.track(dets, counts, state)
    assert t.ids[0, :2].tolist() == [1, 2] and t.counts.tolist() == [2]       # frame 1: born tracked, ids from 1
    assert state[0, :4].tolist() == [1, 2, 0, 0]


def test_bad_arguments_are_einval():
    lib = _lib.lib()
    t = torch.zeros((4096,))
    b = ctypes.c_void_p(t.data_ptr())
    good = yt.params()

    def call(dets=b, counts=b, batch=1, md=4, state=b, streams=1, mt=4, p=good, max_out=2, out=b, ids=b, di=b, oc=b):
        return lib.yh_track_host(dets, counts, batch, md, None, state, streams, mt,
                                 None if p is None else ctypes.byref(p), max_out, out, ids, di, oc, 1)

    assert call() == 0
    for kw, word in ((dict(batch=-1), b"batch"), (dict(md=-1), b"max_det"), (dict(streams=-1), b"streams"),
                     (dict(max_out=-1), b"max_out"), (dict(mt=0), b"max_tracks must be >= 1"),
                     (dict(mt=yt.MAX_TRACKS + 1), b"YH_TRACK_MAX_TRACKS"), (dict(md=yt.MAX_DET + 1), b"YH_TRACK_MAX_DET"),
                     (dict(p=None), b"null params"), (dict(p=yt.params(track_low=0.5, track_high=0.4)), b"track_low"),
                     (dict(p=yt.params(max_age=-1)), b"max_age"), (dict(dets=None), b"null dets"),
                     (dict(counts=None), b"null counts"), (dict(state=None), b"null state"), (dict(out=None), b"null out"),
                     (dict(ids=None), b"null out"), (dict(di=None), b"null out"), (dict(oc=None), b"null counts")):
        assert call(**kw) == -1, kw                                 # YH_EINVAL
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())
    with pytest.raises(RuntimeError, match="track_low"):
        yt.track(torch.zeros((1, 4, 6)), torch.zeros(1, dtype=torch.int32), yt.track_state(1, 4),
                 yt.params(track_low=0.9))


def test_track_rejects_mistyped_misplaced_and_strided_tensors():
    dets, counts = tc.sequence(1)[0]
    state = yt.track_state(3, 8)
    with pytest.raises(TypeError, match="dets"):
        yt.track(dets.double(), counts, state)
    with pytest.raises(TypeError, match="counts"):
        yt.track(dets, counts.long(), state)
    with pytest.raises(TypeError, match="state"):
        yt.track(dets, counts, state.float())
    with pytest.raises(ValueError, match="contiguous"):
        yt.track(dets, torch.zeros(6, dtype=torch.int32)[::2], state)
    with pytest.raises(ValueError, match="expected cpu"):
        yt.track(dets, counts.to("meta"), state)
    with pytest.raises(ValueError, match="words per stream"):
        yt.track(dets, counts, torch.zeros((3, 101), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        yt.track(dets, counts, state, stream_ids=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="max_tracks"):
        yt.track_state(1, yt.MAX_TRACKS + 1)


def test_tracker_class_on_the_host_and_the_package_exports():
    frames = tc.sequence(1)
    want, _ = tc.run_lib(frames, 32, max_age=5)
    trk = yolo_hip.Tracker(3, "cpu", max_tracks=32, max_age=5)
    for (dets, counts), w in zip(frames, want):
        t = trk.update(dets, counts)
        assert isinstance(t, yolo_hip.Tracks) and all(np.array_equal(a.numpy(), b) for a, b in zip(t, w))
    rows = t.tolist()
    assert len(rows) == 3 and rows[0][0].shape == (int(t.counts[0]), 6) and rows[0][1].shape == (int(t.counts[0]),)
    # a Detections, host stream_ids (checked), reset
    from yolo_hip.detect import Detections
    trk.reset()
    assert not trk.state.any()
    t = trk.update(Detections(frames[0][0][[1]].contiguous(), frames[0][1][[1]].contiguous()), stream_ids=[2])
    assert np.array_equal(t.dets.numpy()[0], want[0][0][1]) and not trk.state[:2].any() and trk.state[2].any()
    with pytest.raises(ValueError, match="distinct"):
        trk.update(*frames[0], stream_ids=[0, 1, 1])
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        trk.update(*frames[0], stream_ids=[0, 1, 3])
    trk.reset(streams=2)
    assert trk.streams == 2
    with pytest.raises(ValueError, match="3 rows for 2 streams"):
        trk.update(*frames[0])
    with pytest.raises(ValueError, match="track_low"):
        yolo_hip.Tracker(1, "cpu", track_low=0.5)
    # the function and its module share a name
    t = yolo_hip.track(frames[0][0], frames[0][1], yolo_hip.track_state(3, 32))
    assert t.counts.tolist() == want[0][3].tolist()
