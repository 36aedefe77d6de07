"""The host twins of the appearance stage (yh_embed_quantize_host, yh_embed_similarity_host,
yh_track_reid_host) against the numpy restatement of include/yolo_hip.h in tests/_reid_cases.py:
the same bytes, outputs and whole states; and the two behaviours the plain tracker lacks - ids
that survive a crossing, and a lost track found again away from its prediction. CPU only.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _reid_cases as rc
import _track_cases as tc
import yolo_hip
from yolo_hip import _lib
from yolo_hip import track as yt

NEW_SYMBOLS = ("yh_embed_quantize", "yh_embed_quantize_host", "yh_embed_similarity", "yh_embed_similarity_host",
               "yh_track_reid_state_bytes", "yh_track_reid_workspace_bytes", "yh_track_reid", "yh_track_reid_host")


@pytest.mark.parametrize("dim", [64, 1280])
def test_quantize_host_equals_the_restatement(dim):
    e = rc.quantize_cases(dim)
    want = rc.quantize(e)
    got = yolo_hip.embed_quantize(torch.from_numpy(e), out=torch.full(e.shape, 55, dtype=torch.int8))
    assert got.numpy().tobytes() == want.tobytes()
    assert not want[[1, 3, 4, 5, 11]].any() and want[2, 5] == -127 and np.abs(want[2]).sum() == 127
    assert want[7, 3] == 127 and want[6].any() and want[8].any() and (want[9] == round(127 / np.sqrt(dim))).all()
    norms = (want.astype(np.int64) ** 2).sum(1)[[0, 6, 8, 12, 13]]
    # length 127 up to the rounding: each element moves by at most 0.5, the vector by 0.5 sqrt(dim)
    assert (np.abs(np.sqrt(norms) - 127) <= 0.5 * np.sqrt(dim)).all(), norms
    for count in (0, 9, 24, 99, -3):
        c = torch.tensor([count], dtype=torch.int32)
        got = yolo_hip.embed_quantize(torch.from_numpy(e), count=c, out=torch.full(e.shape, 55, dtype=torch.int8))
        assert got.numpy().tobytes() == rc.quantize(e, count).tobytes(), count
    a = yolo_hip.embed_quantize(torch.from_numpy(e), threads=1)
    b = yolo_hip.embed_quantize(torch.from_numpy(e), threads=3)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dim", [64, 128, 1280])
@pytest.mark.parametrize("rb", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("ra", [1, 31, 32, 33, 70])
def test_similarity_host_is_the_exact_int32_matmul(ra, rb, dim):
    a, b, index = rc.similarity_case(ra, rb, dim)
    want = rc.similarity(a.numpy(), b.numpy(), index.numpy())
    got = yolo_hip.embed_similarity(a, b, index, out=torch.full((3, ra, rb), -9, dtype=torch.int32))
    assert np.array_equal(got.numpy(), want)
    assert not want[1].any() and want[2, 0, :].min() < 0 < want[2, 0, :].max() or rb == 1
    got = yolo_hip.embed_similarity(a[:3].contiguous(), b)             # no index: block b
    assert np.array_equal(got.numpy(), rc.similarity(a[:3].numpy(), b.numpy()))


def test_similarity_of_quantised_rows_is_16129_cosine():
    e = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (6, 1280)).astype(np.float32))
    q = yolo_hip.embed_quantize(e)
    s = yolo_hip.embed_similarity(q[None], q[None])[0].double() / 16129.0
    cos = torch.nn.functional.normalize(e.double(), dim=1)
    assert (s - cos @ cos.T).abs().max() < 0.02


def run_both(frames, max_tracks, dim, **kw):
    """Host twin and restatement over a reid sequence, compared frame by frame and as whole states."""
    got, state = rc.run_lib(frames, max_tracks, dim, **kw)
    kw.pop("threads", None)
    want, refs = rc.run_ref(frames, max_tracks, dim, **kw)
    rc.same(got, want)
    assert np.array_equal(state.numpy(), rc.ref_state(refs, max_tracks, dim)), "state"
    return got, state, refs


@pytest.mark.parametrize("seed,max_tracks,max_det,dim,kw", [
    (1, 64, 70, 64, {}),
    (2, 33, 31, 64, dict(cos_min=0.3, iou_min=0.0)),
    (3, 1, 1, 64, dict(iou_min=0.0)),
    (4, 20, 70, 1280, dict(cos_min=0.2, iou_min=0.1, class_aware=False, max_age=2)),
    (5, 40, 70, 64, dict(cos_min=-1.0, iou_min=0.0, max_out=9)),
])
def test_host_equals_restatement_on_random_sequences(seed, max_tracks, max_det, dim, kw):
    """12 frames, 3 streams: outputs after every frame, whole states (galleries included) at the end."""
    frames = rc.reid_sequence(seed, dim=dim, max_det=max_det)
    got, state, refs = run_both(frames, max_tracks, dim, **kw)
    assert len(frames) == 12 and sum(int(g[3].sum()) for g in got) >= 5
    if max_tracks > 1:
        assert any(r.gallery.any() for r in refs)


def test_appearance_changes_matches_on_the_random_sequences():
    """The sequences have teeth: with the features the ids differ from the plain tracker's."""
    frames = rc.reid_sequence(2, max_det=31)
    got, _ = rc.run_lib(frames, 33, 64, cos_min=0.3, iou_min=0.0)
    plain, _ = tc.run_lib([f[:2] for f in frames], 33)
    assert any(not np.array_equal(g[1], w[1]) for g, w in zip(got, plain))


def test_threads_and_stream_ids_give_the_same_bytes():
    frames = rc.reid_sequence(1)
    a, sa = rc.run_lib(frames, 64, 64, threads=1)
    b, sb = rc.run_lib(frames, 64, 64, threads=3)
    rc.same(a, b)
    assert torch.equal(sa, sb)
    sids = [[2, 7, 0] if i % 2 else [1, 0, 2] for i in range(len(frames))]      # 7: no such stream
    run_both(frames, 40, 64, stream_ids=sids, iou_min=0.0)


@pytest.mark.parametrize("seed", [7, 8])
def test_without_features_it_is_yh_track(seed):
    """embed=None, and feat_counts all zero: the outputs and the base state are track's bytes."""
    frames = tc.sequence(seed)
    want, wstate = tc.run_lib(frames, 64)
    none = [(d, c, None, None, None) for d, c in frames]
    zero = [(d, c, torch.ones((200, 64)), torch.zeros(3, dtype=torch.int32), None) for d, c in frames]
    for name, seq in (("embed=None", none), ("feat_counts=0", zero)):
        got, state = rc.run_lib(seq, 64, 64, cos_min=-1.0, iou_min=0.0)
        tc.same(got, want, name)
        assert np.array_equal(rc.base_words(state, 64), wstate.numpy()), name
        assert not state.numpy()[:, 4 + 24 * 64:].any(), name


def ids_of(res):
    """Per frame {det_index: id} of stream 0."""
    return [{int(r[2][0, k]): int(r[1][0, k]) for k in range(int(r[3][0]))} for r in res]


def crossing():
    """Two objects of one class walk towards each other, meet, and turn back: the Kalman prediction
    carries each past the other, so after the turn each predicted box lies on the other object."""
    rows = []
    for f in range(24):
        step = f if f < 12 else 23 - f
        rows.append([tc.box(100 + 14 * step, 200, 60, 120), tc.box(420 - 14 * step, 200, 60, 120)])
    return tc.single(rows)


def test_crossing_plain_track_swaps_ids_and_reid_does_not():
    frames = crossing()
    plain, _ = tc.run_lib(frames, 8)
    assert ids_of(plain)[0] == {0: 1, 1: 2}
    assert ids_of(plain)[-1] == {0: 2, 1: 1}, "the scenario lost its teeth: plain track no longer swaps"
    protos = rc.prototypes(64)
    seq = rc.with_features(frames, [[protos[:2]] for _ in frames], 64)
    got, _, _ = run_both(seq, 8, 64, cos_min=0.5, iou_min=0.0)
    assert all(r == {0: 1, 1: 2} for r in ids_of(got))
    got, _ = rc.run_lib(seq, 8, 64, cos_min=0.5, iou_min=0.1)          # the boxes overlap: BoT-SORT's gate passes too
    assert all(r == {0: 1, 1: 2} for r in ids_of(got))


def reappearing(hidden=5):
    """An object is tracked for 8 frames, hidden, and comes back 300 px from where it was."""
    rows = []
    for f in range(8 + hidden + 6):
        if f < 8:
            rows.append([tc.box(100 + 2 * f, 200, 60, 120)])
        elif f < 8 + hidden:
            rows.append([])
        else:
            rows.append([tc.box(420 + 2 * f, 210, 60, 120)])
    return tc.single(rows)


def test_reidentification_anywhere_needs_iou_min_zero():
    frames = reappearing()
    e = rc.prototypes(64)[3:4]
    seq = rc.with_features(frames, [[e if int(c[0]) else e[:0]] for _, c in frames], 64)
    got, _, _ = run_both(seq, 8, 64, cos_min=0.5, iou_min=0.0, max_age=30)
    ids = ids_of(got)
    assert all(r == {0: 1} for r in ids[:8]) and all(r == {} for r in ids[8:13])
    assert all(r == {0: 1} for r in ids[13:]), "the old id at once, in the frame it reappears"
    gated, _, _ = run_both(seq, 8, 64, cos_min=0.5, iou_min=0.5, max_age=30)
    plain, _ = tc.run_lib(frames, 8, max_age=30)
    for res in (gated, plain):
        ids = ids_of(res)
        assert ids[13] == {} and all(r == {0: 2} for r in ids[14:])    # tentative for a frame, then a new id
    rc.same(gated, plain)


def test_ties_fall_to_the_slot_then_the_row():
    """Identical embeddings and duplicate boxes: every eligible pair has the same value."""
    e = rc.prototypes(64)[5:6]
    b = tc.box(100, 100, 40, 40)
    frames = tc.single([[b, b, tc.box(300, 100, 40, 40)], [b, b, b, tc.box(300, 100, 40, 40)]], max_det=6)
    seq = rc.with_features(frames, [[np.repeat(e, int(c[0]), 0)] for _, c in frames], 64)
    got, _, _ = run_both(seq, 6, 64, cos_min=0.5, iou_min=0.0)
    # frame 2: slots 0, 1, 2 take rows 0, 1, 2 in that order, although slot 2's box is row 3's
    assert ids_of(got)[1] == {0: 1, 1: 2, 2: 3}


def test_gallery_zero_to_q_then_ema_and_unchanged_without_a_feature():
    protos = rc.prototypes(64)
    frames = tc.single([[tc.box(100, 100, 40, 40)]] * 5, max_det=2)
    e1, e2 = protos[1:2], protos[2:3]
    feats = [e1[:0], e1, e2, e2[:0], e2]
    seq = [(d, c, torch.from_numpy(np.ascontiguousarray(f)), torch.tensor([len(f)], dtype=torch.int32), None)
           for (d, c), f in zip(frames, feats)]
    q1, q2 = rc.quantize(e1)[0], rc.quantize(e2)[0]
    state = yt.track_state(1, 4, reid_dim=64)
    gal = lambda: state.numpy()[0, 4 + 24 * 4:].view(np.int8).reshape(4, 64).copy()
    step = lambda fr: rc.run_lib([fr], 4, 64, state=state)
    step(seq[0])
    assert not gal().any()                                             # born without a feature
    step(seq[1])
    assert np.array_equal(gal()[0], q1) and not gal()[1:].any()        # zero -> q
    step(seq[2])
    g2 = rc.ema(q1, q2)
    assert np.array_equal(gal()[0], g2) and not np.array_equal(g2, q1) and not np.array_equal(g2, q2)
    step(seq[3])
    assert np.array_equal(gal()[0], g2)                                # matched, no feature: unchanged
    step(seq[4])
    assert np.array_equal(gal()[0], rc.ema(g2, q2))
    assert abs(np.sqrt((gal()[0].astype(np.int64) ** 2).sum()) - 127) <= 0.5 * np.sqrt(64)


def test_a_birth_clears_the_bytes_a_freed_slot_kept():
    e = rc.prototypes(64)[1:2]
    rows = [[tc.box(100, 100, 40, 40)], [tc.box(100, 100, 40, 40)], [], [], [], [tc.box(300, 300, 40, 40)]]
    frames = tc.single(rows, max_det=2)
    feats = [e, e, e[:0], e[:0], e[:0], e[:0]]
    seq = [(d, c, torch.from_numpy(np.ascontiguousarray(f)), torch.tensor([len(f)], dtype=torch.int32), None)
           for (d, c), f in zip(frames, feats)]
    state = yt.track_state(1, 1, reid_dim=64)
    gal = lambda: state.numpy()[0, 4 + 24:].view(np.int8).copy()
    rc.run_lib(seq[:5], 1, 64, state=state, max_age=1)
    assert state[0, 4].item() == 0 and gal().any()                     # freed: the bytes stay
    rc.run_lib(seq[5:], 1, 64, state=state, max_age=1)
    assert state[0, 4].item() == 1 and not gal().any()                 # born without a feature: cleared


def test_capacity_and_embed_total_cut_features_off_inside_a_batch_row():
    frames = rc.reid_sequence(1)
    assert frames[1][4] is not None and frames[4][3] is None and frames[4][2].shape[0] < int(frames[4][1].sum())
    for i in (1, 4):
        feats = rc.row_features(frames[i], 70, 64)
        has = [h for _, h in feats]
        assert has[0].all() and not has[-1].all(), i
        assert any(h.any() and not h.all() for h in has), i


def test_workspace_and_state_sizes():
    lib = _lib.lib()
    assert lib.yh_track_reid_state_bytes(3, 64, 128) == yt.track_state(3, 64, reid_dim=128).numel() * 4 \
        == 3 * (16 + 96 * 64 + 64 * 128)
    assert lib.yh_track_reid_state_bytes(3, 64, 100) == 0
    need = lib.yh_track_reid_workspace_bytes(2, 70, 64, 128)
    assert need >= 2 * 70 * 128 + 2 * 70 * 4 + 2 * 64 * 70 * 4
    assert yt.reid_workspace(2, 70, 64, 128).numel() == need


def test_bad_arguments_are_einval():
    lib = _lib.lib()
    t = torch.zeros((1 << 16,))
    b = ctypes.c_void_p(t.data_ptr())
    good, rgood = yt.params(), yt.ReidParams(0.5, 0.5)

    def call(batch=1, md=4, mt=4, embed=b, capacity=4, dim=64, total=None, rp=rgood, ws=b, ws_bytes=1 << 18, dets=b):
        return lib.yh_track_reid_host(dets, b, batch, md, None, b, 1, mt, ctypes.byref(good), 2, b, b, b, b, embed,
                                      capacity, dim, None, total, None if rp is None else ctypes.byref(rp), ws, ws_bytes,
                                      1)

    assert call() == 0
    assert call(embed=None, total=b) == 0                              # a total without embed is ignored
    nan = float("nan")
    for kw, word in ((dict(dim=0), b"dim"), (dict(dim=100), b"dim"), (dict(dim=4096), b"dim"), (dict(dim=-64), b"dim"),
                     (dict(capacity=-1), b"capacity"), (dict(rp=None), b"null reid params"),
                     (dict(rp=yt.ReidParams(nan, 0.5)), b"finite"), (dict(rp=yt.ReidParams(0.5, float("inf"))), b"finite"),
                     (dict(ws=None), b"null workspace"), (dict(ws_bytes=100), b"workspace too small"),
                     (dict(batch=-1), b"batch"), (dict(mt=0), b"max_tracks"), (dict(dets=None), b"null dets")):
        assert call(**kw) == -1, kw
        assert word in lib.yh_last_error(), (kw, lib.yh_last_error())
    q = lib.yh_embed_quantize_host
    assert q(b, 2, 64, None, b, 1) == 0 and q(None, 0, 64, None, None, 1) == 0
    for args, word in (((b, 2, 96, None, b, 1), b"dim"), ((b, -1, 64, None, b, 1), b"rows"),
                       ((None, 2, 64, None, b, 1), b"null"), ((b, 2, 64, None, None, 1), b"null")):
        assert q(*args) == -1 and word in lib.yh_last_error(), args
    s = lib.yh_embed_similarity_host
    assert s(b, 4 * 64, 2, None, b, 2, 4, 3, 64, b, 1) == 0
    for args, word in (((b, 4 * 64, 2, None, b, 2, 4, 3, 32, b, 1), b"dim"), ((b, 4 * 64, 2, None, b, -2, 4, 3, 64, b, 1), b">= 0"),
                       ((b, 4 * 64, 2, None, b, 2, -4, 3, 64, b, 1), b">= 0"), ((b, 4 * 64 - 1, 2, None, b, 2, 4, 3, 64, b, 1), b"stride"),
                       ((None, 4 * 64, 2, None, b, 2, 4, 3, 64, b, 1), b"null a"), ((b, 4 * 64, 2, None, None, 2, 4, 3, 64, b, 1), b"null b"),
                       ((b, 4 * 64, 2, None, b, 2, 4, 3, 64, None, 1), b"null out")):
        assert s(*args) == -1 and word in lib.yh_last_error(), args
    with pytest.raises(ValueError, match="multiple of 64"):
        yolo_hip.embed_quantize(torch.zeros((2, 100)))
    with pytest.raises(ValueError, match="words per stream"):
        yt.track_reid(torch.zeros((1, 4, 6)), torch.zeros(1, dtype=torch.int32), yt.track_state(1, 4), dim=64)
    with pytest.raises(ValueError, match="dim must be given"):
        yt.track_reid(torch.zeros((1, 4, 6)), torch.zeros(1, dtype=torch.int32), yt.track_state(1, 4, reid_dim=64))


def test_tracker_class_with_and_without_reid_dim():
    frames = rc.reid_sequence(1)
    want, wstate = rc.run_lib(frames, 64, 64)
    trk = yolo_hip.Tracker(3, "cpu", max_tracks=64, reid_dim=64)
    assert trk.state.shape == yt.track_state(3, 64, reid_dim=64).shape
    for (dets, counts, embed, fc, total), w in zip(frames, want):
        t = trk.update(dets, counts, embed=embed, feat_counts=fc, embed_total=total, threads=1)
        assert np.array_equal(t.ids.numpy(), w[1]) and t.dets.numpy().tobytes() == w[0].tobytes()
    assert torch.equal(trk.state, wstate)
    plain = yolo_hip.Tracker(3, "cpu", max_tracks=64)
    assert plain.state.shape == yt.track_state(3, 64).shape and plain.reid_dim is None
    with pytest.raises(ValueError, match="reid_dim"):
        plain.update(frames[0][0], frames[0][1], embed=frames[0][2])
    # feature_counts: the leading rows at or above track_high, never beyond the count
    dets = torch.full((2, 5, 6), float("nan"))
    dets[0, :4, 4] = torch.tensor([0.9, 0.25, 0.2, 0.8])
    dets[1, :2, 4] = torch.tensor([0.7, 0.6])
    counts = torch.tensor([4, 1], dtype=torch.int32)
    fc = trk.feature_counts(dets, counts)
    assert fc.dtype == torch.int32 and fc.tolist() == [2, 1]


def test_the_new_symbols_are_in_the_header_the_protos_and_the_library():
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "yolo_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib._PROTOS, name
        assert hasattr(lib, name), name
    assert "YH_REID_MAX_DIM 2048" in header and yt.REID_MAX_DIM == 2048
    assert lib.yh_abi_version() == 7
    for name in ("track_reid", "embed_quantize", "embed_similarity"):
        assert callable(getattr(yolo_hip, name))
