"""Camera-motion compensation on the host (yh_motion_host, yh_track_warp_host; CPU only): the twins
against the numpy restatement of tests/_motion_cases.py bit for bit - motion bits, sad and the state
after every frame -, the tie, window-edge and gate rules, the accuracy of the estimate over the
shake sequence, the warp on a populated state in both layouts, the tracker with and without the
warp, and the argument errors. tests/test_gpu_motion.py holds the kernels to these twins.
"""
import ctypes

import numpy as np
import pytest
import torch

import _motion_cases as mc
import _track_cases as tc
from yolo_hip import _lib
from yolo_hip import motion as ym
from yolo_hip import track as yt


def _run(frames_per_step, streams, thumb, radius, max_mad, ids_per_step=None, threads=1):
    """The host twin over a sequence, poisoned outputs -> per step (motion, sad, state bytes)."""
    state = ym.motion_state(streams, thumb)
    res = []
    for i, frames in enumerate(frames_per_step):
        B = len(frames)
        out = (torch.full((B, 3), -7.0), torch.full((B, 2), -7, dtype=torch.int32))
        ids = None if ids_per_step is None or ids_per_step[i] is None else torch.tensor(ids_per_step[i], dtype=torch.int32)
        got = ym.estimate(frames, state, thumb, radius, max_mad, stream_ids=ids, out=out, threads=threads)
        assert got.motion is out[0] and got.sad is out[1]
        res.append((out[0].numpy().copy(), out[1].numpy().copy(), state.numpy().copy()))
    return res


def _ref(frames_per_step, streams, thumb, radius, max_mad, ids_per_step=None):
    ref = mc.RefMotion(streams, thumb)
    res = []
    for i, frames in enumerate(frames_per_step):
        m, s = ref.step(frames, radius, max_mad, None if ids_per_step is None else ids_per_step[i])
        res.append((m, s, ref.state.copy()))
    return res


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].tobytes() == w[0].tobytes(), f"{what} step {i}: motion {g[0].tolist()} vs {w[0].tolist()}"
        assert np.array_equal(g[1], w[1]), f"{what} step {i}: sad {g[1].tolist()} vs {w[1].tolist()}"
        assert np.array_equal(g[2], w[2]), f"{what} step {i}: state"


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("thumb,radius", mc.THUMBS)
def test_host_twin_matches_restatement(thumb, radius, threads):
    streams = mc.mixed_streams(thumb)
    S = len(streams)
    kinds = [isinstance(s[0], mc.pre.NV12) for s in streams]
    assert any(kinds) and not all(kinds)
    # row b of step i: a permutation that changes per step, one row's id out of range
    steps, ids = [], []
    for i in range(3):
        perm = [(b * 3 + i) % S for b in range(S)] if S % 3 else list(np.random.default_rng(i).permutation(S))
        bad = (2 * i + 1) % S
        row_ids = [int(p) for p in perm]
        row_ids[bad] = S + 3 if i != 1 else -1
        ids.append(row_ids)
        steps.append([streams[p][i] for p in perm])
    want = _ref(steps, S, thumb, radius, 24, ids)
    got = _run(steps, S, thumb, radius, 24, ids, threads)
    _same(got, want, f"thumb {thumb}")
    assert any((w[0][:, 1:] != 0).any() for w in want), "no step estimated a shift"
    # and with the identity order
    plain = [[s[i] for s in streams] for i in range(3)]
    _same(_run(plain, S, thumb, radius, -1, None, threads), _ref(plain, S, thumb, radius, -1), "plain")


def test_ties_and_window_edges():
    thumb, R = (12, 16), 2
    # flat frames: every SAD is 0, the tie rule picks (0, 0)
    got = _run([[mc.flat_frame(36, 64, 90)], [mc.flat_frame(36, 64, 90)]], 1, thumb, R, 24)
    assert got[1][0].tolist() == [[1.0, 0.0, 0.0]] and got[1][1].tolist() == [[0, 0]]
    assert got[0][0].tolist() == [[1.0, 0.0, 0.0]] and got[0][1].tolist() == [[0, 0]]       # no previous frame
    # a shift of exactly +-R thumbnail pixels: no refinement on that axis (36 x 64 -> 12 x 16: 3 x 4 px)
    wd = mc.world(21, 36 + 24, 64 + 24)
    for sy, sx in ((0, R), (0, -R), (R, 0), (-R, 0), (R, -R)):
        a = mc.bgr_frame(wd, 12, 12, 36, 64)
        b = mc.bgr_frame(wd, 12 - 3 * sy, 12 - 4 * sx, 36, 64)                               # content moves by (+sx, +sy)
        frames = [[a], [b]]
        got, want = _run(frames, 1, thumb, R, -1), _ref(frames, 1, thumb, R, -1)
        _same(got, want, f"shift {(sy, sx)}")
        m = got[1][0][0]
        assert got[1][1][0, 0] == 0, "an exact shift by whole thumbnail pixels matches exactly"
        if abs(sx) == R:
            assert m[1] == np.float32(sx) * np.float32(4)
        if abs(sy) == R:
            assert m[2] == np.float32(sy) * np.float32(3)


def test_gate():
    thumb, R = (24, 40), 4
    a = mc.bgr_frame(mc.world(31, 114, 184), 12, 12, 90, 160)
    b = mc.bgr_frame(mc.world(32, 114, 184), 12, 12, 90, 160)                                 # unrelated content
    gated, want = _run([[a], [b]], 1, thumb, R, 8), _ref([[a], [b]], 1, thumb, R, 8)
    _same(gated, want, "gate")
    window = (24 - 8) * (40 - 8)
    assert gated[1][1][0, 0] > 8 * window, "the case must trip the gate"
    assert gated[1][0].tolist() == [[1.0, 0.0, 0.0]]
    assert np.array_equal(gated[1][2][16:16 + 24 * 40].reshape(24, 40), mc.thumbnail(mc.luma(b), 24, 40))
    raw = _run([[a], [b]], 1, thumb, R, -1)
    _same(raw, _ref([[a], [b]], 1, thumb, R, -1), "no gate")
    assert np.array_equal(raw[1][1], gated[1][1])
    t = mc.sad_table(mc.thumbnail(mc.luma(b), 24, 40), mc.thumbnail(mc.luma(a), 24, 40), R)
    assert raw[1][0].tobytes() == mc.result(t, R, 90, 160, 24, 40, -1)[0].tobytes()          # the raw best shift


def _shake_motions():
    offs, frames, boxes = mc.shake()
    est = ym.MotionEstimator(1, "cpu", thumb=mc.SHAKE_THUMB, radius=mc.SHAKE_R, max_mad=24)
    return offs, boxes, [est.estimate([f]).motion.clone() for f in frames]


def test_accuracy_over_the_shake():
    offs, _, motions = _shake_motions()
    assert motions[0].tolist() == [[1.0, 0.0, 0.0]]
    worst = [0.0, 0.0]
    for i in range(1, len(offs)):
        true = (-(offs[i][1] - offs[i - 1][1]), -(offs[i][0] - offs[i - 1][0]))              # content moves against the camera
        assert max(abs(true[0]), abs(true[1])) <= 56
        ex, ey = abs(float(motions[i][0, 1]) - true[0]), abs(float(motions[i][0, 2]) - true[1])
        worst = [max(worst[0], ex), max(worst[1], ey)]
        print(f"frame {i}: true {true}, estimate ({float(motions[i][0, 1]):.3f}, {float(motions[i][0, 2]):.3f})")
        # one thumbnail pixel, the search's integer resolution: 640 / 80 and 360 / 48 source pixels
        assert ex <= 8.0 and ey <= 7.5, f"frame {i}: off by ({ex:.2f}, {ey:.2f}) px"
    print(f"worst error: {worst[0]:.3f} px in x, {worst[1]:.3f} px in y")


def _populated(reid_dim=None, T=16, S=3):
    """A state with tracked, lost and free slots: a few frames of a random sequence."""
    frames = tc.sequence(5, streams=S, frames=4, max_det=24, objects=10)
    state = yt.track_state(S, T, "cpu", reid_dim)
    for dets, counts in frames:
        if reid_dim is None:
            yt.track(dets, counts, state)
        else:
            emb = torch.from_numpy(np.random.default_rng(1).normal(size=(S * 24, reid_dim)).astype(np.float32))
            yt.track_reid(dets, counts, state, embed=emb)
    st = state.numpy()[:, 4:4 + T]
    assert (st != 0).any() and (st == 0).any()
    return state


@pytest.mark.parametrize("reid_dim", [None, 64])
def test_warp_twin_matches_restatement(reid_dim):
    T = 16
    state = _populated(reid_dim, T)
    before = state.numpy().copy()
    motion = torch.tensor([[1.0, 12.5, -7.25], [0.5, 3.0, 4.0], [2.0, -1.5, 0.0]])
    for m, ids in ((motion, None), (motion[[1, 2, 0]].contiguous(), [2, 0, 1]), (motion[:2].contiguous(), [1, 7]),
                   (torch.tensor([[1.0, float("nan"), 0.0], [0.0, 1.0, 1.0], [-1.0, 1.0, 1.0]]), None),
                   (torch.tensor([[float("inf"), 1.0, 1.0]]), [2])):
        want = mc.ref_warp(state.numpy(), T, m.numpy(), ids, reid_dim or 0)
        sid = None if ids is None else torch.tensor(ids, dtype=torch.int32)
        for threads in (1, 3):
            got = state.clone()
            assert yt.warp(got, m, T, reid_dim=reid_dim, stream_ids=sid, threads=threads) is got
            assert np.array_equal(got.numpy(), want), f"ids {ids}"
        if not np.isfinite(m.numpy()).all() or (m[:, 0] <= 0).all():
            assert np.array_equal(want, state.numpy()), "an invalid motion changes nothing"
    # s == 1: only x[0], x[1] of the live slots change; the header, the free slots and the gallery never
    got = yt.warp(state.clone(), torch.tensor([[1.0, 12.5, -7.25]] * 3), T, reid_dim=reid_dim).numpy()
    changed = got != before
    assert changed.any()
    fields = changed[:, 4:4 + 24 * T].reshape(-1, 24, T)
    assert not fields[:, [f for f in range(24) if f not in (4, 5)]].any()
    assert not fields[:, :, :][np.broadcast_to((before[:, None, 4:4 + T] == 0), fields.shape)].any()
    assert not changed[:, :4].any() and not changed[:, 4 + 24 * T:].any()
    if reid_dim:
        assert before[:, 4 + 24 * T:].any(), "the galleries must hold features for this to mean anything"
        scaled = yt.warp(state.clone(), motion, T, reid_dim=reid_dim).numpy()
        assert np.array_equal(scaled[:, 4 + 24 * T:], before[:, 4 + 24 * T:])


def _ids_over_shake(motions, boxes, offs):
    """The tracker over the shake -> (ids handed out, per frame {box -> id})."""
    state = yt.track_state(1, 16)
    per_frame = []
    for i, (dets, counts) in enumerate(mc.shake_dets(offs, boxes)):
        if motions is not None:
            yt.warp(state, motions[i], 16)
        r = yt.track(dets, counts, state)
        k = int(r.counts[0])
        per_frame.append({int(d): int(t) for d, t in zip(r.det_index[0, :k].tolist(), r.ids[0, :k].tolist())})
    return int(state[0, 1]), per_frame


def test_warp_keeps_the_ids_over_the_shake():
    offs, boxes, motions = _shake_motions()
    plain, _ = _ids_over_shake(None, boxes, offs)
    assert plain > 5, f"the plain tracker handed out {plain} ids: the shake does not break it"
    warped, per_frame = _ids_over_shake(motions, boxes, offs)
    assert warped == 5
    assert all(f == per_frame[0] and len(f) == 5 for f in per_frame), "every box keeps its id in every frame"
    # Tracker.update(motion=...) is that composition
    trk = yt.Tracker(1, "cpu", max_tracks=16)
    for i, (dets, counts) in enumerate(mc.shake_dets(offs, boxes)):
        r = trk.update(dets, counts, motion=ym.Motion(motions[i], None))
    assert int(trk.state[0, 1]) == 5 and sorted(r.ids[0, :5].tolist()) == [1, 2, 3, 4, 5]


def test_abi_and_argument_errors():
    L = _lib.lib()
    assert L.yh_abi_version() == _lib.ABI_VERSION
    for name in ("yh_motion", "yh_motion_host", "yh_motion_state_bytes", "yh_track_warp", "yh_track_warp_host"):
        assert hasattr(L, name)
    assert L.yh_motion_state_bytes(3, 12, 16) == 3 * (16 + 192) + 32 * 192
    assert L.yh_motion_state_bytes(1, 256, 256) == 0 and L.yh_motion_state_bytes(-1, 12, 16) == 0
    img = np.zeros((36, 64, 3), np.uint8)
    state = ym.motion_state(1, (12, 16))
    state.fill_(0x5A)
    keep = state.numpy().copy()

    def call(frame=None, thumb=(12, 16), radius=2, h=36, w=64, stride=0, fmt=0, plane0=True, batch=1):
        motion = np.full((1, 3), -7, np.float32)
        sad = np.full((1, 2), -7, np.int32)
        d = _lib.YhFrame(img.ctypes.data if plane0 else None, None, h, w, stride, 0, fmt, 0)
        rc = L.yh_motion_host(ctypes.byref(d), batch, None, ctypes.c_void_p(state.data_ptr()), 1, thumb[0], thumb[1], radius,
                              24, ctypes.c_void_p(motion.ctypes.data), ctypes.c_void_p(sad.ctypes.data), 1)
        return rc, motion, sad

    assert call()[0] == 0
    state.copy_(torch.from_numpy(keep))
    for kw in (dict(thumb=(12, 18)), dict(radius=0), dict(radius=33), dict(thumb=(12, 16), radius=5), dict(radius=7),
               dict(thumb=(256, 256)), dict(h=8), dict(w=12), dict(stride=100), dict(fmt=7), dict(plane0=False),
               dict(batch=-1), dict(fmt=1, h=35)):
        rc, motion, sad = call(**kw)
        assert rc == -1 and L.yh_last_error(), kw
        assert (motion == -7).all() and (sad == -7).all() and np.array_equal(state.numpy(), keep), kw
    # yh_track_warp: nothing is written on an error
    ts = yt.track_state(1, 8)
    ts.fill_(3)
    m = np.array([[1, 5, 5]], np.float32)
    for streams, mt, dim, mp, batch in ((1, 0, 0, True, 1), (1, 2000, 0, True, 1), (1, 8, 60, True, 1), (1, 8, 0, False, 1),
                                        (-1, 8, 0, True, 1), (1, 8, 0, True, -1)):
        rc = L.yh_track_warp_host(ctypes.c_void_p(ts.data_ptr()), streams, mt, dim, ctypes.c_void_p(m.ctypes.data) if mp else None,
                                  None, batch, 1)
        assert rc == -1 and L.yh_last_error() and (ts == 3).all()
    with pytest.raises(ValueError):
        yt.warp(yt.track_state(1, 8), torch.zeros((1, 3)), 9)
    with pytest.raises(ValueError):
        ym.MotionEstimator(1, "cpu", thumb=(12, 16), radius=5)
    with pytest.raises(ValueError):
        ym.estimate([img], torch.zeros(100, dtype=torch.uint8), (12, 16), 2)
