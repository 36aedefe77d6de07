"""Camera-motion compensation on the device (yh_motion, yh_track_warp; marked gpu): the kernels
against their host twins bit for bit - 37 mixed BGR / NV12 frames (two launches) with kept row
strides, three frames per stream, permuted ids -, the tie, window-edge and gate cases, the warp in
both state layouts, a state carried from the host to the device in the middle of a sequence, and
Tracker.update(motion=...) over the shake sequence. The twins are pinned to the numpy restatement in
tests/test_motion_host.py.
"""
import numpy as np
import pytest
import torch

import _motion_cases as mc
import _track_cases as tc
from yolo_hip import motion as ym
from yolo_hip import preprocess as pre
from yolo_hip import track as yt

pytestmark = pytest.mark.gpu


def _to_device(f, gpu):
    """A host frame on the device with its row stride kept: a device buffer as wide as the host's,
    the frame in its leading columns."""
    def wide(t):
        buf = torch.zeros((t.shape[0], t.stride(0) // t.stride(1)) + tuple(t.shape[2:]), dtype=torch.uint8, device=gpu)
        buf[:, :t.shape[1]] = t.to(gpu)
        d = buf[:, :t.shape[1]]
        assert d.stride(0) == t.stride(0)
        return d

    if isinstance(f, pre.NV12):
        return pre.NV12(wide(f.y), wide(f.uv), f.matrix)
    return wide(torch.as_tensor(f))


def _mixed_frames(n, step):
    """n streams over mc.SIZES (the `_mixed_frames` pattern of test_gpu_video.py): BGR and NV12 of both
    matrices, tight and strided -> the host frame of every stream at `step` (0 .. 2)."""
    out = []
    for i in range(n):
        h, w = mc.SIZES[i % len(mc.SIZES)]
        kind = (i // len(mc.SIZES) + i) % 3
        wd = mc.world(300 + i, h + 24, w + 24)
        oy, ox = ((12, 12), (12 + i % 3 - 1, 14 + i % 2), (10, 12 - i % 4))[step]
        if kind == 0 or h % 2 or w % 2:
            out.append(mc.bgr_frame(wd, oy, ox, h, w, pad=5 * (i // 2 % 2)))
        else:
            out.append(mc.nv12_frame(wd, oy, ox, h, w, pad=4 * (i % 3), matrix=601 if kind == 1 else 709))
    return out


@pytest.mark.parametrize("thumb,radius", mc.THUMBS)
def test_device_matches_host_twin(gpu, thumb, radius):
    n = 37                                                  # two launches
    S = n + 2
    hstate, dstate = ym.motion_state(S, thumb), ym.motion_state(S, thumb, gpu)
    for step in range(3):
        host = _mixed_frames(n, step)
        kinds = [isinstance(f, pre.NV12) for f in host]
        assert any(kinds) and not all(kinds)
        ids = [(5 * b + 3) % S for b in range(n)]          # a permutation: 5 and 39 share no factor
        ids[(7 * step + 2) % n] = S + 1 if step else -2      # one row out of range: its stream skips the frame
        assert len(set(ids)) == n
        hid = torch.tensor(ids, dtype=torch.int32)
        want = ym.estimate(host, hstate, thumb, radius, 24, stream_ids=hid, threads=1 + step)
        out = (torch.full((n, 3), -7.0, device=gpu), torch.full((n, 2), -7, dtype=torch.int32, device=gpu))
        dev = [_to_device(f, gpu) if b % 2 == 0 else f for b, f in enumerate(host)]        # device and host sources
        got = ym.estimate(dev, dstate, thumb, radius, 24, stream_ids=hid.to(gpu), out=out)
        torch.cuda.synchronize()
        assert got.motion is out[0]
        assert got.motion.cpu().numpy().tobytes() == want.motion.numpy().tobytes(), f"step {step}: motion"
        assert torch.equal(got.sad.cpu(), want.sad), f"step {step}: sad"
        assert torch.equal(dstate.cpu(), hstate), f"step {step}: state"
    assert (want.motion[:, 1:] != 0).any() and (want.sad[:, 0] > 0).any()


def test_edges_on_the_device(gpu):
    thumb, R = (12, 16), 2
    wd = mc.world(21, 36 + 24, 64 + 24)
    cases = [[mc.flat_frame(36, 64, 90), mc.flat_frame(36, 64, 90)]]
    for sy, sx in ((0, R), (0, -R), (R, 0), (-R, 0), (R, -R)):
        cases.append([mc.bgr_frame(wd, 12, 12, 36, 64), mc.bgr_frame(wd, 12 - 3 * sy, 12 - 4 * sx, 36, 64)])
    # the gate: unrelated content, gated and raw
    a = mc.bgr_frame(mc.world(31, 114, 184), 12, 12, 90, 160)
    b = mc.bgr_frame(mc.world(32, 114, 184), 12, 12, 90, 160)
    for frames, th, r, mad in [(c, thumb, R, -1) for c in cases] + [([a, b], (24, 40), 4, 8), ([a, b], (24, 40), 4, -1)]:
        hs, ds = ym.motion_state(1, th), ym.motion_state(1, th, gpu)
        for f in frames:
            want = ym.estimate([f], hs, th, r, mad)
            got = ym.estimate([f], ds, th, r, mad)
        assert got.motion.cpu().numpy().tobytes() == want.motion.numpy().tobytes()
        assert torch.equal(got.sad.cpu(), want.sad) and torch.equal(ds.cpu(), hs)
    assert got.sad[0, 0].item() > 8 * 16 * 32                                            # the last two: beyond the gate
    flat = ym.MotionEstimator(1, gpu, thumb=thumb, radius=R)
    flat.estimate([cases[0][0]])
    r = flat.estimate([cases[0][1]])
    assert r.motion.cpu().tolist() == [[1.0, 0.0, 0.0]] and r.sad.cpu().tolist() == [[0, 0]]


@pytest.mark.parametrize("h,w,thumb,radius,nv12", [
    (130, 300, (128, 256), 32, True),      # the largest thumbnail and radius
    (4096, 8, (4096, 8), 2, False),        # the tallest thumbnail: the search's largest LDS request
    (16, 8400, (12, 16), 2, True),         # wider than a workgroup's column sums: the thumbnail row in two chunks
    (14, 8400, (12, 16), 2, False),
])
def test_caps_and_wide_frames(gpu, h, w, thumb, radius, nv12):
    wd = mc.world(50 + h, h + 8, w + 8)
    make = mc.nv12_frame if nv12 else mc.bgr_frame
    hs, ds = ym.motion_state(1, thumb), ym.motion_state(1, thumb, gpu)
    for oy, ox in ((4, 4), (4 + min(2, h // thumb[0]), 4 - min(3, w // thumb[1]))):
        f = make(wd, oy, ox, h, w)
        want = ym.estimate([f], hs, thumb, radius, -1)
        got = ym.estimate([f], ds, thumb, radius, -1)
    assert got.motion.cpu().numpy().tobytes() == want.motion.numpy().tobytes()
    assert torch.equal(got.sad.cpu(), want.sad) and torch.equal(ds.cpu(), hs)
    assert want.sad[0, 1] > 0


@pytest.mark.parametrize("reid_dim", [None, 64])
def test_warp_matches_host_twin(gpu, reid_dim):
    T, S = 16, 3
    frames = tc.sequence(5, streams=S, frames=4, max_det=24, objects=10)
    state = yt.track_state(S, T, "cpu", reid_dim)
    emb = None if reid_dim is None else torch.from_numpy(np.random.default_rng(1).normal(size=(S * 24, reid_dim)).astype(np.float32))
    for dets, counts in frames:
        yt.track(dets, counts, state) if reid_dim is None else yt.track_reid(dets, counts, state, embed=emb)
    assert (state[:, 4:4 + T] != 0).any()
    motion = torch.tensor([[1.0, 12.5, -7.25], [0.5, 3.0, 4.0], [2.0, -1.5, 0.0]])
    for m, ids in ((motion, None), (motion[:2].contiguous(), [2, 0]), (motion[:2].contiguous(), [1, 7]),
                   (torch.tensor([[1.0, float("nan"), 0.0], [0.0, 1.0, 1.0], [float("inf"), 1.0, 1.0]]), None)):
        sid = None if ids is None else torch.tensor(ids, dtype=torch.int32)
        want = yt.warp(state.clone(), m, T, reid_dim=reid_dim, stream_ids=sid)
        got = yt.warp(state.to(gpu), m.to(gpu), T, reid_dim=reid_dim, stream_ids=None if sid is None else sid.to(gpu))
        assert torch.equal(got.cpu(), want), f"ids {ids}"
    assert not torch.equal(want, yt.warp(state.clone(), motion, T, reid_dim=reid_dim))


def test_state_moves_from_host_to_device_mid_sequence(gpu):
    thumb, R = (24, 40), 4
    streams = mc.mixed_streams(thumb)
    S = len(streams)
    hs = ym.motion_state(S, thumb)
    ym.estimate([s[0] for s in streams], hs, thumb, R)
    ds = hs.to(gpu)                                          # frame 0 on the host, the rest on the device
    for i in (1, 2):
        want = ym.estimate([s[i] for s in streams], hs, thumb, R)
        got = ym.estimate([s[i] for s in streams], ds, thumb, R)
        assert got.motion.cpu().numpy().tobytes() == want.motion.numpy().tobytes() and torch.equal(got.sad.cpu(), want.sad)
        assert torch.equal(ds.cpu(), hs)
    assert (want.motion[:, 1:] != 0).any()


def test_tracker_with_motion_over_the_shake(gpu):
    offs, frames, boxes = mc.shake()
    hest = ym.MotionEstimator(1, "cpu", thumb=mc.SHAKE_THUMB, radius=mc.SHAKE_R)
    dest = ym.MotionEstimator(1, gpu, thumb=mc.SHAKE_THUMB, radius=mc.SHAKE_R)
    htrk, dtrk = yt.Tracker(1, "cpu", max_tracks=16), yt.Tracker(1, gpu, max_tracks=16)
    dframes = [torch.from_numpy(np.ascontiguousarray(f)).to(gpu) for f in frames]
    first = None
    for i, (dets, counts) in enumerate(mc.shake_dets(offs, boxes)):
        hm = hest.estimate([frames[i]])
        yt.warp(htrk.state, hm, 16)                          # the host composition, call by call
        want = yt.track(dets, counts, htrk.state, htrk.params)
        got = dtrk.update(dets.to(gpu), counts.to(gpu), motion=dest.estimate([dframes[i]]))
        for g, w in zip(got, want):
            assert g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"frame {i}"
        assert torch.equal(dtrk.state.cpu(), htrk.state), f"frame {i}: state"
        k = int(want.counts[0])
        ids = dict(zip(want.det_index[0, :k].tolist(), want.ids[0, :k].tolist()))
        first = ids if first is None else first
        assert k == 5 and ids == first, f"frame {i}: a box changed its id"
    assert int(dtrk.state[0, 1].item()) == 5
