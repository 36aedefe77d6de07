"""The camera-motion rules restated in numpy (yh_motion and yh_track_warp in include/yolo_hip.h), and
the frames the motion tests share. TEST INFRASTRUCTURE ONLY.

`RefMotion` is the state of yh_motion and `RefMotion.step` one call: luma, box-mean thumbnail, the
SAD of every shift, the smallest (SAD, |dy| + |dx|, dy, dx), the fp32 refinement (np.float32
operations, one rounding each), the gate, the state bytes including the staging area. `ref_warp` is
yh_track_warp on a state tensor. tests/test_motion_host.py holds the host twin to them bit for bit,
and tests/test_gpu_motion.py the kernels to the host twin.

Frames are windows of a world larger than the frame - blocky texture at several scales, three
channels - at a camera offset: content is world-static, so a camera that moves by (ax, ay) between
two frames moves the content by (-ax, -ay).
"""
import functools

import numpy as np
import torch

from yolo_hip import preprocess as pre

F = np.float32
HDR, LAUNCH = 16, 32


# ---------------------------------------------------------------- the rules
def luma(frame):
    """(h, w) uint8 luma of a frame: an (h, w, 3) BGR array / tensor or a pre.NV12."""
    if isinstance(frame, pre.NV12):
        return frame.y.cpu().numpy()
    a = torch.as_tensor(frame).cpu().numpy().astype(np.uint32)
    return ((1868 * a[..., 0] + 9617 * a[..., 1] + 4899 * a[..., 2] + 8192) >> 14).astype(np.uint8)


def thumbnail(y, th, tw):
    H, W = y.shape
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = y.astype(np.int64).cumsum(0).cumsum(1)
    r = (np.arange(th + 1) * H) // th
    c = (np.arange(tw + 1) * W) // tw
    s = ii[r[1:, None], c[None, 1:]] - ii[r[:-1, None], c[None, 1:]] - ii[r[1:, None], c[None, :-1]] + ii[r[:-1, None], c[None, :-1]]
    n = (r[1:] - r[:-1])[:, None] * (c[1:] - c[:-1])[None, :]
    assert (n > 0).all()
    return ((s + n // 2) // n).astype(np.uint8)


def sad_table(C, P, R):
    th, tw = C.shape
    win = C[R:th - R, R:tw - R].astype(np.int64)
    t = np.zeros((2 * R + 1, 2 * R + 1), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            t[dy + R, dx + R] = np.abs(win - P[R - dy:th - R - dy, R - dx:tw - R - dx].astype(np.int64)).sum()
    return t


def best_shift(t, R):
    return min((int(t[dy + R, dx + R]), abs(dy) + abs(dx), dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))


def refine(s0, sm, sp):
    den = (sm - s0) + (sp - s0)
    if den <= 0:
        return F(0)
    return (F(0.5) * F(sm - sp)) / F(den)


def result(t, R, H, W, th, tw, max_mad):
    s0, _, dy, dx = best_shift(t, R)
    sad = np.array([s0, t[R, R]], np.int32)
    if max_mad >= 0 and s0 > max_mad * (th - 2 * R) * (tw - 2 * R):
        return np.array([1, 0, 0], F), sad
    fx = refine(s0, int(t[dy + R, dx + R - 1]), int(t[dy + R, dx + R + 1])) if abs(dx) < R else F(0)
    fy = refine(s0, int(t[dy + R - 1, dx + R]), int(t[dy + R + 1, dx + R])) if abs(dy) < R else F(0)
    tx = (F(dx) + fx) * (F(W) / F(tw))
    ty = (F(dy) + fy) * (F(H) / F(th))
    assert tx.dtype == F and ty.dtype == F
    return np.array([1, tx, ty], F), sad


class RefMotion:
    def __init__(self, streams, thumb):
        self.S, (self.th, self.tw) = streams, thumb
        self.n = self.th * self.tw
        self.state = np.zeros(streams * (HDR + self.n) + LAUNCH * self.n, np.uint8)

    def step(self, frames, radius, max_mad, stream_ids=None):
        B, th, tw, n = len(frames), self.th, self.tw, self.n
        motion = np.tile(np.array([1, 0, 0], F), (B, 1))
        sad = np.zeros((B, 2), np.int32)
        for b, f in enumerate(frames):
            s = b if stream_ids is None else int(stream_ids[b])
            if not 0 <= s < self.S:
                continue
            y = luma(f)
            C = thumbnail(y, th, tw)
            blk = self.state[s * (HDR + n):(s + 1) * (HDR + n)]
            if blk[:4].view(np.uint32)[0]:
                P = blk[HDR:].reshape(th, tw)
                motion[b], sad[b] = result(sad_table(C, P, radius), radius, y.shape[0], y.shape[1], th, tw, max_mad)
            blk[:HDR] = 0
            blk[0] = 1
            blk[HDR:] = C.reshape(-1)
            st = self.S * (HDR + n) + (b % LAUNCH) * n
            self.state[st:st + n] = C.reshape(-1)
        return motion, sad


def valid_motion(m):
    return bool(np.isfinite(m).all() and m[0] > 0)


def ref_warp(state, max_tracks, motion, stream_ids=None, reid_dim=0):
    """yh_track_warp on a copy of a (streams, words) int32 state array -> the new array."""
    T = max_tracks
    out = state.copy()
    for b in range(motion.shape[0]):
        s = b if stream_ids is None else int(stream_ids[b])
        m = motion[b].astype(F)
        if not 0 <= s < state.shape[0] or not valid_motion(m):
            continue
        w = out[s]
        fld = w[4:4 + 24 * T].view(F).reshape(24, T)      # a view: writes land in out
        live = w[4:4 + T] != 0
        sc, s2 = m[0], m[0] * m[0]
        x = fld[4:8]
        x[0, live] = sc * x[0, live] + m[1]
        x[1, live] = sc * x[1, live] + m[2]
        x[2, live] = sc * x[2, live]
        x[3, live] = sc * x[3, live]
        fld[8:12, live] = sc * fld[8:12, live]
        fld[12:24, live] = s2 * fld[12:24, live]
    return out


# ---------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def world(seed, h, w):
    """(h, w, 3) uint8: blocks of 64, 24 and 8 pixels on top of each other, a little pixel noise."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w, 3))
    for size, amp in ((64, 90), (24, 70), (8, 50)):
        g = rng.uniform(0, amp, (h // size + 2, w // size + 2, 3))
        acc += np.repeat(np.repeat(g, size, 0), size, 1)[:h, :w]
    acc += rng.uniform(0, 20, (h, w, 3))
    out = np.clip(acc, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def bgr_frame(wd, oy, ox, h, w, pad=0):
    """The h x w window of the world at camera offset (ox, oy) as a BGR frame; pad > 0: a view of a
    wider buffer (strided rows)."""
    buf = np.zeros((h, w + pad, 3), np.uint8)
    buf[:, :w] = wd[oy:oy + h, ox:ox + w]
    return buf[:, :w]


def nv12_frame(wd, oy, ox, h, w, pad=0, matrix=601):
    """The same window as NV12: Y is the world's channel 1, the chroma its other channels at half
    resolution (the luma rules never read it)."""
    yb = np.zeros((h, w + pad), np.uint8)
    ub = np.zeros((h // 2, w + pad), np.uint8)
    yb[:, :w] = wd[oy:oy + h, ox:ox + w, 1]
    ub[:, 0:w:2] = wd[oy:oy + h:2, ox:ox + w:2, 0]
    ub[:, 1:w:2] = wd[oy:oy + h:2, ox:ox + w:2, 2]
    return pre.NV12(yb[:, :w], ub[:, :w], matrix)


def flat_frame(h, w, value):
    return np.full((h, w, 3), value, np.uint8)


SIZES = ((36, 64), (90, 160), (33, 101))          # the last is odd-sized: BGR only
THUMBS = (((12, 16), 2), ((24, 40), 4))


def mixed_streams(thumb):
    """Streams of 3 frames each over SIZES, BGR and NV12 of both matrices, tight and strided rows,
    the camera moving a few pixels between frames -> [per stream: 3 frames]."""
    th, tw = thumb
    streams = []
    k = 0
    for h, w in SIZES:
        for kind in ("bgr", "nv12-601", "nv12-709", "bgr"):
            if kind != "bgr" and (h % 2 or w % 2):
                continue
            wd = world(7 + k, h + 24, w + 24)
            pad = (0, 5, 8, 3)[k % 4]
            offs = [(12, 12), (12 + (k % 3) - 1, 12 + 2 + k % 2), (12 - 2, 12 - (k % 4))]
            if kind == "bgr":
                streams.append([bgr_frame(wd, oy, ox, h, w, pad) for oy, ox in offs])
            else:
                streams.append([nv12_frame(wd, oy, ox, h, w, pad, int(kind[-3:])) for oy, ox in offs])
            k += 1
    return streams


# the shake: a 640 x 360 camera over a world with five world-static 40 x 80 boxes, 12 frames, the
# camera moving by at most 56 pixels per frame and axis
SHAKE_HW, SHAKE_THUMB, SHAKE_R = (360, 640), (48, 80), 8


@functools.lru_cache(maxsize=None)
def shake(seed=3, frames=12, step=56, span=160):
    """-> (offsets [(oy, ox)], frames [BGR arrays], boxes (5, 4) world x1 y1 x2 y2)"""
    rng = np.random.default_rng(seed)
    h, w = SHAKE_HW
    wd = world(100 + seed, h + span, w + span)
    offs = [(span // 2, span // 2)]
    while len(offs) < frames:
        oy, ox = offs[-1]
        ny, nx = oy + int(rng.integers(-step, step + 1)), ox + int(rng.integers(-step, step + 1))
        if 0 <= ny <= span and 0 <= nx <= span and max(abs(ny - oy), abs(nx - ox)) >= step // 2:
            offs.append((ny, nx))
    centres = [(span + 100, span // 2 + 150), (span + 300, span // 2 + 60), (span + 420, span // 2 + 200),
               (span + 200, span // 2 + 260), (span + 520, span // 2 + 120)]
    boxes = np.array([[cx - 20, cy - 40, cx + 20, cy + 40] for cx, cy in centres], F)
    return tuple(offs), tuple(bgr_frame(wd, oy, ox, h, w) for oy, ox in offs), boxes


def shake_dets(offs, boxes, max_det=8):
    """Per frame (dets (1, max_det, 6) f32 with NaN padding, counts (1,) i32): the boxes in frame pixels."""
    out = []
    for oy, ox in offs:
        d = torch.full((1, max_det, 6), float("nan"))
        rows = np.concatenate([boxes - np.array([ox, oy, ox, oy], F), np.full((len(boxes), 1), 0.9, F),
                               np.zeros((len(boxes), 1), F)], 1)
        d[0, :len(boxes)] = torch.from_numpy(rows)
        out.append((d, torch.tensor([len(boxes)], dtype=torch.int32)))
    return out
