"""The track-propagation rules restated in numpy (yh_propagate_remember and yh_propagate in
include/yolo_hip.h), and the cases the propagation tests share. TEST INFRASTRUCTURE ONLY.

`RefPropagate` is the state and its two calls: the geometry of a box, the box-mean cells with edge
replication, the SAD of every shift, the smallest (SAD, |dy| + |dx|, dy, dx), the fp32 refinement
and box move (np.float32 operations, one rounding each), the gate, the ordered compaction, the state
bytes. Luma, the candidates' order and the refinement are yh_motion's, taken from _motion_cases.
tests/test_propagate_host.py holds the host twin to it bit for bit, tests/test_gpu_propagate.py the
kernels to the host twin. A case is a list of steps on one state; `run` plays it through the library.
"""
import functools

import numpy as np
import torch

import _motion_cases as mc
from yolo_hip import propagate as yp

F = np.float32
P, CMAX, HDR = 32, 32, 16
ENTRY = np.dtype([("id", "<i4"), ("box0", "<f4", 4), ("score", "<f4"), ("cls", "<f4"), ("cw", "<i4"), ("ch", "<i4"),
                  ("ox0", "<i4"), ("oy0", "<i4"), ("ox", "<i4"), ("oy", "<i4"), ("zero", "<i4", 3), ("tmpl", "u1", (P, P))])
assert ENTRY.itemsize == 1088


# ---------------------------------------------------------------- the rules
def axis(lo, hi):
    """Rule 2 along one axis -> (cell size, origin)."""
    lo, hi = (F(-2 ** 20) if not v >= -2 ** 20 else min(F(v), F(2 ** 20)) for v in (lo, hi))
    b0, b1 = int(np.floor(lo)), int(np.ceil(hi))
    c = min(max((max(1, b1 - b0) + 16) // 32, 1), CMAX)
    return c, ((b0 + b1) >> 1) - 16 * c


def cells(y, oy, ox, ch, cw, lo, hi):
    """The cells (i, j) in [lo, hi)^2 of luma y relative to (oy, ox), coordinates clamped."""
    rows = np.clip(oy + np.arange(lo * ch, hi * ch), 0, y.shape[0] - 1)
    cols = np.clip(ox + np.arange(lo * cw, hi * cw), 0, y.shape[1] - 1)
    s = y[np.ix_(rows, cols)].astype(np.int64).reshape(hi - lo, ch, hi - lo, cw).sum((1, 3))
    return ((s + cw * ch // 2) // (cw * ch)).astype(np.uint8)


class RefPropagate:
    def __init__(self, streams, max_tracks):
        self.S, self.T = streams, max_tracks
        self.state = np.zeros((streams, HDR + ENTRY.itemsize * max_tracks), np.uint8)

    def _table(self, s):
        return self.state[s, :4].view(np.uint32), self.state[s, HDR:].view(ENTRY)

    def remember(self, frames, dets, ids, counts, stream_ids=None):
        for b, f in enumerate(frames):
            s = b if stream_ids is None else int(stream_ids[b])
            if not 0 <= s < self.S:
                continue
            n, tab = self._table(s)
            y = mc.luma(f)
            self.state[s, :HDR] = 0
            n[0] = min(max(int(counts[b]), 0), dets.shape[1], self.T)
            for r in range(int(n[0])):
                e = tab[r]
                e["id"], e["box0"], e["score"], e["cls"], e["zero"] = ids[b, r], dets[b, r, :4], dets[b, r, 4], dets[b, r, 5], 0
                e["cw"], e["ox0"] = axis(dets[b, r, 0], dets[b, r, 2])
                e["ch"], e["oy0"] = axis(dets[b, r, 1], dets[b, r, 3])
                e["ox"], e["oy"] = e["ox0"], e["oy0"]
                e["tmpl"] = cells(y, int(e["oy"]), int(e["ox"]), int(e["ch"]), int(e["cw"]), 0, P)

    def propagate(self, frames, R, max_mad, stream_ids=None, max_out=None):
        B, mo = len(frames), self.T if max_out is None else max_out
        dets, ids = np.zeros((B, mo, 6), F), np.zeros((B, mo), np.int32)
        sad, counts = np.zeros((B, mo), np.int32), np.zeros((B,), np.int32)
        for b, f in enumerate(frames):
            s = b if stream_ids is None else int(stream_ids[b])
            if not 0 <= s < self.S:
                continue
            n, tab = self._table(s)
            y = mc.luma(f)
            H, W = y.shape
            kept = []
            for k in range(int(n[0])):
                e = tab[k].copy()
                cw, ch = int(e["cw"]), int(e["ch"])
                Wn = cells(y, int(e["oy"]), int(e["ox"]), ch, cw, -R, P + R).astype(np.int64)
                win = np.lib.stride_tricks.sliding_window_view(Wn, (P, P))
                t = np.abs(win - e["tmpl"].astype(np.int64)).sum((2, 3))
                s0, _, dy, dx = mc.best_shift(t, R)
                fx = mc.refine(s0, int(t[dy + R, dx + R - 1]), int(t[dy + R, dx + R + 1])) if abs(dx) < R else F(0)
                fy = mc.refine(s0, int(t[dy + R - 1, dx + R]), int(t[dy + R + 1, dx + R])) if abs(dy) < R else F(0)
                e["ox"], e["oy"] = e["ox"] + dx * cw, e["oy"] + dy * ch
                mx = F(int(e["ox"]) - int(e["ox0"])) + fx * F(cw)
                my = F(int(e["oy"]) - int(e["oy0"])) + fy * F(ch)
                box = e["box0"] + np.array([mx, my, mx, my], F)
                cx, cy = F(0.5) * (box[0] + box[2]), F(0.5) * (box[1] + box[3])
                assert box.dtype == F and cx.dtype == F
                if (max_mad >= 0 and s0 > max_mad * P * P) or not (0 <= cx < W and 0 <= cy < H):
                    continue
                if len(kept) < mo:
                    dets[b, len(kept)] = (*box, e["score"], e["cls"])
                    ids[b, len(kept)], sad[b, len(kept)] = e["id"], s0
                kept.append(e)
            old = int(n[0])
            tab[:old] = np.zeros((), ENTRY)
            tab[:len(kept)] = np.array(kept, ENTRY) if kept else tab[:0]
            n[0] = len(kept)
            counts[b] = min(len(kept), mo)
        return dets, ids, sad, counts


# ---------------------------------------------------------------- cases
def tracks(rows, max_det=None, counts=None):
    """Tracker-shaped rows from per-batch-row lists of boxes -> (dets (B, md, 6), ids (B, md), counts);
    ids 1, 2, .. per row, the rows beyond the boxes NaN (they must never be read)."""
    md = max_det or max(1, max(len(r) for r in rows))
    dets, ids = np.full((len(rows), md, 6), np.nan, F), np.zeros((len(rows), md), np.int32)
    for b, r in enumerate(rows):
        for k, box in enumerate(r[:md]):
            dets[b, k] = (*box, 0.5 + 0.001 * k, k % 3)
            ids[b, k] = 100 * b + k + 1
    return dets, ids, np.array([len(r) for r in rows] if counts is None else counts, np.int32)


def _frame(kind, seed, oy, ox):
    if kind == "nv12":
        return mc.nv12_frame(mc.world(seed, 96 + 64, 128 + 64), 32 + oy, 32 + ox, 96, 128, pad=4)
    if kind == "bgr4":               # rows of 384 bytes: the only BGR frames here whose rows the device loads as dwords
        return mc.bgr_frame(mc.world(seed, 96 + 64, 128 + 64), 32 + oy, 32 + ox, 96, 128)
    return mc.bgr_frame(mc.world(seed, 97 + 64, 131 + 64), 32 + oy, 32 + ox, 97, 131, pad=0 if seed % 2 else 5)


# boxes with (cw, ch) of (1, 1) and (3, 2), one clamped at CMAX, one hanging over each frame edge
GEOMETRY = [(40, 30, 72, 62), (10.3, 10.2, 106.1, 73.9), (-900, -900, 1100, 1100), (-20, 30, 12, 62),
            (112, 30, 150, 70), (50, -15, 82, 17), (50, 80, 90, 112.5)]


def _geometry(kind, R):
    f = [_frame(kind, 11, *o) for o in ((0, 0), (1, -1), (1, -2), (0, 1))]
    t0, t2 = tracks([GEOMETRY]), tracks([GEOMETRY[::-1]])
    return dict(S=1, T=8, R=R, mad=24, steps=[("r", [f[0]], t0, None), ("p", [f[1]], None), ("p", [f[2]], None),
                                               ("r", [f[2]], t2, None), ("p", [f[3]], None)])


def _shift(box, sy, sx, R, flat=False):
    """One box, the content moved by (sx, sy) of its cells between the two frames."""
    (cw, _), (ch, _) = axis(box[0], box[2]), axis(box[1], box[3])
    a, b = (mc.flat_frame(97, 131, 90),) * 2 if flat else (_frame("bgr", 21, 0, 0), _frame("bgr", 21, -sy * ch, -sx * cw))
    return dict(S=1, T=2, R=R, mad=24, steps=[("r", [a], tracks([[box]]), None), ("p", [b], None)], planted=(sx * cw, sy * ch))


def _batch(T, counts, seed=5):
    """3 batch rows over 4 streams, permuted ids with one out of range; a patch of unrelated content
    in the later frames puts some entries beyond the gate: the compaction moves the others."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(3):
        xy = rng.uniform(-10, 100, (80, 2))
        wh = rng.uniform(8, 70, (80, 2))
        rows.append([(x, y, x + w, y + h) for (x, y), (w, h) in zip(xy, wh)])
    def frames(step):
        out = [_frame(("bgr", "nv12", "bgr4")[b], 30 + b, step % 2, -step) for b in range(3)]
        if step:
            out[0][20:70, 30:90] = mc.world(77, 97, 131)[20:70, 30:90]
        return out
    ids0, ids1 = [2, 7, 0], [0, 3, -1]
    return dict(S=4, T=T, R=2, mad=12, steps=[
        ("r", frames(0), tracks(rows, 80, counts), ids0), ("p", frames(1), ids0), ("p", frames(2), ids0),
        ("r", frames(2), tracks(rows[::-1], 80, counts[::-1]), ids1), ("p", frames(3), ids1), ("p", frames(1), ids0)])


CASES = {
    "geometry-bgr": lambda: _geometry("bgr", 2),
    "geometry-nv12": lambda: _geometry("nv12", 3),
    "geometry-bgr4": lambda: _geometry("bgr4", 3),
    **{f"shift{sy:+d}{sx:+d}": (lambda sy=sy, sx=sx: _shift(GEOMETRY[1], sy, sx, 2))
       for sy, sx in ((2, 0), (-2, 0), (0, 2), (0, -2), (2, -2), (1, -1))},
    "shift-beyond": lambda: _shift(GEOMETRY[1], 0, 4, 2),
    "flat": lambda: _shift(GEOMETRY[0], 0, 0, 2, flat=True),
    "radius8": lambda: _shift(GEOMETRY[0], -8, 8, 8),
    "radius16": lambda: _shift(GEOMETRY[0], 16, -3, 16),
    "batch70": lambda: _batch(70, [0, 1, 70]),
    "batch-over": lambda: _batch(70, [80, 75, 3]),
    "batch1": lambda: _batch(1, [3, 0, 1]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement over a case -> per step (outputs or None, state bytes)."""
    c = case(name)
    ref, res = RefPropagate(c["S"], c["T"]), []
    for op, frames, arg, *ids in c["steps"]:
        out = ref.remember(frames, *arg, ids[0]) if op == "r" else ref.propagate(frames, c["R"], c["mad"], arg)
        res.append((out, ref.state.copy()))
    return res


def run(name, device="cpu", threads=1, move_at=None):
    """A case through the library on `device` -> per step (outputs or None, state bytes), as `reference`.
    move_at: play the steps before it on the CPU, then carry the state to `device`."""
    c = case(name)
    state = yp.propagate_state(c["S"], c["T"], "cpu" if move_at is not None else device)
    res = []
    for i, (op, frames, arg, *ids) in enumerate(c["steps"]):
        if i == move_at:
            state = state.to(device)
        dev = state.device
        sid = ids[0] if op == "r" else arg
        sid = None if sid is None else torch.tensor(sid, dtype=torch.int32, device=dev)
        out = None
        if op == "r":
            yp.remember(frames, tuple(torch.from_numpy(a).to(dev) for a in arg), state, stream_ids=sid, threads=threads)
        else:
            B = len(frames)
            bufs = (torch.full((B, c["T"], 6), -7.0, device=dev), *(torch.full((B, c["T"]), -7, dtype=torch.int32, device=dev)
                    for _ in range(2)), torch.full((B,), -7, dtype=torch.int32, device=dev))
            out = tuple(t.cpu().numpy() for t in yp.propagate(frames, state, c["R"], c["mad"], stream_ids=sid, out=bufs,
                                                             threads=threads))
        res.append((out, state.cpu().numpy().copy()))
    return res


def same(got, want, what):
    assert len(got) == len(want)
    for i, ((go, gs), (wo, ws)) in enumerate(zip(got, want)):
        for g, w, field in zip(go or (), wo or (), ("dets", "ids", "sad", "counts")):
            assert g.tobytes() == w.tobytes(), f"{what} step {i}: {field}\n{g}\nvs\n{w}"
        assert np.array_equal(gs, ws), f"{what} step {i}: state differs at bytes {np.argwhere(gs != ws)[:8].tolist()}"
