"""The tracker's specification restated in numpy (np.float32 operations, one rounding each), and
the frame sequences the tracker tests share.

`RefStream` is one stream's track table and `RefStream.step` the six steps stated at yh_track in
include/yolo_hip.h, with the plain sorted greedy walk for the association. It is the yardstick of
tests/test_track_host.py (the host twin equals it bit for bit) and, through the host twin, of
tests/test_gpu_track.py.

A sequence is a list of frames (dets (S, max_det, 6) f32, counts (S,) i32) as torch tensors; rows
at or beyond a count are NaN in every case, so reading one shows in the outputs.
"""
import functools

import numpy as np
import torch

F = np.float32
P, V, P2, V10 = F(0.05), F(0.00625), F(0.1), F(0.0625)
HALF, TWO, ZERO = F(0.5), F(2.0), F(0.0)

DEFAULTS = dict(track_high=0.25, track_low=0.1, track_new=0.25, iou_first=0.2, iou_second=0.5, iou_tentative=0.3,
                max_age=30, class_aware=True)


def sq(c, u):
    s = c * u
    return s * s


def corners(x):
    """(.., 4) cx, cy, w, h -> x1, y1, x2, y2 as the specification's step 1 computes them."""
    hw, hh = x[..., 2] * HALF, x[..., 3] * HALF
    return x[..., 0] - hw, x[..., 1] - hh, x[..., 0] + hw, x[..., 1] + hh


def measure(row):
    return np.array([(row[0] + row[2]) * HALF, (row[1] + row[3]) * HALF, row[2] - row[0], row[3] - row[1]], dtype=F)


class RefStream:
    def __init__(self, max_tracks, **params):
        self.p = dict(DEFAULTS, **params)
        for k in ("track_high", "track_low", "track_new", "iou_first", "iou_second", "iou_tentative"):
            self.p[k] = F(self.p[k])
        T = self.T = max_tracks
        self.status = np.zeros(T, np.int32)
        self.id = np.zeros(T, np.int32)
        self.last = np.zeros(T, np.int32)
        self.cls = np.zeros(T, F)
        self.x, self.v, self.a, self.b, self.c = (np.zeros((T, 4), F) for _ in range(5))
        self.f = 0
        self.next_id = 1

    def _assoc(self, slots, rows, thr, det, box, mrow, mslot):
        tx1, ty1, tx2, ty2 = (v[:, None] for v in box)
        dx1, dy1, dx2, dy2 = (det[None, :, i] for i in range(4))
        w = np.maximum(ZERO, np.minimum(tx2, dx2) - np.maximum(tx1, dx1))
        h = np.maximum(ZERO, np.minimum(ty2, dy2) - np.maximum(ty1, dy1))
        inter = w * h
        union = ((tx2 - tx1) * (ty2 - ty1) + (dx2 - dx1) * (dy2 - dy1)) - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = inter / union
        assert iou.dtype == F
        cand = slots[:, None] & rows[None, :] & (inter != 0) & (iou >= thr)
        if self.p["class_aware"]:
            cand &= self.cls[:, None] == det[None, :, 5]
        ts, ds = np.nonzero(cand)
        for i in np.lexsort((ds, ts, -iou[ts, ds])):           # iou descending, then slot, then row
            t, d = ts[i], ds[i]
            if mrow[t] < 0 and mslot[d] < 0:
                mrow[t], mslot[d] = d, t

    def step(self, det, max_out):
        """det: (n, 6) f32, the rows below the count. -> out (max_out, 6), ids, det_index, count"""
        p, T = self.p, self.T
        det = np.ascontiguousarray(det, dtype=F)
        n = det.shape[0]
        assert np.isfinite(det).all()
        # step 1
        self.f += 1
        f = self.f
        for t in range(T):
            if self.status[t] == 0:
                continue
            if self.status[t] != 2:
                self.v[t, 3] = ZERO
            wh4 = self.x[t, [2, 3, 2, 3]]
            qp, qv = sq(P, wh4), sq(V, wh4)
            self.x[t] = self.x[t] + self.v[t]
            self.a[t] = ((self.a[t] + TWO * self.b[t]) + self.c[t]) + qp
            self.b[t] = self.b[t] + self.c[t]
            self.c[t] = self.c[t] + qv
        box = corners(self.x)
        # step 2
        score = det[:, 4]
        high = score >= p["track_high"]
        low = (score >= p["track_low"]) & ~high
        # step 3
        mrow, mslot = np.full(T, -1), np.full(n, -1)
        st = self.status
        self._assoc((st == 2) | (st == 3), high, p["iou_first"], det, box, mrow, mslot)
        self._assoc((st == 2) & (mrow < 0), low, p["iou_second"], det, box, mrow, mslot)
        self._assoc(st == 1, high & (mslot < 0), p["iou_tentative"], det, box, mrow, mslot)
        # step 4
        for t in range(T):
            if st[t] == 0:
                continue
            d = mrow[t]
            if d >= 0:
                z = measure(det[d])
                r = sq(P, self.x[t, [2, 3, 2, 3]])
                a, b, c = self.a[t].copy(), self.b[t].copy(), self.c[t].copy()
                S = a + r
                kx, kv = a / S, b / S
                y = z - self.x[t]
                self.x[t] = self.x[t] + kx * y
                self.v[t] = self.v[t] + kv * y
                self.a[t], self.b[t], self.c[t] = a - kx * a, b - kx * b, c - kv * b
                st[t], self.last[t], self.cls[t] = 2, f, det[d, 5]
            elif st[t] == 2:
                st[t] = 3
            elif st[t] == 1:
                st[t] = 0
            if st[t] == 3 and f - self.last[t] > p["max_age"]:
                st[t] = 0
        # step 5
        free = [t for t in range(T) if st[t] == 0]
        births = [d for d in range(n) if high[d] and mslot[d] < 0 and score[d] >= p["track_new"]]
        owner = mslot.copy()                      # row -> the slot that puts it out
        for t, d in zip(free, births):
            z = measure(det[d])
            wh4 = z[[2, 3, 2, 3]]
            self.x[t], self.v[t] = z, ZERO
            self.a[t], self.b[t], self.c[t] = sq(P2, wh4), ZERO, sq(V10, wh4)
            self.id[t] = self.next_id
            self.next_id += 1
            self.last[t], self.cls[t] = f, det[d, 5]
            st[t] = 2 if f == 1 else 1
            owner[d] = t
        # step 6
        out, ids, idx = np.zeros((max_out, 6), F), np.zeros(max_out, np.int32), np.zeros(max_out, np.int32)
        post = corners(self.x)
        k = 0
        for d in range(n):
            t = owner[d]
            if t < 0 or not (st[t] == 2 and self.last[t] == f) or k == max_out:
                continue
            out[k] = [post[0][t], post[1][t], post[2][t], post[3][t], det[d, 4], det[d, 5]]
            ids[k], idx[k] = self.id[t], d
            k += 1
        return out, ids, idx, k


def run_ref(frames, max_tracks, max_out=None, streams=None, stream_ids=None, **params):
    """The restatement over a sequence -> per frame (out (B, max_out, 6), ids, det_index, counts) as
    numpy arrays. stream_ids: per frame a list (or None: row b is stream b)."""
    B, md = frames[0][0].shape[:2]
    streams = B if streams is None else streams
    max_out = md if max_out is None else max_out
    refs = [RefStream(max_tracks, **params) for _ in range(streams)]
    res = []
    for i, (dets, counts) in enumerate(frames):
        sid = list(range(dets.shape[0])) if stream_ids is None or stream_ids[i] is None else stream_ids[i]
        nb = dets.shape[0]
        out = np.zeros((nb, max_out, 6), F)
        ids, idx = np.zeros((nb, max_out), np.int32), np.zeros((nb, max_out), np.int32)
        cnt = np.zeros(nb, np.int32)
        for b, s in enumerate(sid):
            if not 0 <= s < streams:
                continue
            k = min(max(int(counts[b]), 0), md)
            out[b], ids[b], idx[b], cnt[b] = refs[s].step(dets[b, :k].numpy(), max_out)
        res.append((out, ids, idx, cnt))
    return res


def pack(rows_per_stream, max_det, count_override=None):
    """[(n_b, 6) array-likes] -> (dets (B, max_det, 6) f32 with NaN padding, counts (B,) i32)."""
    B = len(rows_per_stream)
    dets = torch.full((B, max_det, 6), float("nan"))
    counts = torch.zeros((B,), dtype=torch.int32)
    for b, rows in enumerate(rows_per_stream):
        r = np.asarray(rows, dtype=F).reshape(-1, 6)[:max_det]
        dets[b, :len(r)] = torch.from_numpy(r)
        counts[b] = len(r)
    if count_override is not None:
        counts = torch.tensor(count_override, dtype=torch.int32)
    return dets, counts


def single(rows_per_frame, max_det=8):
    """One stream: a list of per-frame row lists -> a sequence."""
    return [pack([rows], max_det) for rows in rows_per_frame]


def box(cx, cy, w, h, score=0.9, cls=0.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, cls]


@functools.lru_cache(maxsize=None)
def sequence(seed, streams=3, frames=12, max_det=70, objects=24, classes=3):
    """A random multi-frame sequence: objects on straight lines with jittered boxes (on a 1/4 px
    grid), drop-outs, score dips into the low band, spurious rows, exact duplicates of rows (equal
    IoUs: the tie rules decide) and several classes; the rows of a frame are shuffled. Objects
    are crowded into a small field so that boxes overlap and the greedy order matters."""
    rng = np.random.default_rng(seed)
    seq = []
    pos = rng.uniform(40, 360, size=(streams, objects, 2))
    vel = rng.uniform(-6, 6, size=(streams, objects, 2))
    size = rng.uniform(30, 110, size=(streams, objects, 2))
    cls = rng.integers(0, classes, size=(streams, objects))
    for _ in range(frames):
        per = []
        for s in range(streams):
            rows = []
            for o in range(objects):
                if rng.random() < 0.12:                                   # drop-out
                    continue
                c = pos[s, o] + rng.normal(0, 1.5, 2)
                wh = size[s, o] * rng.uniform(0.95, 1.05, 2)
                score = rng.uniform(0.3, 0.95) if rng.random() > 0.2 else rng.uniform(0.1, 0.25)   # low band
                row = box(c[0], c[1], wh[0], wh[1], score, float(cls[s, o]))
                row[:4] = [round(v * 4) / 4 for v in row[:4]]
                rows.append(row)
                if rng.random() < 0.1:                                    # an exact duplicate, other score
                    rows.append(row[:4] + [rng.uniform(0.3, 0.95), row[5]])
            for _ in range(rng.integers(0, 5)):                           # spurious rows
                c, wh = rng.uniform(20, 380, 2), rng.uniform(20, 120, 2)
                rows.append([round(v * 4) / 4 for v in box(c[0], c[1], wh[0], wh[1])[:4]] +
                            [rng.uniform(0.02, 0.9), float(rng.integers(0, classes))])
            order = rng.permutation(len(rows))
            per.append([rows[i] for i in order])
            pos[s] += vel[s]
        seq.append(pack(per, max_det))
    return tuple(seq)


def run_lib(frames, max_tracks, device="cpu", max_out=None, streams=None, stream_ids=None, threads=1, state=None,
            keep_state=False, **params):
    """The library over a sequence, poisoned reused output buffers -> per frame numpy
    (out, ids, det_index, counts) [+ the state bytes after the frame], and the final state."""
    from yolo_hip import track as yt
    B, md = frames[0][0].shape[:2]
    streams = B if streams is None else streams
    max_out = md if max_out is None else max_out
    p = yt.params(**dict(DEFAULTS, **params))
    if state is None:
        state = yt.track_state(streams, max_tracks, device)
    res = []
    for i, (dets, counts) in enumerate(frames):
        nb = dets.shape[0]
        out = (torch.full((nb, max_out, 6), -7.0, device=device),
               torch.full((nb, max_out), -7, dtype=torch.int32, device=device),
               torch.full((nb, max_out), -7, dtype=torch.int32, device=device),
               torch.full((nb,), -7, dtype=torch.int32, device=device))
        sid = None
        if stream_ids is not None and stream_ids[i] is not None:
            sid = torch.tensor(stream_ids[i], dtype=torch.int32, device=device)
        got = yt.track(dets.to(device), counts.to(device), state, p, stream_ids=sid, max_out=max_out, out=out,
                       threads=threads)
        assert all(g is o for g, o in zip(got, out))
        r = tuple(t.clone() if keep_state else t for t in out)
        res.append(r + ((state.clone(),) if keep_state else ()))
    return [tuple(t.cpu().numpy() for t in r) for r in res], state


def same(got, want, what=""):
    """Bit-for-bit equality of two per-frame result lists (the first four arrays)."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[3], w[3]), f"{what} frame {i}: counts {g[3].tolist()} vs {w[3].tolist()}"
        assert np.array_equal(g[1], w[1]), f"{what} frame {i}: ids"
        assert np.array_equal(g[2], w[2]), f"{what} frame {i}: det_index"
        assert np.isfinite(g[0]).all(), f"{what} frame {i}: a padding row was read"
        assert g[0].tobytes() == w[0].tobytes(), f"{what} frame {i}: out"
