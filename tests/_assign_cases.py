"""yh_assign's specification restated in numpy, the tracker's restatements extended with the
OPTIMAL association, and the cases the assignment tests share.

`solve` is the algorithm stated at yh_assign in include/yolo_hip.h - successive shortest augmenting
paths with one private "stay unmatched" column per slot - written over whole columns at a time; it
is the yardstick of tests/test_assign_host.py (the host twin equals it byte for byte) and, through
the host twin, of tests/test_gpu_assign.py. `RefAssignStream` / `RefAssignReidStream` are
`_track_cases.RefStream` / `_reid_cases.RefReidStream` whose associations, in "optimal" mode, keep
the candidate pairs and hand their weights to `solve` instead of walking them.
"""
import functools

import numpy as np
import torch

import _reid_cases as rc
import _track_cases as tc

F = np.float32
M = 1 << 16                      # YH_ASSIGN_MAX_WEIGHT
INF = int(np.iinfo(np.int32).max)


def solve(W, nt=None, nd=None):
    """W (T, D) integers -> row_of_slot (T,), slot_of_row (D,) int32 by the normative algorithm."""
    W = np.asarray(W)
    T, D = W.shape
    nt = T if nt is None else min(max(int(nt), 0), T)
    nd = D if nd is None else min(max(int(nd), 0), D)
    w = np.clip(W[:nt, :nd].astype(np.int64), 0, M)            # only this corner is read
    u, v = np.zeros(nt, np.int64), np.zeros(nd, np.int64)
    ros, sor = np.full(T, -1, np.int32), np.full(D, -1, np.int32)
    for root in range(nt):
        dist = np.full(nd, INF, np.int64)
        pred = np.full(nd, -1, np.int64)
        done = np.zeros(nd, bool)
        i, base = root, 0
        pdist, pslot = INF, -1
        end, total = -1, None
        for _ in range(nd + 1):
            pd = base + M - u[i]                                # a.
            if pd < pdist or (pd == pdist and i < pslot):
                pdist, pslot = pd, i
            cand = base + (M - w[i]) - u[i] - v                 # b.
            better = ~done & (w[i] > 0) & (cand < dist)
            dist[better] = cand[better]
            pred[better] = i
            open_ = np.where(done, INF + 1, dist)               # c. (argmin: the first of equal minima)
            bj = int(np.argmin(open_)) if nd else -1
            if bj < 0 or open_[bj] > pdist:
                total = pdist
                break
            done[bj] = True                                     # d.
            if sor[bj] < 0:
                end, total = bj, dist[bj]
                break
            i, base = int(sor[bj]), dist[bj]
        assert total is not None and 0 <= total <= M
        u[root] += total
        for d in np.nonzero(done)[0]:
            if d != end:
                delta = total - dist[d]
                u[sor[d]] += delta
                v[d] -= delta
        assert np.abs(u).max(initial=0) < 1 << 27 and np.abs(v).max(initial=0) < 1 << 27
        d = end
        if d < 0:
            t = pslot
            d = ros[t]
            ros[t] = -1
            if t == root:
                continue
        while True:
            t = int(pred[d])
            nxt = ros[t]
            ros[t], sor[d] = d, t
            if t == root:
                break
            d = nxt
    return ros, sor


def solve_batch(weights, t_counts=None, d_counts=None):
    """(P, T, D) -> (row_of_slot (P, T), slot_of_row (P, D)) int32"""
    P, T, D = weights.shape
    ros, sor = np.full((P, T), -1, np.int32), np.full((P, D), -1, np.int32)
    for p in range(P):
        ros[p], sor[p] = solve(weights[p], None if t_counts is None else t_counts[p],
                               None if d_counts is None else d_counts[p])
    return ros, sor


def live(weights, t_counts, d_counts, p):
    """The clamped corner of problem p that takes part."""
    _, T, D = weights.shape
    nt = T if t_counts is None else min(max(int(t_counts[p]), 0), T)
    nd = D if d_counts is None else min(max(int(d_counts[p]), 0), D)
    return np.clip(weights[p, :nt, :nd].astype(np.int64), 0, M)


def greedy_total(w):
    """The weight of the sorted greedy walk (weight descending, then slot, then row) on w (nt, nd)."""
    ts, ds = np.nonzero(w > 0)
    used_t, used_d, total = set(), set(), 0
    for k in np.lexsort((ds, ts, -w[ts, ds])):
        t, d = int(ts[k]), int(ds[k])
        if t not in used_t and d not in used_d:
            used_t.add(t)
            used_d.add(d)
            total += int(w[t, d])
    return total


def sparse(T, D, seed, per=4):
    """At most `per` allowed pairs per slot, in clusters along the diagonal, as IoU gating gives."""
    rng = np.random.default_rng(seed)
    w = np.zeros((T, D), np.int32)
    for t in range(T):
        centre = t * D // T
        for d in rng.integers(centre - 3, centre + 4, per):
            if 0 <= d < D:
                w[t, d] = rng.integers(1, M + 1) if rng.random() < 0.7 else rng.choice([M // 3, M // 2, M])
    return w


def band(n):
    """Slot i allows rows i (1000) and i + 1 (1001); the last slot only its own row: its path moves
    every earlier slot (length n), and the greedy walk loses it."""
    w = np.zeros((n, n), np.int32)
    for i in range(n):
        w[i, i] = 1000
        if i + 1 < n:
            w[i, i + 1] = 1001
    return w


@functools.lru_cache(maxsize=None)
def solver_cases():
    """name -> (weights (P, T, D) int32, t_counts or None, d_counts or None) as numpy arrays."""
    rng = np.random.default_rng(2024)
    one = lambda w: np.ascontiguousarray(np.asarray(w, np.int32)[None])
    c = {}
    c["1x1_allowed"] = (one([[5]]), None, None)
    c["1x1_forbidden"] = (one([[0]]), None, None)
    c["2x3"] = (one([[7, 9, 0], [8, 9, 3]]), None, None)
    c["3x2"] = (one([[7, 8], [9, 9], [0, 3]]), None, None)
    c["all_forbidden"] = (np.zeros((2, 5, 7), np.int32), None, None)
    c["identity"] = (one(np.eye(9, dtype=np.int32) * 100), None, None)
    c["constant"] = (np.stack([np.full((12, 12), 77, np.int32), np.full((12, 12), M, np.int32)]), None, None)
    c["two_weights"] = (one(rng.choice([3, 5], (20, 17))), None, None)
    c["band_64"] = (one(band(64)), None, None)
    for n in (63, 64, 65):
        c[f"cols_{n}"] = (one(rng.integers(0, 50, (40, n))), None, None)
    c["dense_70"] = (one(rng.integers(1, M + 1, (70, 70))), None, None)
    c["ties_128"] = (one(rng.choice([0, 10, 20, 30], (128, 128), p=[0.1, 0.3, 0.3, 0.3])), None, None)
    c["sparse_256x300"] = (np.stack([sparse(256, 300, s) for s in (1, 2)]), None, None)
    c["sparse_1024"] = (one(sparse(1024, 1024, 3)), None, None)
    w = rng.integers(-5 * M, 5 * M, (5, 40, 50)).astype(np.int32)            # garbage everywhere ...
    tcnt = np.array([17, 0, 40, 45, -3], np.int32)                           # ... 45: above T, -3: below 0
    dcnt = np.array([50, 23, 9, 70, 12], np.int32)
    for p in range(5):
        nt, nd = min(max(tcnt[p], 0), 40), min(max(dcnt[p], 0), 50)
        w[p, :nt, :nd] = rng.integers(0, 200, (nt, nd)) * (rng.random((nt, nd)) < 0.5)
    c["counts"] = (w, tcnt, dcnt)
    w = rng.integers(-3, 4, (1, 30, 30)).astype(np.int32) * (M // 2)          # -1.5 M .. 1.5 M: the clamp
    w[0, 0, 0], w[0, 1, 1] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    c["clamp"] = (w, None, None)
    return c


def run_lib(case, device="cpu", threads=1):
    """yolo_hip.assign on a solver case with poisoned reused outputs -> numpy (row_of_slot, slot_of_row)."""
    import yolo_hip
    w, tcnt, dcnt = case
    P, T, D = w.shape
    mv = lambda a: None if a is None else torch.from_numpy(a).to(device)
    out = (torch.full((P, T), -7, dtype=torch.int32, device=device),
           torch.full((P, D), -7, dtype=torch.int32, device=device))
    got = yolo_hip.assign(mv(w), mv(tcnt), mv(dcnt), out=out, threads=threads)
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the tracker

def weight(val):
    """w = 1 + (int)(val * 65535.0f), clamped to [1, M]; val f32 array (finite where it matters)."""
    s = val.astype(F) * F(65535.0)
    assert s.dtype == F
    return np.clip(1 + np.trunc(s).astype(np.int64), 1, M)


def _optimal(slots, rows, cand, val, mrow, mslot):
    """The OPTIMAL association: `solve` over the live slots and rows in ascending order."""
    ts, ds = np.nonzero(slots)[0], np.nonzero(rows)[0]
    if len(ts) == 0 or len(ds) == 0:
        return
    sub = np.ix_(ts, ds)
    W = np.where(cand[sub], weight(np.where(cand[sub], val[sub], F(0))), 0)
    ros, _ = solve(W)
    for a, c in enumerate(ros):
        if c >= 0:
            mrow[ts[a]], mslot[ds[c]] = ds[c], ts[a]


def _iou(box, det):
    tx1, ty1, tx2, ty2 = (v[:, None] for v in box)
    dx1, dy1, dx2, dy2 = (det[None, :, i] for i in range(4))
    w = np.maximum(tc.ZERO, np.minimum(tx2, dx2) - np.maximum(tx1, dx1))
    h = np.maximum(tc.ZERO, np.minimum(ty2, dy2) - np.maximum(ty1, dy1))
    inter = w * h
    union = ((tx2 - tx1) * (ty2 - ty1) + (dx2 - dx1) * (dy2 - dy1)) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(inter != 0, inter / union, tc.ZERO).astype(F)
    return inter, iou


class RefAssignStream(tc.RefStream):
    assign = "greedy"             # the mode of the next step

    def _assoc(self, slots, rows, thr, det, box, mrow, mslot):
        if self.assign != "optimal":
            return super()._assoc(slots, rows, thr, det, box, mrow, mslot)
        inter, iou = _iou(box, det)
        cand = slots[:, None] & rows[None, :] & (inter != 0) & (iou >= thr)
        if self.p["class_aware"]:
            cand &= self.cls[:, None] == det[None, :, 5]
        _optimal(slots, rows, cand, iou, mrow, mslot)


class RefAssignReidStream(rc.RefReidStream):
    assign = "greedy"

    def _assoc(self, slots, rows, thr, det, box, mrow, mslot):
        if self.assign != "optimal":
            return super()._assoc(slots, rows, thr, det, box, mrow, mslot)
        self._calls += 1
        self._mrow, self._mslot = mrow, mslot
        inter, iou = _iou(box, det)
        cand = (inter != 0) & (iou >= thr)
        val = iou
        if self._calls == 1:
            dot = self.gallery.astype(np.int32) @ self._q.astype(np.int32).T
            cosv = dot.astype(F) / F(16129.0)
            app = F(0.5) + F(0.5) * cosv
            both = self.gallery.any(axis=1)[:, None] & self._q.any(axis=1)[None, :]
            eligible = both & (cosv >= self.cos_min) & (iou >= self.iou_min)
            cand = cand | eligible
            val = np.where(eligible, np.maximum(iou, app), iou).astype(F)
        cand = cand & slots[:, None] & rows[None, :]
        if self.p["class_aware"]:
            cand &= self.cls[:, None] == det[None, :, 5]
        _optimal(slots, rows, cand, val, mrow, mslot)


def _modes(assign, n):
    return [assign] * n if isinstance(assign, str) else list(assign)


def ref_state(refs, gallery=False):
    """The streams as the library's state tensor would hold them: (S, words) int32."""
    rows = []
    for r in refs:
        hdr = np.array([r.f, r.next_id - 1, 0, 0], np.int32)
        f32 = lambda a: np.ascontiguousarray(a.T).view(np.int32).reshape(-1)
        parts = [hdr, r.status, r.id, r.last, r.cls.view(np.int32), f32(r.x), f32(r.v), f32(r.a), f32(r.b), f32(r.c)]
        if gallery:
            parts.append(r.gallery.reshape(-1).view(np.int32))
        rows.append(np.concatenate(parts))
    return np.stack(rows)


def run_ref(frames, max_tracks, assign="optimal", dim=None, max_out=None, cos_min=0.5, iou_min=0.5, **params):
    """The restatement over a sequence (a reid sequence when dim is given); assign: a mode, or one
    per frame -> per frame (out, ids, det_index, counts, state words)."""
    B, md = frames[0][0].shape[:2]
    max_out = md if max_out is None else max_out
    if dim is None:
        refs = [RefAssignStream(max_tracks, **params) for _ in range(B)]
    else:
        refs = [RefAssignReidStream(max_tracks, dim, cos_min, iou_min, **params) for _ in range(B)]
    res = []
    for fr, mode in zip(frames, _modes(assign, len(frames))):
        dets, counts = fr[0], fr[1]
        feats = rc.row_features(fr, md, dim) if dim is not None else [()] * B
        out = np.zeros((B, max_out, 6), F)
        ids, idx = np.zeros((B, max_out), np.int32), np.zeros((B, max_out), np.int32)
        cnt = np.zeros(B, np.int32)
        for b in range(B):
            refs[b].assign = mode
            k = min(max(int(counts[b]), 0), md)
            out[b], ids[b], idx[b], cnt[b] = refs[b].step(dets[b, :k].numpy(), max_out, *feats[b])
        res.append((out, ids, idx, cnt, ref_state(refs, dim is not None)))
    return res


def run_track(frames, max_tracks, assign="optimal", dim=None, device="cpu", max_out=None, threads=1, state=None,
              cos_min=0.5, iou_min=0.5, handover=None, **params):
    """yolo_hip.track (track_reid when dim is given) over a sequence with poisoned reused outputs;
    assign: a mode, one per frame, or None (the call without the argument). handover: the frame
    before which the state goes to the host and back -> (per frame numpy (out, ids, det_index,
    counts, state words), the final state)."""
    from yolo_hip import track as yt
    B, md = frames[0][0].shape[:2]
    max_out = md if max_out is None else max_out
    p = yt.params(**dict(tc.DEFAULTS, **params))
    if state is None:
        state = yt.track_state(B, max_tracks, device, reid_dim=dim)
    ws = None if dim is None else yt.reid_workspace(B, md, max_tracks, dim, device)
    modes = [None] * len(frames) if assign is None else _modes(assign, len(frames))
    res = []
    mv = lambda t: None if t is None else t.to(device)
    for i, (fr, mode) in enumerate(zip(frames, modes)):
        if handover is not None and i == handover:
            state = state.cpu().clone().to(device)
        out = (torch.full((B, max_out, 6), -7.0, device=device),
               torch.full((B, max_out), -7, dtype=torch.int32, device=device),
               torch.full((B, max_out), -7, dtype=torch.int32, device=device),
               torch.full((B,), -7, dtype=torch.int32, device=device))
        kw = {} if mode is None else {"assign": mode}
        if dim is None:
            yt.track(mv(fr[0]), mv(fr[1]), state, p, max_out=max_out, out=out, threads=threads, **kw)
        else:
            ws.fill_(0x5A)
            yt.track_reid(mv(fr[0]), mv(fr[1]), state, embed=mv(fr[2]), feat_counts=mv(fr[3]), embed_total=mv(fr[4]),
                          dim=dim, reid_cos=cos_min, reid_iou=iou_min, p=p, max_out=max_out, out=out, workspace=ws,
                          threads=threads, **kw)
        res.append(tuple(t.cpu().numpy() for t in out) + (state.cpu().numpy().copy(),))
    return res, state


def same(got, want, what=""):
    """Bit-for-bit equality of two per-frame result lists, state words included."""
    tc.same(got, want, what)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[4].tobytes() == w[4].tobytes(), f"{what} frame {i}: state"


def two_person():
    """DESIGN.md section 18's scene: two people side by side step right so that the detection of the first lies
    nearer to the second's track. Frame 1 starts both tracks, frame 2 is the contested one, then
    two quiet frames."""
    a = [(0, 100), (35, 135), (45, 145), (55, 155)]
    b = [(60, 160), (110, 210), (120, 220), (130, 230)]
    return tc.single([[[xa[0], 0, xa[1], 200, 0.9, 0.0], [xb[0], 0, xb[1], 200, 0.8, 0.0]] for xa, xb in zip(a, b)])


def duplicates():
    """Exact duplicate boxes: every weight ties and the tie rules decide."""
    rows = [tc.box(100, 100, 50, 80, 0.9), tc.box(100, 100, 50, 80, 0.8), tc.box(100, 100, 50, 80, 0.7),
            tc.box(112, 100, 50, 80, 0.6)]
    moved = [tc.box(104, 100, 50, 80, 0.9), tc.box(104, 100, 50, 80, 0.85), tc.box(108, 100, 50, 80, 0.5),
             tc.box(108, 100, 50, 80, 0.2), tc.box(108, 100, 50, 80, 0.15)]
    return tc.single([rows, moved, rows[:3], moved])


def separated(frames=6):
    """Objects far apart, one class each way: no slot or row ever has two candidates."""
    rng = np.random.default_rng(11)
    seq = []
    for f in range(frames):
        per = []
        for s in range(2):
            rows = []
            for o in range(9):
                if rng.random() < 0.15:
                    continue
                score = 0.9 if rng.random() < 0.8 else 0.2
                rows.append(tc.box(100 + 200 * (o % 3) + 3 * f, 100 + 200 * (o // 3) + 2 * f, 60, 80, score, float(o % 2)))
            per.append([rows[i] for i in rng.permutation(len(rows))])
        seq.append(tc.pack(per, 16))
    return seq


@functools.lru_cache(maxsize=None)
def tracker_cases():
    """name -> (frames, max_tracks, params) for the plain tracker."""
    return {
        "two_person": (two_person(), 8, {}),
        "duplicates": (duplicates(), 8, {}),
        "crowd": (tc.sequence(5, streams=2, frames=8, max_det=70, objects=40, classes=1), 64, {}),
        "crowd_classes": (tc.sequence(6, streams=2, frames=8, max_det=70, objects=30, classes=2), 48, {}),
        "crowd_class_blind": (tc.sequence(6, streams=2, frames=8, max_det=70, objects=30, classes=2), 48,
                              {"class_aware": False}),
        "crowd_full_table": (tc.sequence(7, streams=2, frames=8, max_det=70, objects=30, classes=1), 20, {"max_age": 2}),
    }


REID_DIM = 64


@functools.lru_cache(maxsize=None)
def reid_case():
    """A reid sequence whose objects cross (they move on straight lines through one small field)."""
    return rc.reid_sequence(3, dim=REID_DIM, streams=2, frames=8, max_det=70, objects=24), 48
