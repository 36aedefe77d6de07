"""The appearance side of the tracker restated in numpy, and the cases its tests share.

`quantize` and `similarity` are yh_embed_quantize / yh_embed_similarity as include/yolo_hip.h
states them (np.float64 operations, one rounding each; integer sums). `RefReidStream` is
`_track_cases.RefStream` with yh_track_reid's first association and gallery update; everything
else of a frame is RefStream's own code. They are the yardstick of tests/test_reid_host.py (the
host twins equal them byte for byte) and, through the host twins, of tests/test_gpu_reid.py.

A reid sequence is a list of frames (dets, counts, embed (capacity, dim) f32, feat_counts (S,)
i32, embed_total (1,) i32 or None); rows of dets at or beyond a count are NaN, and so are the
rows of embed no feature maps to.
"""
import functools

import numpy as np
import torch

import _track_cases as tc

F = np.float32
D64 = np.float64


def quantize(e, count=None):
    """(rows, dim) f32 -> (rows, dim) int8 by the four steps of yh_embed_quantize."""
    e = np.ascontiguousarray(e, dtype=F)
    rows, dim = e.shape
    q = np.zeros((rows, dim), np.int8)
    n = rows if count is None else min(max(int(count), 0), rows)
    for r in range(n):
        row = e[r]
        if not np.isfinite(row).all():
            continue
        m = np.abs(row).max()
        if m == 0:
            continue
        scale = D64(16384.0) / D64(m)
        p = np.rint(row.astype(D64) * scale).astype(np.int64)
        S = int((p * p).sum())
        k = D64(127.0) / np.sqrt(D64(S))
        q[r] = np.rint(p.astype(D64) * k).astype(np.int8)
    return q


def similarity(a_blocks, b, a_index=None):
    """a_blocks (nblocks, ra, dim) int8, b (B, rb, dim) int8 -> (B, ra, rb) int32, exact."""
    nblocks, ra = a_blocks.shape[:2]
    B, rb = b.shape[:2]
    out = np.zeros((B, ra, rb), np.int32)
    for i in range(B):
        k = i if a_index is None else int(a_index[i])
        if 0 <= k < nblocks:
            out[i] = a_blocks[k].astype(np.int32) @ b[i].astype(np.int32).T
    return out


def ema(g, q):
    """The gallery update of a slot that had a feature: g, q (dim,) int8 -> int8."""
    t = 7 * g.astype(np.int64) + q.astype(np.int64)
    S = int((t * t).sum())
    if S == 0:
        return np.zeros_like(g)
    k = D64(127.0) / np.sqrt(D64(S))
    return np.rint(t.astype(D64) * k).astype(np.int8)


def quantize_cases(dim):
    """(rows, dim) f32 with every special row the header names, and random ones."""
    rng = np.random.default_rng(dim)
    e = rng.normal(0, 1, (24, dim)).astype(F)
    e[1] = 0                                         # zeros: no feature
    e[2] = 0; e[2, 5] = -3.5                         # a single non-zero
    e[3, 7] = np.inf
    e[4, 0] = np.nan
    e[5, dim - 1] = -np.inf
    e[6] *= F(1e-42)                                 # subnormal magnitudes
    e[7] = 0; e[7, 3] = F(1.4e-45)                   # the smallest subnormal alone
    e[8] *= F(1e37); e[8, 1] = F(3e38)
    e[9] = F(3e38)                                   # every element at the top
    e[10] = 1                                        # equal elements: 127 / sqrt(dim) each
    e[11] = np.where(np.arange(dim) % 2, -0.0, 0.0)  # signed zeros only
    e[12] = rng.integers(-3, 4, dim)                 # small integers: many rint ties
    return e


def similarity_case(ra, rb, dim, seed=0):
    """Three batch rows over five strided blocks, permuted, one index out of range; full-range int8
    with rows of -128 (the largest products)."""
    rng = np.random.default_rng(seed + 7 * ra + 13 * rb + dim)
    big = torch.from_numpy(rng.integers(-128, 128, (5, ra + 3, dim), dtype=np.int8))
    big[1, 0] = -128
    a = big[:, :ra]                                                    # blocks (ra + 3) * dim bytes apart
    b = torch.from_numpy(rng.integers(-128, 128, (3, rb, dim), dtype=np.int8))
    b[0, rb - 1] = -128
    index = torch.tensor([4, 7, 1], dtype=torch.int32)                 # 7: no such block
    return a, b, index


class RefReidStream(tc.RefStream):
    def __init__(self, max_tracks, dim, cos_min=0.5, iou_min=0.5, **params):
        super().__init__(max_tracks, **params)
        self.dim = dim
        self.cos_min, self.iou_min = F(cos_min), F(iou_min)
        self.gallery = np.zeros((max_tracks, dim), np.int8)

    def _assoc(self, slots, rows, thr, det, box, mrow, mslot):
        self._calls += 1
        self._mrow, self._mslot = mrow, mslot          # the arrays RefStream.step goes on filling
        if self._calls != 1:
            return super()._assoc(slots, rows, thr, det, box, mrow, mslot)
        tx1, ty1, tx2, ty2 = (v[:, None] for v in box)
        dx1, dy1, dx2, dy2 = (det[None, :, i] for i in range(4))
        w = np.maximum(tc.ZERO, np.minimum(tx2, dx2) - np.maximum(tx1, dx1))
        h = np.maximum(tc.ZERO, np.minimum(ty2, dy2) - np.maximum(ty1, dy1))
        inter = w * h
        union = ((tx2 - tx1) * (ty2 - ty1) + (dx2 - dx1) * (dy2 - dy1)) - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.where(inter != 0, inter / union, tc.ZERO).astype(F)
        dot = self.gallery.astype(np.int32) @ self._q.astype(np.int32).T
        cosv = dot.astype(F) / F(16129.0)
        app = F(0.5) + F(0.5) * cosv
        assert cosv.dtype == F and app.dtype == F
        both = self.gallery.any(axis=1)[:, None] & self._q.any(axis=1)[None, :]
        eligible = both & (cosv >= self.cos_min) & (iou >= self.iou_min)
        cand = slots[:, None] & rows[None, :] & (((inter != 0) & (iou >= thr)) | eligible)
        if self.p["class_aware"]:
            cand &= self.cls[:, None] == det[None, :, 5]
        val = np.where(eligible, np.maximum(iou, app), iou)
        ts, ds = np.nonzero(cand)
        for i in np.lexsort((ds, ts, -val[ts, ds])):
            t, d = ts[i], ds[i]
            if mrow[t] < 0 and mslot[d] < 0:
                mrow[t], mslot[d] = d, t

    def step(self, det, max_out, q=None, has=None):
        """q (n, dim) int8 and has (n,) bool: the rows' quantised features (None: no row has one)."""
        det = np.ascontiguousarray(det, dtype=F)
        n = det.shape[0]
        self._q = np.zeros((n, self.dim), np.int8) if q is None else q
        has = np.zeros(n, bool) if has is None else has
        self._calls = 0
        first_new = self.next_id
        res = super().step(det, max_out)
        p = self.p
        score = det[:, 4]
        births = [d for d in range(n)
                  if score[d] >= p["track_high"] and self._mslot[d] < 0 and score[d] >= p["track_new"]]
        for t in range(self.T):
            if self.status[t] != 0 and self.id[t] >= first_new:       # born in this frame
                d = births[self.id[t] - first_new]
                self.gallery[t] = self._q[d] if has[d] else 0
            elif self._mrow[t] >= 0:
                d = self._mrow[t]
                if has[d]:
                    self.gallery[t] = ema(self.gallery[t], self._q[d]) if self.gallery[t].any() else self._q[d]
        return res


def row_features(frame, max_det, dim):
    """yh_crop_rois' compaction: per batch row (q (c_b, dim) int8, has (c_b,) bool) of a reid frame."""
    dets, counts, embed, feat_counts, total = frame
    B = dets.shape[0]
    limit = 0 if embed is None else embed.shape[0]
    if embed is not None and total is not None:
        limit = min(limit, int(total[0]))
    base, res = 0, []
    for b in range(B):
        c = min(max(int(counts[b]), 0), max_det)
        nf = c if feat_counts is None else min(max(int(feat_counts[b]), 0), c)
        q, has = np.zeros((c, dim), np.int8), np.zeros(c, bool)
        for r in range(nf):
            if base + r < limit:
                has[r] = True
                q[r] = quantize(embed[base + r:base + r + 1].numpy())[0]
        base += nf
        res.append((q, has))
    return res


def run_ref(frames, max_tracks, dim, max_out=None, streams=None, stream_ids=None, cos_min=0.5, iou_min=0.5, **params):
    """The restatement over a reid sequence -> (per frame (out, ids, det_index, counts), the streams)."""
    B, md = frames[0][0].shape[:2]
    streams = B if streams is None else streams
    max_out = md if max_out is None else max_out
    refs = [RefReidStream(max_tracks, dim, cos_min, iou_min, **params) for _ in range(streams)]
    res = []
    for i, fr in enumerate(frames):
        dets, counts = fr[0], fr[1]
        nb = dets.shape[0]
        sid = list(range(nb)) if stream_ids is None or stream_ids[i] is None else stream_ids[i]
        feats = row_features(fr, md, dim)
        out = np.zeros((nb, max_out, 6), F)
        ids, idx = np.zeros((nb, max_out), np.int32), np.zeros((nb, max_out), np.int32)
        cnt = np.zeros(nb, np.int32)
        for b, s in enumerate(sid):
            if not 0 <= s < streams:
                continue
            k = min(max(int(counts[b]), 0), md)
            out[b], ids[b], idx[b], cnt[b] = refs[s].step(dets[b, :k].numpy(), max_out, *feats[b])
        res.append((out, ids, idx, cnt))
    return res, refs


def ref_state(refs, max_tracks, dim):
    """The streams of run_ref as the library's state tensor would hold them: (S, words) int32."""
    rows = []
    for r in refs:
        hdr = np.array([r.f, r.next_id - 1, 0, 0], np.int32)
        f32 = lambda a: np.ascontiguousarray(a.T).view(np.int32).reshape(-1)   # (T, 4) -> field major
        words = np.concatenate([hdr, r.status, r.id, r.last, r.cls.view(np.int32), f32(r.x), f32(r.v), f32(r.a),
                                f32(r.b), f32(r.c), r.gallery.reshape(-1).view(np.int32)])
        rows.append(words)
    return np.stack(rows)


def run_lib(frames, max_tracks, dim, device="cpu", max_out=None, streams=None, stream_ids=None, threads=1, state=None,
            cos_min=0.5, iou_min=0.5, **params):
    """yolo_hip.track_reid over a reid sequence with poisoned, reused outputs and workspace ->
    (per frame numpy (out, ids, det_index, counts), the final state tensor)."""
    from yolo_hip import track as yt
    B, md = frames[0][0].shape[:2]
    streams = B if streams is None else streams
    max_out = md if max_out is None else max_out
    p = yt.params(**dict(tc.DEFAULTS, **params))
    if state is None:
        state = yt.track_state(streams, max_tracks, device, reid_dim=dim)
    ws = yt.reid_workspace(max(f[0].shape[0] for f in frames), md, max_tracks, dim, device)
    res = []
    for i, (dets, counts, embed, feat_counts, total) in enumerate(frames):
        nb = dets.shape[0]
        ws.fill_(0x5A)
        out = (torch.full((nb, max_out, 6), -7.0, device=device),
               torch.full((nb, max_out), -7, dtype=torch.int32, device=device),
               torch.full((nb, max_out), -7, dtype=torch.int32, device=device),
               torch.full((nb,), -7, dtype=torch.int32, device=device))
        sid = None
        if stream_ids is not None and stream_ids[i] is not None:
            sid = torch.tensor(stream_ids[i], dtype=torch.int32, device=device)
        mv = lambda t: None if t is None else t.to(device)
        got = yt.track_reid(dets.to(device), counts.to(device), state, embed=mv(embed), feat_counts=mv(feat_counts),
                            embed_total=mv(total), dim=dim, reid_cos=cos_min, reid_iou=iou_min, p=p, stream_ids=sid,
                            max_out=max_out, out=out, workspace=ws, threads=threads)
        assert all(g is o for g, o in zip(got, out))
        res.append(tuple(t.cpu().numpy() for t in out))
    return res, state


def base_words(state, max_tracks):
    """The yh_track part of a reid state (S, words) -> numpy (S, 4 + 24 * max_tracks) int32."""
    return state.cpu().numpy()[:, :4 + 24 * max_tracks]


@functools.lru_cache(maxsize=None)
def prototypes(dim, n=16, seed=99):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (n, dim)).astype(F)


@functools.lru_cache(maxsize=None)
def reid_sequence(seed, dim=64, streams=3, frames=12, max_det=70, objects=24):
    """`_track_cases.sequence(seed)` with features: a row's embedding is the prototype of its class
    and width bucket - the same for an object from frame to frame most of the time, shared with
    other objects often enough that appearance and IoU disagree - without noise for half the rows
    (equal products: the tie rules decide) and with noise for the others; a few rows carry zeros,
    an infinity or a NaN ("no feature"). Most frames embed every row; some only the leading
    feat_counts rows, and some cut the features off in the middle of a batch row with a short
    embed_total."""
    base = tc.sequence(seed, streams=streams, frames=frames, max_det=max_det, objects=objects)
    rng = np.random.default_rng(1000 + seed)
    protos = prototypes(dim)
    seq = []
    for i, (dets, counts) in enumerate(base):
        c = counts.clamp(0, max_det)
        mode = i % 4
        if mode == 2:
            fc = torch.tensor([int(rng.integers(0, int(v) + 1)) for v in c], dtype=torch.int32)
        elif mode == 3:
            fc = torch.tensor([int(v) + 5 for v in c], dtype=torch.int32)      # above the count: clamped
        else:
            fc = None
        nf = c if fc is None else torch.minimum(fc.clamp(min=0), c)
        rows = []
        for b in range(dets.shape[0]):
            for r in range(int(nf[b])):
                d = dets[b, r].numpy()
                e = protos[(int(d[5]) * 7 + int((d[2] - d[0]) / 10)) % len(protos)].copy()
                if rng.random() < 0.5:
                    e += rng.normal(0, 0.4, dim).astype(F)
                u = rng.random()
                if u < 0.04:
                    e[:] = 0
                elif u < 0.07:
                    e[int(rng.integers(dim))] = np.inf
                elif u < 0.1:
                    e[int(rng.integers(dim))] = np.nan
                rows.append(e)
        n = len(rows)
        embed = torch.full((n + 3, dim), float("nan"))
        if n:
            embed[:n] = torch.from_numpy(np.stack(rows))
        total = None
        if mode == 1:
            total = torch.tensor([max(n - int(nf[-1]) // 2 - 1, 0)], dtype=torch.int32)   # inside the last row
        if i == 4:
            embed = embed[:max(n - int(nf[-1]) - 2, 0)].contiguous()                     # capacity inside another
        seq.append((dets, counts, embed, fc, total))
    return tuple(seq)


def with_features(frames, embeds, dim):
    """A `_track_cases` sequence plus per frame a list (per stream) of (n_b, dim) arrays, one feature
    per row -> a reid sequence."""
    seq = []
    for (dets, counts), per in zip(frames, embeds):
        rows = [np.asarray(e, F).reshape(-1, dim) for e in per]
        assert [len(r) for r in rows] == counts.tolist()
        flat = np.concatenate(rows) if rows else np.zeros((0, dim), F)
        seq.append((dets, counts, torch.from_numpy(np.ascontiguousarray(flat)), None, None))
    return seq


def same(got, want, what=""):
    tc.same(got, want, what)
