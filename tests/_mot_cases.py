"""yh_mot_eval's rules (include/yolo_hip.h) restated in numpy, and the cases the tracking-evaluation
tests share. `ref_eval` is the yardstick of tests/test_mot_host.py (the host twin equals it byte for
byte) and, through the host twin, of tests/test_gpu_mot.py. The assignment, the IoU and the weight
are tests/_assign_cases.py's restatements: there is no second solver here.
"""
import functools

import numpy as np
import torch

import _assign_cases as ac

F32 = np.float32


def _weights(G, T, class_aware):
    """(ng, 5), (nh, 6) f32 -> iou (ng, nh) f32 (0 where the boxes are disjoint), class test, weight"""
    _, iou = ac._iou(tuple(G[:, i] for i in range(4)), T)
    same = (G[:, None, 4] == T[None, :, 5]) if class_aware else np.ones(iou.shape, bool)
    return iou, same, ac.weight(iou)


def _eval_one(tr, ti, tc, gt, gi, gc, nf, thr, n_gt_ids, n_tr_ids, class_aware):
    mo, mg = tr.shape[1], gt.shape[1]
    out = np.zeros((len(thr), 8), np.int64)
    ign = np.zeros(2, np.int32)
    last = [dict() for _ in thr]        # gt id -> last matched track id
    prev = [dict() for _ in thr]        # gt id -> track id matched in the previous live frame
    C = np.zeros((len(thr), n_gt_ids, n_tr_ids), np.int64)
    for f in range(nf):
        ng, nh = min(max(int(gc[f]), 0), mg), min(max(int(tc[f]), 0), mo)
        G, T, gid, tid = gt[f, :ng], tr[f, :nh], gi[f, :ng], ti[f, :nh]
        gok, tok = (gid >= 0) & (gid < n_gt_ids), (tid >= 0) & (tid < n_tr_ids)
        ign += (int((~gok).sum()), int((~tok).sum()))
        iou, same, w = _weights(G, T, class_aware)
        row_of = {int(t): c for c, t in enumerate(tid) if tok[c]}
        for a, th in enumerate(thr):
            W = np.where(same & (iou >= th) & gok[:, None] & tok[None, :], w, 0)
            rs, cs = np.nonzero(W)
            np.add.at(C[a], (gid[rs], tid[cs]), 1)
            mate = {}
            for r in np.nonzero(gok)[0]:                       # the carry
                c = row_of.get(prev[a].get(int(gid[r]), -1), -1)
                if c >= 0 and W[r, c] > 0:
                    mate[int(r)] = c
            rows = [r for r in np.nonzero(gok)[0] if r not in mate]
            cols = [c for c in np.nonzero(tok)[0] if c not in mate.values()]
            if rows and cols:                                  # the assignment of the rest
                ros, _ = ac.solve(W[np.ix_(rows, cols)])
                mate.update({int(rows[s]): int(cols[c]) for s, c in enumerate(ros) if c >= 0})
            prev[a] = {}
            for r, c in mate.items():
                g, t = int(gid[r]), int(tid[c])
                out[a, 3] += g in last[a] and last[a][g] != t
                out[a, 4] += W[r, c] - 1
                last[a][g] = prev[a][g] = t
            out[a, 0] += len(mate)
            out[a, 6] += gok.sum()
            out[a, 7] += tok.sum()
    for a in range(len(thr)):
        if n_gt_ids and n_tr_ids:
            ros, _ = ac.solve(np.minimum(C[a], ac.M))
            out[a, 5] = sum(C[a, g, t] for g, t in enumerate(ros) if t >= 0)
        out[a, 1], out[a, 2] = out[a, 7] - out[a, 0], out[a, 6] - out[a, 0]
    return out, ign


def ref_eval(c):
    """A case -> (out (S, num_thr, 8) int64, ignored (S, 2) int32) by the rules."""
    S, F = c["tr_counts"].shape
    res = [_eval_one(c["tr"][s], c["tr_ids"][s], c["tr_counts"][s], c["gt"][s], c["gt_ids"][s], c["gt_counts"][s],
                     F if c["frames"] is None else min(max(int(c["frames"][s]), 0), F), c["thr"], c["n_gt_ids"],
                     c["n_tr_ids"], c["class_aware"]) for s in range(S)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def pack(gt_rows, tr_rows, max_gt, max_out, thr, n_gt_ids, n_tr_ids, class_aware=1, frames=None, counts=None):
    """gt_rows[s][f] = rows of (x1, y1, x2, y2, class, id), tr_rows[s][f] = rows of (x1, y1, x2, y2, score,
    class, id) -> a case; what lies beyond a count is NaN boxes and ids that would index far away.
    counts: {(side, s, f): value} overrides a count (the clamp)."""
    S, F = len(gt_rows), len(gt_rows[0])
    c = {"gt": np.full((S, F, max_gt, 5), np.nan, F32), "gt_ids": np.full((S, F, max_gt), 1 << 28, np.int32),
         "gt_counts": np.zeros((S, F), np.int32), "tr": np.full((S, F, max_out, 6), np.nan, F32),
         "tr_ids": np.full((S, F, max_out), -(1 << 28), np.int32), "tr_counts": np.zeros((S, F), np.int32)}
    for side, rows, k in (("gt", gt_rows, 5), ("tr", tr_rows, 6)):
        for s in range(S):
            for f in range(F):
                r = np.asarray(rows[s][f], np.float64).reshape(-1, k + 1)
                c[side][s, f, :len(r)] = r[:, :k]
                c[side + "_ids"][s, f, :len(r)] = r[:, k]
                c[side + "_counts"][s, f] = len(r)
    for (side, s, f), v in (counts or {}).items():
        c[side + "_counts"][s, f] = v
    c.update(thr=np.asarray(thr, F32), n_gt_ids=n_gt_ids, n_tr_ids=n_tr_ids, class_aware=class_aware,
             frames=None if frames is None else np.asarray(frames, np.int32))
    return c


def scene(seed, g_rows, h_rows, max_gt, max_out, thr, n_gt_ids, n_tr_ids, **kw):
    """Objects on a grid whose neighbours overlap, drifting; g_rows[s][f] / h_rows[s][f] of them (a
    random choice, in random order) are the frame's ground truth / hypotheses, the latter jittered,
    a tenth with the wrong class, two tracks trading ids half way; ids reach n_*_ids - 1 and a few
    lie outside the range."""
    rng = np.random.default_rng(seed)
    S, F = len(g_rows), len(g_rows[0])
    gt_rows, tr_rows = [], []
    for s in range(S):
        O = max(1, max(max(g_rows[s]), max(h_rows[s])))
        # distinct ids, the largest one first; without identities every row is out of range
        ids = lambda n: np.concatenate([[n - 1], rng.permutation(n - 1)])[:O] if n else np.zeros(O, np.int64)
        gid, tid = ids(n_gt_ids), ids(n_tr_ids)
        gs, ts = [], []
        for f in range(F):
            if f == F // 2 and O > 3:
                tid[[2, 3]] = tid[[3, 2]]
            x = 40.0 * (np.arange(O) % 16) + 3 * f
            y = 60.0 * (np.arange(O) // 16) + 2 * f
            cls = (np.arange(O) % 2).astype(np.float64)
            wild = lambda n, ids, hi: np.where(rng.random(n) < 0.04, rng.choice([-1, hi, 1 << 30], n), ids)
            pool = min(O, max(g_rows[s][f], h_rows[s][f]) + 8)     # mostly the same objects on both sides
            og = rng.permutation(pool)[:g_rows[s][f]]
            gs.append(np.stack([x[og], y[og], x[og] + 50, y[og] + 50, cls[og], wild(len(og), gid[og], n_gt_ids)], 1))
            oh = rng.permutation(pool)[:h_rows[s][f]]
            j = rng.uniform(-6, 6, (len(oh), 4))
            hc = np.where(rng.random(len(oh)) < 0.1, 1 - cls[oh], cls[oh])
            ts.append(np.stack([x[oh] + j[:, 0], y[oh] + j[:, 1], x[oh] + 50 + j[:, 2], y[oh] + 50 + j[:, 3],
                                rng.random(len(oh)), hc, wild(len(oh), tid[oh], n_tr_ids)], 1))
        gt_rows.append(gs)
        tr_rows.append(ts)
    return pack(gt_rows, tr_rows, max_gt, max_out, thr, n_gt_ids, n_tr_ids, **kw)


def carry_case():
    """Frame 0 matches ground truth A to track 1. In frame 1 track 2 lies nearer to A and track 1
    nearer to B, all four pairs above 0.4: the carry keeps (A, 1) and leaves (B, 2), the plain
    assignment would take (A, 2) and (B, 1). At 0.5 the carried pair is not allowed any more."""
    gt = [[[(0, 0, 100, 100, 0.0, 0)], [(0, 0, 100, 100, 0.0, 0), (40, 0, 140, 100, 0.0, 1)]]]
    tr = [[[(0, 0, 100, 100, 0.9, 0.0, 1)], [(38, 0, 138, 100, 0.9, 0.0, 1), (5, 0, 105, 100, 0.9, 0.0, 2)]]]
    return pack(gt, tr, 2, 2, [0.4, 0.5], 2, 3)


def swap_case(F=10, k=6):
    """Two objects, tracked perfectly, whose tracks trade ids at frame k."""
    gt = [[[(0, 0, 50, 50, 0.0, 0), (200, 0, 250, 50, 0.0, 1)] for _ in range(F)]]
    tr = [[[(0, 0, 50, 50, 0.9, 0.0, 1 if f < k else 2), (200, 0, 250, 50, 0.9, 0.0, 2 if f < k else 1)]
           for f in range(F)]]
    return pack(gt, tr, 2, 2, [0.5], 2, 3)


THR16 = np.linspace(0.05, 0.95, 16)


@functools.lru_cache(maxsize=None)
def cases():
    mixed_g = [[64, 0, 256, 65, 63, 1, 64], [1, 63, 65, 0, 64, 256, 256]]
    mixed_h = [[65, 1, 256, 0, 64, 63, 63], [0, 64, 63, 1, 256, 65, 256]]
    small_g, small_h = [[5, 0, 3, 5, 1, 4, 5], [2, 5, 5, 0, 5, 3, 1]], [[3, 3, 0, 2, 3, 3, 1], [3, 0, 3, 3, 2, 1, 3]]
    return {
        "f1_thr1": scene(1, [[1], [64], [0]], [[1], [65], [3]], 64, 65, [0.5], 70, 80),
        "f1_thr16": scene(2, [[63], [1]], [[64], [0]], 64, 64, THR16, 64, 64, class_aware=0),
        # every row count on both sides, a count above the cap and one below 0, a short sequence
        "mixed_thr16": scene(3, mixed_g, mixed_h, 256, 256, THR16, 300, 320, frames=[7, 5],
                             counts={("gt", 0, 2): 300, ("tr", 1, 3): -4}),
        "mixed_thr1_blind": scene(4, mixed_g, mixed_h, 256, 256, [0.3], 256, 257, class_aware=0, frames=[9, 0]),
        # frame strides that no 16-byte load fits
        "odd_strides": scene(5, small_g, small_h, 5, 3, [0.1, 0.5, 0.75], 6, 7),
        "no_ids": scene(6, small_g, small_h, 5, 3, [0.5], 0, 0),
        "carry": carry_case(),
        "swap": swap_case(),
    }


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref_eval of a case, computed once and shared"""
    return ref_eval(cases()[name])


def run_lib(c, device="cpu", threads=1):
    """yolo_hip.mot_eval on a case with poisoned reused outputs and workspace -> numpy (out, ignored)"""
    import yolo_hip
    S = c["tr_counts"].shape[0]
    mv = lambda a: None if a is None else torch.from_numpy(a).to(device)
    out = (torch.full((S, len(c["thr"]), 8), -7, dtype=torch.int64, device=device),
           torch.full((S, 2), -7, dtype=torch.int32, device=device))
    ws = None
    if torch.device(device).type == "cuda":
        ws = yolo_hip.mot_workspace(S, len(c["thr"]), c["n_gt_ids"], c["n_tr_ids"], device).fill_(0x5A)
    got = yolo_hip.mot_eval(mv(c["tr"]), mv(c["tr_ids"]), mv(c["tr_counts"]), mv(c["gt"]), mv(c["gt_ids"]),
                            mv(c["gt_counts"]), mv(c["thr"]), c["n_gt_ids"], c["n_tr_ids"], frames=mv(c["frames"]),
                            class_aware=c["class_aware"], out=out, workspace=ws, threads=threads)
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()
