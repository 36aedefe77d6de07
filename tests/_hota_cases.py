"""The yardstick and the cases of the HOTA tests. `ref_eval` is TrackEval's HOTA (Luiten et al. 2021)
in float64 numpy with scipy's assignment: the similarity is the fp32 IoU of include/yolo_hip.h's rule
1 widened to float64, everything after it - Jaccard terms, alignment, scores, ratios - is float64. It
shares no integer rule with yh_hota_eval; tests/test_hota_host.py holds the host twin to it, and
tests/test_gpu_hota.py the kernels to the host twin byte for byte.

The scene recipe: objects as 40 px squares, positions uniform in a square arena, velocities uniform in
[-6, 6)^2 px per frame; per frame a random subset is ground truth and another one the hypotheses, the
latter with N(0, 3) px noise on every coordinate; hypothesis ids go through a permutation that is rolled
by one every 13th frame. The arena is 200 px a side for up to 8 objects and grows with the square root
of their number, which keeps the number of neighbours a box overlaps at what it is for 8.
"""
import functools

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

F32 = np.float32
THR19 = (np.arange(1, 20).astype(F32) * F32(0.05)).astype(F32)


def _iou32(G, T):
    """(ng, 5), (nh, 6) f32 -> (ng, nh) fp32 IoU, one rounding per operation, 0 where disjoint"""
    g, t = G[:, None, :], T[None, :, :]
    w = np.maximum(np.minimum(g[..., 2], t[..., 2]) - np.maximum(g[..., 0], t[..., 0]), F32(0))
    h = np.maximum(np.minimum(g[..., 3], t[..., 3]) - np.maximum(g[..., 1], t[..., 1]), F32(0))
    inter = (w * h).astype(F32)
    ag = ((g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])).astype(F32)
    at = ((t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = (inter / ((ag + at).astype(F32) - inter).astype(F32)).astype(F32)
    return np.where(inter == 0, F32(0), iou)


def _ref_one(tr, ti, tc, gt, gi, gc, nf, thr, n_gt_ids, n_tr_ids, class_aware):
    """One sequence -> dict of (num_thr,) arrays (counts as int64, ratios as float64), rows, ignored"""
    frames, rows, ign = [], np.zeros(2, np.int64), np.zeros(2, np.int32)
    P, cg, ct = np.zeros((n_gt_ids, n_tr_ids)), np.zeros(n_gt_ids), np.zeros(n_tr_ids)
    for f in range(nf):
        ng, nh = min(max(int(gc[f]), 0), gt.shape[1]), min(max(int(tc[f]), 0), tr.shape[1])
        gok, tok = (gi[f, :ng] >= 0) & (gi[f, :ng] < n_gt_ids), (ti[f, :nh] >= 0) & (ti[f, :nh] < n_tr_ids)
        ign += (int((~gok).sum()), int((~tok).sum()))
        G, T, g, t = gt[f, :ng][gok], tr[f, :nh][tok], gi[f, :ng][gok], ti[f, :nh][tok]
        iou = _iou32(G, T)
        sim = iou.astype(np.float64)
        if class_aware:
            sim = np.where(G[:, None, 4] == T[None, :, 5], sim, 0.0)
        denom = sim.sum(1, keepdims=True) + sim.sum(0, keepdims=True) - sim
        np.add.at(P, (g[:, None], t[None, :]), np.divide(sim, denom, out=np.zeros_like(sim), where=sim > 0))
        cg[g] += 1
        ct[t] += 1
        rows += (len(g), len(t))
        frames.append((g, t, sim, iou))
    A = P / np.maximum(cg[:, None] + ct[None, :] - P, 1.0)
    M = np.zeros((len(thr), n_gt_ids, n_tr_ids))
    tp, loc = np.zeros(len(thr), np.int64), np.zeros(len(thr))
    for g, t, sim, iou in frames:
        r, c = linear_sum_assignment(-(A[g[:, None], t[None, :]] * sim))
        keep = sim[r, c] > 0
        r, c = r[keep], c[keep]
        for a, th in enumerate(thr):
            ok = iou[r, c] >= th
            tp[a] += ok.sum()
            loc[a] += sim[r[ok], c[ok]].sum()
            np.add.at(M[a], (g[r[ok]], t[c[ok]]), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"tp": tp, "fn": rows[0] - tp, "fp": rows[1] - tp, "pairs": (M > 0).sum((1, 2)),
               "assa": (M * M / np.maximum(cg[:, None] + ct[None, :] - M, 1.0)).sum((1, 2)) / tp,
               "assre": (M * M / np.maximum(cg[:, None], 1.0)).sum((1, 2)) / tp,
               "asspr": (M * M / np.maximum(ct[None, :], 1.0)).sum((1, 2)) / tp, "loca": loc / tp}
        res["deta"] = tp / (tp + res["fn"] + res["fp"])
        res["hota_alpha"] = np.sqrt(res["deta"] * res["assa"])
    return res, rows, ign


def ref_eval(c):
    """A case -> (list of per-sequence dicts, rows (S, 2), ignored (S, 2)) by the float64 formulas."""
    S, F = c["tr_counts"].shape
    res = [_ref_one(c["tr"][s], c["tr_ids"][s], c["tr_counts"][s], c["gt"][s], c["gt_ids"][s], c["gt_counts"][s],
                    F if c["frames"] is None else min(max(int(c["frames"][s]), 0), F), c["thr"], c["n_gt_ids"],
                    c["n_tr_ids"], c["class_aware"]) for s in range(S)]
    return [r[0] for r in res], np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def scene(seed, F, rows, ids, max_gt, max_out, thr=THR19, class_aware=1, frames=None, n_gt_ids=None, n_tr_ids=None,
          wild=0.0, flip=0.0, side=None):
    """rows[s] = (ground-truth rows, hypothesis rows) of every frame of sequence s, out of `ids` objects.
    wild: the share of ids replaced by one out of range; flip: the share of hypotheses of the other class;
    side: the arena (None: the one that keeps 8 objects' density). What lies beyond a count is NaN boxes
    and ids that would index far away."""
    rng = np.random.default_rng(seed)
    S, side = len(rows), 200.0 * np.sqrt(max(ids, 8) / 8.0) if side is None else side
    n_gt_ids, n_tr_ids = ids if n_gt_ids is None else n_gt_ids, ids if n_tr_ids is None else n_tr_ids
    c = {"gt": np.full((S, F, max_gt, 5), np.nan, F32), "gt_ids": np.full((S, F, max_gt), 1 << 28, np.int32),
         "gt_counts": np.zeros((S, F), np.int32), "tr": np.full((S, F, max_out, 6), np.nan, F32),
         "tr_ids": np.full((S, F, max_out), -(1 << 28), np.int32), "tr_counts": np.zeros((S, F), np.int32)}
    for s, (ng, nh) in enumerate(rows):
        pos, vel, perm = rng.uniform(0, side, (ids, 2)), rng.uniform(-6, 6, (ids, 2)), rng.permutation(ids)
        cls = (np.arange(ids) % 2).astype(np.float64)
        for f in range(F):
            if f and f % 13 == 0:
                perm = np.roll(perm, 1)
            xy = pos + vel * f
            og, oh = rng.permutation(ids)[:ng], rng.permutation(ids)[:nh]
            strays = lambda n, ident, hi: np.where(rng.random(n) < wild, rng.choice([-1, hi, 1 << 30], n), ident)
            c["gt"][s, f, :ng] = np.concatenate([xy[og], xy[og] + 40.0, cls[og, None]], 1)
            c["gt_ids"][s, f, :ng] = strays(ng, og, n_gt_ids)
            box = np.concatenate([xy[oh], xy[oh] + 40.0], 1) + rng.normal(0, 3, (nh, 4))
            hc = np.where(rng.random(nh) < flip, 1 - cls[oh], cls[oh])
            c["tr"][s, f, :nh] = np.concatenate([box, rng.random((nh, 1)), hc[:, None]], 1)
            c["tr_ids"][s, f, :nh] = strays(nh, perm[oh], n_tr_ids)
            c["gt_counts"][s, f], c["tr_counts"][s, f] = ng, nh
    c.update(thr=np.asarray(thr, F32), n_gt_ids=n_gt_ids, n_tr_ids=n_tr_ids, class_aware=class_aware,
             frames=None if frames is None else np.asarray(frames, np.int32))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return {
        # the recipe as it was checked: three sequences of different live lengths, the 19 thresholds
        "recipe": scene(0, 40, [(6, 6)] * 3, 8, 6, 6, frames=[40, 27, 1]),
        "one_row": scene(1, 30, [(1, 1)], 2, 1, 1),
        "empty_sides": scene(2, 20, [(0, 3), (3, 0), (0, 0)], 4, 3, 3, thr=[0.5]),
        # 63, 64 and 65 rows across the solver's lane stride; unequal row caps that no 16-byte load fits
        "lane_stride": scene(3, 12, [(63, 65), (64, 64), (65, 63)], 70, 65, 67, frames=[12, 7, 3], flip=0.1),
        # one wave per workgroup: the whole tile in one frame; thresholds out of order, classes ignored
        "full_tile": scene(4, 1, [(256, 256)], 256, 256, 256, thr=[0.75, 0.25, 0.5, 0.95, 0.05], class_aware=0, flip=0.5),
        # ids out of range on both sides, identities the scene never uses, equal thresholds
        "wild_ids": scene(5, 40, [(6, 5), (4, 6)], 8, 7, 6, thr=[0.5, 0.3, 0.5, 0.9], n_gt_ids=9, n_tr_ids=11, wild=0.05,
                          flip=0.1),
        # buffers without a row on either side: zeros everywhere, and no launch may need a byte of LDS
        "no_rows": scene(6, 3, [(0, 0), (0, 0)], 4, 0, 0, thr=[0.5, 0.25]),
    }


@functools.lru_cache(maxsize=None)
def dense_cases():
    """The fixed 200 px arena at row counts where every box overlaps dozens of others: long augmenting
    paths in the solver. Near-ties between matchings are then common, so these cases are held to the
    host twin only (tests/test_gpu_hota.py), not to the float64 reference."""
    return {
        "dense_tile": scene(7, 2, [(256, 256)], 256, 256, 256, thr=[0.75, 0.25, 0.5, 0.95, 0.05], flip=0.1, side=200.0),
        "dense_stride": scene(8, 6, [(63, 65), (65, 64)], 70, 65, 67, frames=[6, 4], class_aware=0, side=200.0),
    }


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref_eval of a case, computed once and shared"""
    return ref_eval(cases()[name])


def run_lib(c, device="cpu", threads=1):
    """yolo_hip.hota_eval on a case with poisoned reused outputs and workspace -> numpy (out, rows, ignored)"""
    import yolo_hip
    S, nt = c["tr_counts"].shape[0], len(c["thr"])
    mv = lambda a: None if a is None else torch.from_numpy(a).to(device)
    out = (torch.full((S, nt, 8), -7, dtype=torch.int64, device=device), torch.full((S, 2), -7, dtype=torch.int64, device=device),
           torch.full((S, 2), -7, dtype=torch.int32, device=device))
    ws = None
    if torch.device(device).type == "cuda":
        ws = yolo_hip.hota_workspace(S, nt, c["n_gt_ids"], c["n_tr_ids"], device).fill_(0x5A)
    got = yolo_hip.hota_eval(mv(c["tr"]), mv(c["tr_ids"]), mv(c["tr_counts"]), mv(c["gt"]), mv(c["gt_ids"]),
                             mv(c["gt_counts"]), c["n_gt_ids"], c["n_tr_ids"], thr=mv(c["thr"]), frames=mv(c["frames"]),
                             class_aware=c["class_aware"], out=out, workspace=ws, threads=threads)
    assert all(g is o for g, o in zip(got, out))
    return tuple(o.cpu().numpy() for o in out)
