"""Inputs and reference shared by the yh_fuse / yh_fuse_host tests (CPU and GPU).

`wbf_ref` is weighted boxes fusion as include/yolo_hip.h states it (steps 1-5), a plain float64 numpy
loop that shares nothing with the library. Coordinates lie on an integer grid, scores are k/256 and
weights have a few bits, so every s = score * weight is exact in fp32. While it runs, `wbf_ref`
asserts what the comparison of an fp32 implementation with an fp64 one needs of the inputs: no IoU
within 1e-4 of the threshold, a joined cluster's IoU ahead of the runner-up by 1e-4, and two cluster
scores that meet in the output order either 1e-6 apart (relative) or equal with equal n and S.

Cases are built once per process and never modified. Rows at or beyond a group's count, and the
padding groups beyond the offsets, are NaN: they must never be read.
"""
import functools

import numpy as np
import torch

from yolo_hip import _lib

CAP = _lib.FUSE_MAX_CAND
ONE = (1, 1, 0, 0, 0, 0)


def wbf_ref(c):
    """-> per image the clusters [(class, n, x1, y1, x2, y2, score), ...] in output order, float64."""
    dets, counts, xf = c["dets"].numpy().astype(np.float64), c["counts"].numpy(), c["group_xf"].numpy().astype(np.float64)
    wt, off, wh = c["group_weight"].numpy().astype(np.float64), c["group_offsets"].numpy(), c["image_wh"].numpy()
    thr, result = c["iou"], []
    for i in range(len(off) - 1):
        W, H = float(wh[i, 0]), float(wh[i, 1])
        groups = range(int(off[i]), min(int(off[i + 1]), int(off[i]) + c["max_groups"]))
        wtot, cand = sum(wt[g] for g in groups), []
        for g in groups:
            sx, sy, px, py, ox, oy = xf[g]
            for r in range(min(max(int(counts[g]), 0), dets.shape[1])):
                x1, y1, x2, y2, score, cls = dets[g, r]
                xs = sorted(((x1 - px) * sx + ox, (x2 - px) * sx + ox))
                ys = sorted(((y1 - py) * sy + oy, (y2 - py) * sy + oy))
                box = np.array([min(max(xs[0], 0), W), min(max(ys[0], 0), H), min(max(xs[1], 0), W), min(max(ys[1], 0), H)])
                s = score * wt[g]
                assert float(np.float32(s)) == s
                if box[2] > box[0] and box[3] > box[1] and s >= c["skip_score"]:
                    cand.append((cls, -s, len(cand), box))
        clusters = []                                   # [class, creation index, n, S, weighted sums (4)]
        for cls in sorted({k[0] for k in cand}):
            mine = []
            for _, ns, _, b in sorted((k for k in cand if k[0] == cls), key=lambda k: k[:3]):
                s = -ns
                if mine:
                    f = np.array([m[4] / m[3] for m in mine])
                    iw = np.clip(np.minimum(f[:, 2], b[2]) - np.maximum(f[:, 0], b[0]), 0, None)
                    ih = np.clip(np.minimum(f[:, 3], b[3]) - np.maximum(f[:, 1], b[1]), 0, None)
                    area = (f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1]) + (b[2] - b[0]) * (b[3] - b[1])
                    iou = iw * ih / (area - iw * ih)
                    assert (np.abs(iou - thr) >= 1e-4).all(), "an IoU within 1e-4 of the threshold"
                    k = int(np.argmax(iou))             # the first of equal maxima: the lowest k
                if mine and iou[k] > thr:
                    assert (np.delete(iou, k) < iou[k] - 1e-4).all(), "two clusters within 1e-4 of the best IoU"
                    mine[k][2] += 1
                    mine[k][3] += s
                    mine[k][4] = mine[k][4] + s * b
                else:
                    mine.append([cls, len(mine), 1, s, s * b])
            clusters += mine
        rows = sorted(((-(m[3] / m[2]) * min(m[2], wtot) / wtot, m[0], m[1], m) for m in clusters), key=lambda t: t[:3])
        for p, q in zip(rows, rows[1:]):
            assert q[0] - p[0] > 1e-6 * -p[0] or (q[0] == p[0] and q[3][2:4] == p[3][2:4]), "two scores too close to order"
        result.append([(m[0], m[2], *(m[4] / m[3]), -ns) for ns, _, _, m in rows[:c["max_out"]]])
    return result


def pack(images, max_det, iou=0.55, skip_score=0.0, max_out=300, pad_groups=0):
    """images: [(W, H, [(xf, weight, source-space rows (k, 6)), ...]), ...] -> a case of CPU tensors.
    The rows are taken to each group's canvas through the inverse of xf (exact on the grid)."""
    gl = [g for _, _, gs in images for g in gs]
    G = len(gl) + pad_groups
    dets = np.full((G, max_det, 6), np.nan, np.float32)
    counts, xf, wt = np.zeros(G, np.int32), np.full((G, 6), np.nan, np.float32), np.full(G, np.nan, np.float32)
    counts[len(gl):] = max_det
    for g, (f, w, rows) in enumerate(gl):
        rows = np.asarray(rows, np.float64).reshape(-1, 6)
        sx, sy, px, py, ox, oy = f
        cx = np.sort(np.stack(((rows[:, 0] - ox) / sx + px, (rows[:, 2] - ox) / sx + px), 1), 1)
        cy = np.sort(np.stack(((rows[:, 1] - oy) / sy + py, (rows[:, 3] - oy) / sy + py), 1), 1)
        dets[g, :len(rows)] = np.stack((cx[:, 0], cy[:, 0], cx[:, 1], cy[:, 1], rows[:, 4], rows[:, 5]), 1)
        counts[g], xf[g], wt[g] = len(rows), f, w
    off = np.cumsum([0] + [len(gs) for _, _, gs in images]).astype(np.int32)
    c = dict(dets=torch.from_numpy(dets), counts=torch.from_numpy(counts), group_xf=torch.from_numpy(xf),
             group_weight=torch.from_numpy(wt), group_offsets=torch.from_numpy(off),
             image_wh=torch.tensor([[W, H] for W, H, _ in images], dtype=torch.float32).reshape(-1, 2),
             max_groups=max([len(gs) for _, _, gs in images] + [1]), iou=iou, skip_score=skip_score, max_out=max_out)
    assert c["max_groups"] * max_det <= CAP
    c["want"] = wbf_ref(c)
    return c


def scene(seed, full, single, P, classes):
    """One image: `full` objects that each of the P groups sees (a copy moved by up to 2 px, the same
    score k/256) and `single` objects that one group sees, every object in a 100 px cell of its own,
    so that objects never overlap. Single objects take a k that is no multiple of P: their score
    s / P then meets no full object's. Rows are shuffled within a group."""
    rng = np.random.default_rng(seed)
    n = full + single
    side = int(np.ceil(np.sqrt(n)))
    groups = [[] for _ in range(P)]
    for o in range(n):
        x0, y0 = 100 * (o % side) + 8, 100 * (o // side) + 8
        w, h, k = rng.integers(30, 80, 2).tolist() + [int(rng.integers(40, 250))]
        if o >= full and k % P == 0:
            k += 1
        for g in (range(P) if o < full else [o % P]):
            dx, dy, dw, dh = rng.integers(-2, 3, 4)
            groups[g].append([x0 + dx, y0 + dy, x0 + w + dx + dw, y0 + h + dy + dh, k / 256, o % classes])
    gs = [(ONE, 1.0, [rows[j] for j in rng.permutation(len(rows))]) for g, rows in enumerate(groups)]
    return (100 * side, 100 * side, gs)


def _scene(full, single, P, classes, **kw):
    return lambda: pack([scene(full + single, full, single, P, classes)], full + single, **kw)


def _mixed():
    """A mirrored and a half-scale group whose boxes coincide with the plain group's; weights 2, 1, 0.5
    (Wtot 3.5); an object one group alone found (n = 1 < Wtot); a candidate that overlaps two
    clusters (the nearer one takes it); equal scores at equal boxes (ties go to the lower position);
    rows below skip_score; boxes across and beyond the border. Then an image with no groups, one
    whose groups are empty, one with a single candidate; NaN padding groups at the end."""
    W, H = 640, 480
    plain, mirror, half = ONE, (-1, 1, W, 0, 0, 0), (2, 2, 16, 8, 0, 0)
    a = [100, 100, 200, 180, 192 / 256, 0]
    rows0 = [a, [300, 100, 400, 200, 128 / 256, 0], [340, 100, 440, 200, 100 / 256, 0], [10, 300, 90, 400, 64 / 256, 1],
             [10, 300, 90, 400, 64 / 256, 1], [-20, 420, 60, 500, 200 / 256, 2], [700, 10, 760, 50, 250 / 256, 2]]
    rows1 = [[102, 100, 202, 182, 160 / 256, 0], [306, 100, 406, 200, 90 / 256, 0], [500, 300, 560, 380, 8 / 256, 1]]
    rows2 = [[98, 102, 198, 178, 224 / 256, 0], [10, 300, 90, 400, 128 / 256, 1], [500, 40, 580, 120, 32 / 256, 3]]
    first = (W, H, [(plain, 2.0, rows0), (mirror, 1.0, rows1), (half, 0.5, rows2)])
    empty = (320, 240, [(plain, 1.0, []), (mirror, 3.0, [])])
    one = (320, 240, [(plain, 0.75, [[5, 5, 50, 60, 96 / 256, 7]])])
    return pack([first, (800, 600, []), empty, one], 8, skip_score=10 / 256, pad_groups=2)


def _max_out():
    return pack([scene(3, 20, 9, 3, 4), scene(4, 2, 1, 3, 2)], 29, max_out=12)


CASES = {
    "mixed": _mixed,
    "max_out": _max_out,
    "clusters_64": _scene(64, 0, 2, 1),          # one class whose clusters fill the 64 lanes exactly
    "clusters_65": _scene(60, 5, 2, 1),          # ... and wrap to lane 0
    "clusters_200": _scene(150, 50, 3, 1),       # several clusters per lane
    "classes_16": _scene(48, 7, 3, 16),          # one segment per wave
    "classes_17": _scene(48, 7, 3, 17),          # ... and a second one for wave 0
    "total_1023": _scene(341, 0, 3, 5),
    "total_1024": _scene(341, 1, 3, 5),
    "total_1025": _scene(341, 2, 3, 5),
    "cap": _scene(CAP // 4, 0, 4, 16),           # YH_FUSE_MAX_CAND candidates, every row valid
}
ALL = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict of CPU tensors dets, counts, group_xf, group_weight, group_offsets, image_wh; max_groups,
    iou, skip_score, max_out; want = wbf_ref's clusters."""
    return CASES[name]()
