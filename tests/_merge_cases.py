"""Inputs and restatement shared by the yh_merge / yh_merge_host tests (CPU and GPU).

`restate` is the numpy statement of include/yolo_hip.h's merge semantics: the map in np.float32
operations in the stated order, the clip, the drop of empty boxes, and for images of two or more
tiles the greedy step through oracle.nms.torchvision_nms - once per class on that class's
candidates in global sorted order, the kept sets merged by global order and cut at max_out
(classes are independent, so this equals the one-pass rule).

Cases are built once per process and never modified. Rows at or beyond a tile's (clamped)
count are NaN in every case: they must never be read.
"""
import functools

import numpy as np
import torch

from oracle.nms import torchvision_nms
from yolo_hip import _lib
from yolo_hip.detect import tile_transform, tiles

CAP = _lib.MERGE_MAX_CAND


# ----------------------------------------------------------------------------- restatement
def map_rows(rows, xf, W, H):
    """(k, 6) f32 canvas rows of one tile -> (mapped (k, 6) f32, keep (k,) bool)."""
    sx, sy, px, py, ox, oy = (np.float32(v) for v in xf)
    W, H, zero = np.float32(W), np.float32(H), np.float32(0)
    out = rows.astype(np.float32).copy()
    for col, (s, p, o, hi) in enumerate(((sx, px, ox, W), (sy, py, oy, H), (sx, px, ox, W), (sy, py, oy, H))):
        t = rows[:, col] - p
        t = t * s
        t = t + o
        assert t.dtype == np.float32
        out[:, col] = np.minimum(np.maximum(t, zero), hi)
    keep = ~((out[:, 2] <= out[:, 0]) | (out[:, 3] <= out[:, 1]))
    return out, keep


def restate(c):
    """-> (out (N, max_out, 6) f32, out_counts (N,) i32) of a case, in numpy."""
    dets, counts, xf = c["dets"].numpy(), c["counts"].numpy(), c["tile_xf"].numpy()
    off, wh = c["tile_offsets"].numpy(), c["image_wh"].numpy()
    T, md = dets.shape[:2]
    N, max_out = len(off) - 1, c["max_out"]
    out = np.zeros((N, max_out, 6), np.float32)
    out_counts = np.zeros((N,), np.int32)
    for i in range(N):
        lo = min(max(int(off[i]), 0), T)
        hi = min(max(int(off[i + 1]), lo), T)
        hi = min(hi, lo + c["max_tiles"])
        cand = []
        for t in range(lo, hi):
            cnt = min(max(int(counts[t]), 0), md)
            m, keep = map_rows(dets[t, :cnt], xf[t], wh[i, 0], wh[i, 1])
            cand.append(m[keep])
        cand = np.concatenate(cand, 0) if cand else np.zeros((0, 6), np.float32)
        if hi - lo >= 2 and len(cand):
            cand = cand[np.argsort(-cand[:, 4].astype(np.float64), kind="stable")]
            kept = []
            for k in np.unique(cand[:, 5]):
                idx = np.nonzero(cand[:, 5] == k)[0]
                kept.append(idx[torchvision_nms(cand[idx, :4], cand[idx, 4], np.float64(c["iou"]))])
            cand = cand[np.sort(np.concatenate(kept))]
        cand = cand[:max_out]
        out[i, :len(cand)] = cand
        out_counts[i] = len(cand)
    return out, out_counts


# ----------------------------------------------------------------------------- builders
def to_canvas(box, xf):
    """Source-space boxes (k, 4) float64 -> canvas coordinates of a tile, in float64 (the forward
    letterbox transform: (X - ox) / sx + px)."""
    sx, sy, px, py, ox, oy = (float(v) for v in xf)
    b = np.asarray(box, np.float64)
    return np.stack(((b[:, 0] - ox) / sx + px, (b[:, 1] - oy) / sy + py,
                     (b[:, 2] - ox) / sx + px, (b[:, 3] - oy) / sy + py), 1)


def pack(images, max_det, iou=0.65, max_out=300, max_tiles=None, pad_tiles=0, raw_counts=None):
    """images: [(W, H, [(xf, rows (k, 6)), ...]), ...] -> a case of CPU tensors. Rows keep their
    order; everything beyond a tile's rows is NaN. pad_tiles: unreferenced tiles at the end,
    count max_det, all NaN. raw_counts: {tile: count} overrides (clamping tests)."""
    tl = [t for _, _, ts in images for t in ts]
    T = len(tl) + pad_tiles
    dets = np.full((T, max_det, 6), np.nan, np.float32)
    counts = np.zeros((T,), np.int32)
    xf = np.zeros((T, 6), np.float32)
    for t, (f, rows) in enumerate(tl):
        rows = np.asarray(rows, np.float32).reshape(-1, 6)
        assert len(rows) <= max_det
        dets[t, :len(rows)] = rows
        counts[t] = len(rows)
        xf[t] = f
    counts[len(tl):] = max_det
    xf[len(tl):] = np.nan
    for t, v in (raw_counts or {}).items():
        counts[t] = v
        dets[t, min(max(v, 0), max_det):] = np.nan
    off = np.cumsum([0] + [len(ts) for _, _, ts in images]).astype(np.int32)
    wh = np.asarray([[W, H] for W, H, _ in images], np.float32).reshape(-1, 2)
    if max_tiles is None:
        max_tiles = max([len(ts) for _, _, ts in images] + [1])
    c = dict(dets=torch.from_numpy(dets), counts=torch.from_numpy(counts), tile_xf=torch.from_numpy(xf),
             tile_offsets=torch.from_numpy(off), image_wh=torch.from_numpy(wh), max_tiles=int(max_tiles),
             iou=float(iou), max_out=int(max_out))
    assert c["max_tiles"] * max_det <= CAP
    c["want"] = restate(c)
    return c


def _objects(rng, n, W, H, classes, lo=12, hi=90):
    xy = rng.uniform(0, [W - lo, H - lo], size=(n, 2))
    wh = rng.uniform(lo, hi, size=(n, 2))
    box = np.concatenate([xy, np.minimum(xy + wh, [W, H])], 1)
    return box, rng.integers(0, classes, size=n).astype(np.float64)


def random_image(rng, per_tile, W=900, H=700, classes=3, dup=0.6, equal_scores=False, scales=(1.0, 1.0, 1.5625, 1.3),
                 lo=12, hi=90, outside=0.0):
    """One image whose tiles hold per_tile[t] rows each: jittered copies of a pool of objects
    (dup: share of rows that repeat an object some other row has), seen through tiles with
    arbitrary transforms. Rows at the image border are clipped; a share `outside` of the rows
    lies wholly beyond the right or the bottom edge and is dropped by the map."""
    total = int(sum(per_tile))
    nobj = max(1, int(round(total * (1 - dup))))
    obox, ocls = _objects(rng, nobj, W, H, classes, lo, hi)
    ts = []
    for k in per_tile:
        s = rng.choice(scales)
        f = (np.float32(s), np.float32(s), np.float32(rng.integers(0, 40)), np.float32(rng.integers(0, 40)),
             np.float32(rng.integers(0, 200)), np.float32(rng.integers(0, 200)))
        pick = rng.integers(0, nobj, size=k)
        box = obox[pick] + rng.normal(0, 0.75, size=(k, 4))
        out = rng.uniform(size=k) < outside
        box[out] += np.where(rng.uniform(size=(int(out.sum()), 1)) < 0.5, [[W, 0, W, 0]], [[0, H, 0, H]])
        score = np.full(k, 0.5) if equal_scores else np.sort(rng.uniform(0.001, 1, size=k))[::-1]
        rows = np.concatenate([to_canvas(box, f), score[:, None], ocls[pick][:, None]], 1)
        ts.append((f, rows))
    return (W, H, ts)


def projected_image(rng, H, W, tile, size, overlap, boxes, full_image=False):
    """A geometrically consistent image: source boxes (k, 6) projected into every tile of
    tiles(H, W, tile, overlap) that sees at least 60 % of the box, with sub-pixel jitter, each
    tile's rows by score descending as an NMS writes them."""
    ts = []
    for crop in tiles(H, W, tile, overlap, full_image):
        x0, y0, w, h = crop
        f = tile_transform(crop, size)
        rows = []
        for b in boxes:
            ix = max(0.0, min(b[2], x0 + w) - max(b[0], x0)) * max(0.0, min(b[3], y0 + h) - max(b[1], y0))
            if ix >= 0.6 * (b[2] - b[0]) * (b[3] - b[1]):
                vis = np.array([[max(b[0], x0), max(b[1], y0), min(b[2], x0 + w), min(b[3], y0 + h)]])
                vis = vis + rng.uniform(-0.3, 0.3, size=(1, 4))
                rows.append(np.concatenate([to_canvas(vis, f)[0], [b[4] - rng.uniform(0, 0.01), b[5]]]))
        rows = np.asarray(sorted(rows, key=lambda r: -r[4]), np.float64).reshape(-1, 6)
        ts.append((f, rows))
    return (W, H, ts)


def _split(total, parts):
    base = [total // parts] * parts
    for i in range(total % parts):
        base[i] += 1
    return base


# ----------------------------------------------------------------------------- the case list
def _single():
    """Single-tile images: a 480 x 640 source on a 320 canvas (scale 2, top border 40), a 320 x 320
    source (scale exactly 1) and a 200 x 300 one (upscaled). Rows inside, across the image border
    (clipped), wholly in the border padding (dropped), degenerate after the clip, unsorted scores."""
    rng = np.random.default_rng(5)
    images = []
    for (H, W) in ((480, 640), (320, 320), (200, 300)):
        f = tile_transform((0, 0, W, H), 320)
        left, top = float(f[2]), float(f[3])
        rows = [[left + 10.25, top + 20.5, left + 100.75, top + 90.0, 0.9, 1],        # inside
                [-5.0, top - 12.0, left + 50.0, top + 40.0, 0.8, 0],                  # crosses top-left: clipped
                [left + 200.0, top + 100.0, 330.0, 325.0, 0.95, 2],                   # crosses bottom-right
                [left + 5.0, top - 30.0, left + 60.0, top - 2.0, 0.7, 0],             # wholly above the image
                [left + 70.0, top + 30.0, left + 70.0, top + 80.0, 0.6, 1]]           # zero width
        box, cls = _objects(rng, 20, W, H, 3)
        more = np.concatenate([to_canvas(box, f), rng.uniform(0.01, 1, size=(20, 1)), cls[:, None]], 1)
        images.append((W, H, [(f, np.concatenate([np.asarray(rows, np.float64), more], 0))]))
    return pack(images, 32)


def _overlap_once():
    """416 x 544 image tiled 320 / 0.25: an object wholly inside the overlap of two tiles, one in
    the overlap of all four, one seen by a single tile."""
    rng = np.random.default_rng(6)
    boxes = [[250, 30, 300, 80, 0.9, 0],       # x overlap of the top two tiles (x 224..320)
             [240, 110, 310, 300, 0.8, 1],     # all four (y 96..320)
             [10, 10, 60, 70, 0.7, 2]]         # top-left only
    return pack([projected_image(rng, 416, 544, 320, 320, 0.25, boxes)], 8, iou=0.5)


def _chain():
    """A kills B, B would have killed C, C survives (IoU(A, B) = IoU(B, C) = 0.54, IoU(A, C) = 0.25)."""
    one = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    a = [0, 0, 100, 50, 0.9, 0]
    b = [30, 0, 130, 50, 0.8, 0]
    cc = [60, 0, 160, 50, 0.7, 0]
    return pack([(400, 100, [(one, [a, cc]), (one, [b])])], 4, iou=0.5)


def _classes():
    """Equal boxes of different classes: neither is killed; equal class: the later one is."""
    one = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    r = [[10, 10, 60, 60, 0.9, 0], [10, 10, 60, 60, 0.8, 1]]
    return pack([(100, 100, [(one, r), (one, [[10, 10, 60, 60, 0.7, 1], [10, 10, 60, 60, 0.6, 2]])])], 4)


def _total(total, tiles_, md, **kw):
    def make():
        rng = np.random.default_rng(total)
        return pack([random_image(rng, _split(total, tiles_), **kw)], md)
    return make


def _ties():
    rng = np.random.default_rng(8)
    return pack([random_image(rng, [40, 40, 37], equal_scores=True, dup=0.8, classes=2, outside=0.1),
                 random_image(rng, [64, 64], equal_scores=True, dup=0.5, classes=1)], 64)


def _mixed():
    """A tile with count 0 between two full ones (with rows the map drops among them); an image with no tiles; a single-tile image whose
    count exceeds max_det (clamped); a negative count; unreferenced padding tiles at the end."""
    rng = np.random.default_rng(9)
    md = 48
    a = random_image(rng, [md, 0, md], outside=0.15)
    none = (640, 480, [])
    one = random_image(rng, [md])
    neg = random_image(rng, [md, 20], outside=0.15)
    return pack([a, none, one, neg], md, pad_tiles=3, raw_counts={3: md + 5, 4: -2})


def _max_out():
    rng = np.random.default_rng(10)
    return pack([random_image(rng, [60, 60, 60], dup=0.3, outside=0.1), random_image(rng, [60], outside=0.1)], 60, max_out=7)


def _cap():
    """Exactly MERGE_MAX_CAND candidates, every row valid: 16 tiles x MERGE_MAX_CAND / 16 rows."""
    rng = np.random.default_rng(11)
    md = CAP // 16
    return pack([random_image(rng, [md] * 16, W=3840, H=2160, classes=4, dup=0.5, lo=20, hi=200)], md)


def _deep_walk():
    """The walk crosses several blocks of 1024 sorted candidates with a few hundred rows kept: heavy
    duplication, max_out above the number of survivors, two images of different depth."""
    rng = np.random.default_rng(13)
    return pack([random_image(rng, [300] * 14, W=2000, H=1500, classes=2, dup=0.9, outside=0.02),
                 random_image(rng, [300] * 7 + [0] * 7, W=2000, H=1500, classes=1, dup=0.8)], 300, max_out=2500)


def _bound():
    """max_tiles below an image's tile count: the range is cut to max_tiles tiles."""
    rng = np.random.default_rng(12)
    return pack([random_image(rng, [30, 30, 30]), random_image(rng, [30, 30])], 30, max_tiles=2)


CASES = {
    "single": _single,
    "overlap_once": _overlap_once,
    "chain": _chain,
    "classes": _classes,
    "ties": _ties,
    "total_255": _total(255, 3, 128),
    "total_256": _total(256, 4, 64),
    "total_257": _total(257, 5, 64),
    "total_1024": _total(1024, 4, 256),
    "total_1025": _total(1025, 5, 256),
    "mixed": _mixed,
    "max_out": _max_out,
    "bound": _bound,
    "deep_walk": _deep_walk,
    "cap": _cap,
}
ALL = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: dets (T, md, 6), counts (T,), tile_xf (T, 6), tile_offsets (N + 1,), image_wh (N, 2)
    CPU tensors; max_tiles, iou, max_out; want = restate's (out, out_counts) numpy arrays."""
    return CASES[name]()
