"""numpy restatement of yh_crop_rois' semantics (include/yolo_hip.h) and the cases that
test_crop_host.py / test_gpu_crop.py share. The resize is the unchanged
oracle.preprocess.resize_linear, the letterbox and the NV12 conversion are _video_cases'; only the
rectangle rule (np.float32, step by step), the compaction and the composition are stated here.
TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import _video_cases as vc
from oracle import preprocess as opre

F32 = np.float32
NAN, INF = float("nan"), float("inf")

# frame kinds of a case, cycled over the batch: (format, height, width, matrix, row padding)
KINDS = (("bgr", 50, 70, 0, 5), ("bgr", 17, 23, 0, 1), ("nv12", 36, 64, 601, 0), ("nv12", 90, 40, 709, 3),
         ("bgr", 96, 128, 0, 0))
SWEEP_KIND = 4   # the 96 x 128 BGR frame


def rect(box, pad, H, W):
    """(x0, y0, w, h) of the padded box, rounded outwards and clipped to the H x W frame, in fp32 with
    one rounding per operation; None for an empty ROI."""
    x1, y1, x2, y2 = (F32(v) for v in box[:4])
    pad = F32(pad)
    with np.errstate(all="ignore"):
        bw = F32(x2 - x1)
        bh = F32(y2 - y1)
        px = F32(bw * pad)
        py = F32(bh * pad)
        X1, Y1, X2, Y2 = F32(x1 - px), F32(y1 - py), F32(x2 + px), F32(y2 + py)
    if not all(np.isfinite(v) for v in (X1, Y1, X2, Y2)):
        return None
    ix0 = int(min(max(np.floor(X1), F32(0)), F32(W)))
    ix1 = int(min(max(np.ceil(X2), F32(0)), F32(W)))
    iy0 = int(min(max(np.floor(Y1), F32(0)), F32(H)))
    iy1 = int(min(max(np.ceil(Y2), F32(0)), F32(H)))
    w, h = ix1 - ix0, iy1 - iy0
    if w < 1 or h < 1:
        return None
    return ix0, iy0, w, h


def geometry_fails(h, w, oh, ow):
    nh, nw, _, _ = vc.geometry(h, w, oh, ow)
    return nh < 1 or nw < 1


def crop(view, oh, ow, keep_aspect):
    """(h, w, 3) BGR view -> (3, oh, ow) RGB crop; None where the keep-aspect geometry fails."""
    if keep_aspect:
        if geometry_fails(view.shape[0], view.shape[1], oh, ow):
            return None
        return vc.letterbox(view, oh, ow)
    return np.ascontiguousarray(opre.resize_linear(view, oh, ow).transpose(2, 0, 1)[::-1])


def expected(case, oh, ow, keep_aspect, pad, capacity=None):
    """(data (capacity, 3, oh, ow) u8, rois (capacity, 6) i32, total (1,) i32) of a case."""
    boxes, counts = case["boxes"], case["counts"]
    B, M = boxes.shape[:2]
    capacity = B * M if capacity is None else capacity
    data = np.zeros((capacity, 3, oh, ow), np.uint8)
    rois = np.zeros((capacity, 6), np.int32)
    s = 0
    for b in range(B):
        for r in range(min(max(int(counts[b]), 0), M)):
            if s < capacity:
                bgr = case["bgr"][b]
                rc = rect(boxes[b, r], pad, bgr.shape[0], bgr.shape[1])
                c = None
                if rc is not None:
                    x0, y0, w, h = rc
                    c = crop(bgr[y0:y0 + h, x0:x0 + w], oh, ow, keep_aspect)
                rois[s, :2] = (b, r)
                if c is not None:
                    rois[s, 2:] = rc
                    data[s] = c
            s += 1
    return data, rois, np.array([min(s, capacity)], np.int32)


def _frame(kind, seed):
    """(description for lib_frames, BGR image for the restatement)"""
    fmt, h, w, matrix, padding = KINDS[kind]
    if fmt == "nv12":
        y, uv = vc.nv12_planes(h, w, seed, padding)
        return ("nv12", y, uv, matrix), vc.nv12_to_bgr(y, uv, matrix)
    img = vc.bgr_image(h, w, seed)
    wide = np.zeros((h, w + padding, 3), np.uint8)
    wide[:, :w] = img
    return ("bgr", wide[:, :w]), img


def _kind_boxes(kind, oh, ow):
    """Boxes (x1, y1, x2, y2) of one frame kind for an oh x ow crop."""
    if kind == 0:     # 50 x 70 BGR
        return [(0.5, 0.5, 69.5, 49.5), (12, 7, 31, 44), (0, 0, 70, 50), (33.25, 20.75, 33.5, 21.0),
                (-3.5, 40.2, 8.1, 60.0), (69, 49, 70, 50), (10.1, 10.9, 26.6, 14.2), (60, 5, 90, 45)]
    if kind == 1:     # 17 x 23 BGR
        return [(0, 0, 23, 17), (2.2, 3.3, 9.9, 16.1), (22, 16, 23, 17), (22.5, 0, 40, 17), (5, 5, 8, 10)]
    if kind == 2:     # 36 x 64 NV12: odd origins
        out = [(3, 5, 20, 30), (7.5, 1.2, 33.3, 20.9), (-5, -5, 11, 13), (0, 0, 64, 36), (1, 1, 2, 2),
               (63, 35, 64, 36), (31, 3, 34, 8)]
        if ow + 5 <= 64 and oh + 3 <= 36:
            out.append((5, 3, 5 + ow, 3 + oh))            # copy, odd origin
        if 2 * ow + 1 <= 64 and 2 * oh + 1 <= 36:
            out.append((1, 1, 1 + 2 * ow, 1 + 2 * oh))    # exact 2x, odd origin
        return out
    if kind == 3:     # 90 x 40 NV12
        return [(1, 1, 40, 89), (9, 33, 30, 76), (0.4, 10.6, 39.7, 55.5), (35, 80, 60, 100), (13, 27, 16, 32),
                (5, 7, 6, 8)]
    out = [(4, 3, 4 + ow, 3 + oh),                        # the output's size: copy
           (10, 10, 11, 11),                              # 1 x 1
           (20, 30, 23, 35),                              # 3 x 5, upscaled
           (10.3, 5.7, 50.2, 40.9),                       # fractional
           (-10.5, -4, 30, 20), (100, 80, 140.5, 120),    # partly outside
           (130, 10, 150, 30), (-30, -30, -1, -2),        # wholly outside
           (50, 10, 40, 30),                              # x2 < x1
           (NAN, 1, 5, 5), (0, 0, INF, 10), (-INF, 0, 10, 10), (3, NAN, 9, 9),
           (5, 7, 65, 8), (3, 9, 123, 10)]                # 60 x 1, 120 x 1: no keep-aspect geometry
    if 2 * ow + 8 <= 128 and 2 * oh + 6 <= 96:
        out.insert(1, (8, 6, 8 + 2 * ow, 6 + 2 * oh))     # exact 2x: the area path
    return out


def build(oh, ow, batch=8, max_rois=16, seed=0):
    """A case for oh x ow crops: `batch` frames cycling KINDS, every row of boxes filled from its
    kind's list (frame instance j starts at box j * max_rois, cyclically), counts max_rois - b % 3,
    and the last three frames with counts 0, max_rois + 3 and -2."""
    B, M = batch, max_rois
    frames, bgr = [], []
    boxes = np.zeros((B, M, 6), np.float32)
    counts = np.zeros((B,), np.int32)
    seen = {}
    for b in range(B):
        kind = b % len(KINDS)
        f, img = _frame(kind, seed + 11 * b + 1)
        frames.append(f)
        bgr.append(img)
        lst = _kind_boxes(kind, oh, ow)
        j = seen.get(kind, 0)
        seen[kind] = j + 1
        for r in range(M):
            boxes[b, r, :4] = lst[(j * M + r) % len(lst)]
            boxes[b, r, 4] = 0.5 + 0.001 * r
            boxes[b, r, 5] = (b * M + r) % 7
        counts[b] = M - b % 3
    if B >= 3:
        counts[B - 3:] = (0, M + 3, -2)
    return dict(frames=frames, bgr=bgr, boxes=boxes, counts=counts)


def sweep(seed=3):
    """One 96 x 128 BGR frame with 200 integer rectangles, 20 widths x 10 heights: the device's
    double-precision geometry against the host's."""
    f, img = _frame(SWEEP_KIND, seed)
    ws = (1, 2, 3, 5, 7, 8, 13, 16, 21, 31, 32, 33, 47, 63, 64, 65, 80, 97, 127, 128)
    hs = (1, 2, 3, 7, 16, 31, 32, 48, 77, 96)
    boxes = np.zeros((1, len(ws) * len(hs), 6), np.float32)
    k = 0
    for w in ws:
        for h in hs:
            x0, y0 = (k * 7) % (128 - w + 1), (k * 5) % (96 - h + 1)
            boxes[0, k, :4] = (x0, y0, x0 + w, y0 + h)
            k += 1
    return dict(frames=[f], bgr=[img], boxes=boxes, counts=np.array([k], np.int32))


def valid_rects(case, pad):
    """[(frame, rect or None, box)] of every row below its frame's clamped count."""
    M = case["boxes"].shape[1]
    out = []
    for b, n in enumerate(case["counts"]):
        H, W = case["bgr"][b].shape[:2]
        for r in range(min(max(int(n), 0), M)):
            out.append((b, rect(case["boxes"][b, r], pad, H, W), case["boxes"][b, r, :4]))
    return out


def assert_coverage(case, oh, ow, want_area=False):
    """Every branch the box list is there for is present among the valid rows (pad 0)."""
    rows = valid_rects(case, 0.0)
    rects = [(b, rc) for b, rc, _ in rows if rc is not None]
    sizes = {(rc[3], rc[2]) for _, rc in rects}
    assert (oh, ow) in sizes, "no rectangle of the output's size (copy path)"
    assert (1, 1) in sizes and (5, 3) in sizes
    assert any(h < oh and w < ow for h, w in sizes), "no upscaled rectangle"
    if want_area:
        assert (2 * oh, 2 * ow) in sizes, "no exact-2x rectangle (area path)"
    nv12 = [rc for b, rc in rects if case["frames"][b][0] == "nv12"]
    assert any(rc[0] % 2 and rc[1] % 2 for rc in nv12), "no odd NV12 origin"
    assert any(rc[0] % 2 and not rc[1] % 2 for rc in nv12) or any(not rc[0] % 2 and rc[1] % 2 for rc in nv12)
    shape = lambda b: case["bgr"][b].shape[:2]   # noqa: E731
    finite = [(b, rc, bx) for b, rc, bx in rows if np.isfinite(bx).all()]
    assert any(rc is not None and (bx[0] < 0 or bx[1] < 0 or bx[2] > shape(b)[1] or bx[3] > shape(b)[0])
               for b, rc, bx in finite), "no box partly outside its frame"
    assert any(rc is None and bx[2] > bx[0] and bx[3] > bx[1] for b, rc, bx in finite), "no box wholly outside"
    assert any(bx[2] < bx[0] for _, _, bx in finite), "no x2 < x1"
    assert any(np.isnan(bx).any() for _, _, bx in rows), "no NaN row"
    assert any((bx == INF).any() for _, _, bx in rows) and any((bx == -INF).any() for _, _, bx in rows)
    assert all(rc is None for _, rc, bx in rows if not np.isfinite(bx).all())
    assert (1, 60) in sizes
    assert any(geometry_fails(h, w, oh, ow) for h, w in sizes), "no rectangle whose keep-aspect geometry fails"
    assert any(bx[0] != np.floor(bx[0]) or bx[3] != np.floor(bx[3]) for _, _, bx in finite), "no fractional box"
    M = case["boxes"].shape[1]
    assert (case["counts"] == 0).any() and (case["counts"] > M).any() and (case["counts"] < 0).any()


def lib_frames(case, device=None):
    """The case's frames for the library: numpy BGR arrays and preprocess.NV12 objects (host), or
    tensors / NV12 on `device`."""
    import torch
    from yolo_hip import preprocess as pre
    out = []
    for f in case["frames"]:
        if f[0] == "nv12":
            n = pre.NV12(f[1], f[2], f[3])
            out.append(n if device is None else n.to(device))
        else:
            out.append(f[1] if device is None else torch.from_numpy(f[1]).to(device))
    return out
