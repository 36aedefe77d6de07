"""Inputs, path census and oracle shared by the yh_nms / yh_nms_host tests (CPU and GPU).

Every case is named for the edge of csrc/nms.hip it forces; `census` says which paths an input
takes (a numpy restatement of the batch *selection* only - whether the greedy goes on after a
batch is asked of the oracle), and LABELS annotates each case with the labels it must produce.
Cases are built once per process and never modified.

A case is (y float32 (B, 4 + nc, A), kwargs of engine.nms, dtype): dtype None runs y as float32,
torch.float16 / torch.bfloat16 run y cast to it against the oracle's half= mode.
"""
import functools

import numpy as np
import torch

from oracle import nms as onms

# The selection constants of csrc/nms.hip (tests/test_nms_host.py reads its constexpr lines and
# fails when these drift).
FIRST_TARGET = 960   # constexpr int FIRST_TARGET: keys the first batch takes at least
LATER_TARGET = 640   # constexpr int LATER_TARGET: keys a later fast batch takes at least
CAP = 4096           # constexpr int CAP: keys sorted per batch
NB_LDS = 19          # constexpr int NB_LDS: row blocks (of 64) of the mask nms_finish reads from LDS
NBINS = 2048         # constexpr int NBINS: score bins (top 16 bits of the fp32 score)
LDS_ENTRIES = NB_LDS * 64

SIZE_CLASSES = (0, 64, 1024, LDS_ENTRIES, 2048, CAP)


# ---------------------------------------------------------------- census
def _round(a, dtype):
    return onms._round_to(np.array(a, np.float32), dtype)


def _select(C, target, bin_hi):
    """select_bins of nms.hip on the suffix sums C (C[b] = candidates in bins >= b): the next batch
    below bin bin_hi -> ("batch", blo, count, bin_hi) | ("overflow", ...) | ("done", ...)."""
    while True:
        c0 = int(C[bin_hi + 1])
        blo, cnt = -1, int(C[0]) - c0
        if C[0] >= c0 + target:
            b = max(b for b in range(bin_hi + 1) if C[b + 1] < c0 + target <= C[b])
            if C[b] <= c0 + CAP:
                blo, cnt = b - 1, int(C[b]) - c0
            else:
                blo, cnt = b, int(C[b + 1]) - c0
        if cnt > 0:
            return "batch", blo, cnt, bin_hi
        if C[0] == c0:
            return "done", blo, 0, bin_hi
        if blo == bin_hi:
            return "overflow", blo, 0, bin_hi
        bin_hi = blo


def census(y, dtype=None, confidence_threshold=0.001, iou_threshold=0.65, max_det=300, max_nms=30000,
           max_wh=7680.0):
    """-> per image the set of path labels (strings):

    first:0 | first:<=64 | first:<=1024 | first:<=1216 | first:<=2048 | first:<=4096 | first:overflow
    mask_from_workspace      the first batch has more than 1216 entries
    resolve_from_workspace   and the oracle keeps fewer than max_det of the first 1216, so the greedy
                             goes on into the row blocks that are read from the workspace
    later_fast:K             K > 0 fast later batches (whole score bins)
    later_radix:K            K > 0 batches of the general loop; radix_select:K of them had more keys
                             left than they take, so the four digit levels ran
    radix_distinct_scores    the first overflowing bin holds more than one score value
    stop:max_det | stop:max_nms | stop:exhausted
    separable | not_separable   extent of the processed keys <= max_wh / 2, finite, iou >= 0
    degenerate_union         a zero-area, infinite or NaN box among the processed keys

    Processed keys are counted in whole batches, as the selection hands them out."""
    y = _round(y, dtype)
    conf = np.float32(_round([confidence_threshold], dtype)[0])
    bin_base = max(int(conf.view(np.uint32)) >> 16, 0x3F80 - (NBINS - 1))   # post_abi.cpp: yh_nms
    kw = dict(confidence_threshold=confidence_threshold, iou_threshold=iou_threshold, max_det=max_det,
              max_wh=max_wh, half=dtype)
    out = []
    for img in y:
        s = img[4:].T                                    # (A, nc): flat index = pair
        cand = s > conf
        count = int(cand.sum())
        ktot = min(count, max_nms)
        sv = s[cand]
        bins = np.clip((sv.view(np.uint32) >> 16).astype(np.int64) - bin_base, 0, NBINS - 1)
        hist = np.bincount(bins, minlength=NBINS)
        C = np.concatenate([np.cumsum(hist[::-1])[::-1], [0]])

        def goes_on(p):
            kept = onms.non_max_suppression(img[None], max_nms=max(p, 1), **kw)[0].shape[0] if p else 0
            return kept < max_det and p < ktot

        lab = set()
        p, fast, radix, rsel = 0, 0, 0, 0
        sel, blo, cnt, bin_hi = _select(C, FIRST_TARGET, NBINS - 1) if ktot else ("done", -1, 0, NBINS - 1)
        first = min(cnt, ktot)
        lab.add("first:overflow" if sel == "overflow" else
                "first:0" if first == 0 else f"first:<={min(c for c in SIZE_CLASSES if c >= first)}")
        if first > LDS_ENTRIES:
            lab.add("mask_from_workspace")
            if onms.non_max_suppression(img[None], max_nms=LDS_ENTRIES, **kw)[0].shape[0] < max_det:
                lab.add("resolve_from_workspace")
        p = first
        overflow_bin = bin_hi if sel == "overflow" else None
        if sel == "batch":
            bin_hi = blo
            while goes_on(p) and bin_hi >= 0:
                sel, blo, cnt, bin_hi = _select(C, LATER_TARGET, bin_hi)
                if sel != "batch":
                    overflow_bin = bin_hi if sel == "overflow" else None
                    break
                fast += 1
                p += min(cnt, ktot - p)
                bin_hi = blo
        if sel == "overflow":
            if len(np.unique(sv[bins == overflow_bin])) > 1:
                lab.add("radix_distinct_scores")
            while goes_on(p):
                want = min(CAP, ktot - p)
                radix += 1
                rsel += count - p > want
                p += want
        if fast:
            lab.add(f"later_fast:{fast}")
        if radix:
            lab.add(f"later_radix:{radix}")
        if rsel:
            lab.add(f"radix_select:{rsel}")
        kept = onms.non_max_suppression(img[None], max_nms=max(p, 1), **kw)[0].shape[0] if p else 0
        lab.add("stop:max_det" if kept >= max_det else "stop:max_nms" if p < count else "stop:exhausted")
        # the processed keys' plain boxes, in the reference order (score descending, then pair)
        pair = np.flatnonzero(cand.reshape(-1))
        order = pair[np.argsort(-sv.astype(np.float64), kind="stable")][:p]
        box = _round(onms.wh2xy(img[:4].T[order // s.shape[1]]), dtype)
        fin = bool(np.isfinite(box).all())
        ext = (box.max() - box.min()) if p and fin else np.float32(0)
        sep = fin and iou_threshold >= 0 and 0 < max_wh < 3e38 and ext <= np.float32(0.5) * np.float32(max_wh)
        lab.add("separable" if sep else "not_separable")
        with np.errstate(invalid="ignore"):
            area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        if p and (not fin or (area == 0).any()):
            lab.add("degenerate_union")
        out.append(lab)
    return out


# ---------------------------------------------------------------- builders
def _below(rng, shape, conf=0.001):
    return rng.uniform(0.0, 0.9 * conf, size=shape).astype(np.float32)


def one_bin(N, order="shuffled", nc=3, stacked=False):
    """N candidates in the score bin of 0.75, distinct f32 scores, every other score below the
    threshold. One candidate class per anchor; boxes 32 x 32 on a 56-pixel grid whose corners are
    exact in bf16 (multiples of 8 within +-1800), so the same planted overlaps hold in every dtype
    and the classes stay separable. Entry = rank in the reference order. Planted (iou 0.5: a box
    shifted by 8 px overlaps with IoU 0.6, by 16 px with 1 / 3):
      * 64 b (the first entry of row block b >= 1) is shifted 8 px from a keeper among entries 0..15 of
        block 0: a mask word far left of the diagonal, in the last row block too;
      * N - 1 likewise from entry 17;
      * 64 b + 30 from 64 (b - 1) + 31: the word next to the diagonal;
      * 64 b + 20, + 21, + 22: a keeps, suppresses b (8 px), b would suppress c (8 px more; a-c 16 px):
        a chain inside the diagonal word.
    stacked: entries r, r + K, r + 2 K, .. (K = ceil(N / 5)) share one box and class, so one of five is
    kept, each of the others suppressed by an entry K or more ranks (several row blocks) before it, and
    the greedy stays below max_det = 1024 through the last row block: without it 1024 are kept within
    the first 17 blocks and the rows from block 19 on, which nms_finish reads from the workspace, are
    never looked at. The plants above then stand among the first K entries.
    order: "shuffled" ranks the anchors at random (f32); "pair" ranks them by anchor, so the order
    survives rounding the scores to 16 bits (ties break by pair index)."""
    rng = np.random.default_rng(1000 + N)
    A = N + 3 + (N % 5)
    y = np.zeros((1, 4 + nc, A), np.float32)
    y[0, 4:] = _below(rng, (nc, A))
    y[0, 0:2] = -1000.0
    y[0, 2:4] = 16.0
    anchors = np.sort(rng.choice(A, size=N, replace=False))
    if order == "shuffled":
        anchors = rng.permutation(anchors)
    K = (N + 4) // 5 if stacked else N
    cell = np.arange(N) % K
    cls = cell % nc
    gx, gy = cell % 65, cell // 65
    cx, cy = 56.0 * (gx - 32), 56.0 * (gy - 32)

    def plant(j, i, shift):
        if 0 <= i < j < K:
            cx[j], cy[j], cls[j] = cx[i] + shift, cy[i], cls[i]

    for b in range((N + 63) // 64):
        plant(64 * b + 21, 64 * b + 20, 8.0)
        plant(64 * b + 22, 64 * b + 20, 16.0)
        if b:
            plant(64 * b, (5 * b) % 16, 8.0)
            plant(64 * b + 30, 64 * (b - 1) + 31, 8.0)
    if (N - 1) % 64 not in (0, 20, 21, 22, 30) and N - 1 > 64:
        plant(N - 1, 17, -8.0)
    bits = np.uint32(0x3F400000) + (np.uint32(7) * np.arange(N, 0, -1).astype(np.uint32))
    y[0, 0, anchors], y[0, 1, anchors], y[0, 2:4, anchors] = cx, cy, 32.0
    y[0, 4 + cls, anchors] = bits.view(np.float32)
    return y


def radix_bin(first):
    """A bin past CAP of 40 distinct f32 scores (some differing only in the last two bits, which
    share a radix digit with the pair index), each on more than 64 pairs drawn from all 20 800
    (pair indices on both sides of 2^14, so every digit level decides somewhere). Boxes of every
    class piled on one spot, except every 32nd anchor: a small box of its own, kept in every class
    it is a candidate of, so what each batch took shows in the output. first: the bin is all there
    is (overflow at the first selection); else 1500 pairs above it, at most 32 per bin: a first batch,
    one fast later batch, then the bin."""
    rng = np.random.default_rng(31 if first else 32)
    A, nc = 2600, 8
    y = np.zeros((1, 4 + nc, A), np.float32)
    y[0, 0:2] = 320.0 + rng.uniform(-2, 2, size=(2, A))
    y[0, 2:4] = 100.0 + rng.uniform(-2, 2, size=(2, A))
    lone = np.arange(7, A, 32)
    y[0, 0, lone] = 10.0 + 7.0 * (np.arange(len(lone)) % 40)
    y[0, 1, lone] = 600.0 + 7.0 * (np.arange(len(lone)) // 40)
    y[0, 2:4, lone] = 4.0
    s = _below(rng, (A * nc,))
    idx = rng.permutation(A * nc)
    nbin = 9000
    step = np.concatenate([np.arange(8), 8 + 1237 * np.arange(32)]).astype(np.uint32)   # 40 values
    s[idx[:nbin]] = (np.uint32(0x3E800000) + step[rng.integers(0, 40, size=nbin)]).view(np.float32)
    if not first:
        s[idx[nbin:nbin + 1500]] = rng.uniform(0.6, 0.99, 1500).astype(np.float32)
    y[0, 4:] = s.reshape(A, nc).T
    return y


def conf_zero():
    """confidence_threshold = 0: 5000 scores from the smallest subnormal up to 1e-5 are clamped into
    bin 0 (past CAP, hundreds of different top-16-bit values), 300 ordinary scores above. Exact
    zeros are no candidates. Piled boxes with lone ones, as radix_bin."""
    rng = np.random.default_rng(33)
    A, nc = 700, 8
    y = np.zeros((1, 4 + nc, A), np.float32)
    y[0, 0:2] = 320.0 + rng.uniform(-2, 2, size=(2, A))
    y[0, 2:4] = 100.0 + rng.uniform(-2, 2, size=(2, A))
    lone = np.arange(3, A, 16)
    y[0, 0, lone] = 10.0 + 7.0 * np.arange(len(lone))
    y[0, 1, lone] = 600.0
    y[0, 2:4, lone] = 4.0
    s = np.zeros((A * nc,), np.float32)
    idx = rng.permutation(A * nc)
    tiny = np.exp(rng.uniform(np.log(1e-44), np.log(1e-5), 5000)).astype(np.float32)
    tiny[:8] = np.array([1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 1, 1], np.uint32).view(np.float32)
    s[idx[:5000]] = tiny
    s[idx[5000:5300]] = rng.uniform(0.001, 0.99, 300).astype(np.float32)
    y[0, 4:] = s.reshape(A, nc).T
    return y


def scores_ge_one(n_top, largest=float(np.uint32(0x3FFFFFFF).view(np.float32))):
    """Scores in [1, 2) and exactly 1.0 among ordinary ones; scores equal to the threshold and NaN
    scores, which are no candidates. n_top pairs lie in [1, 2): with confidence_threshold = 0 they all
    clamp into the top bin. largest: the top score, the largest value below 2 of the dtype the case runs
    in (yh_nms takes scores in [0, 2), include/yolo_hip.h; the others stay below 1.999, which no 16-bit
    rounding lifts to 2).

    The NaN scores sit on 60 anchors that have no candidate class (one of them NaN in every class).
    Where a NaN shares an anchor with candidates the reference drops the whole anchor (its amax over
    the classes is NaN, util.py:130) while yh_nms and yh_nms_host drop only the NaN pair: a known
    deviation (NMS), not part of this case."""
    rng = np.random.default_rng(34 + n_top)
    A, nc = 1203, 5
    y = np.zeros((1, 4 + nc, A), np.float32)
    y[0, 0:2] = rng.uniform(0, 640, size=(2, A))
    y[0, 2:4] = rng.uniform(20, 200, size=(2, A))
    s = (rng.uniform(0, 1, size=(A * nc,)) ** 6).astype(np.float32)
    idx = rng.permutation(A * nc)
    s[idx[:n_top]] = rng.uniform(1.0, 1.999, n_top).astype(np.float32)
    s[idx[:n_top:3]] = 1.0
    s[idx[1:n_top:7]] = np.float32(largest)
    s[idx[n_top:n_top + 400]] = np.float32(0.001)                            # == threshold
    s = s.reshape(A, nc)
    nan_a = rng.choice(A, size=60, replace=False)
    s[nan_a] = _below(rng, (60, nc))
    s[nan_a, rng.integers(0, nc, size=60)] = np.nan
    s[nan_a[0]] = np.nan
    y[0, 4:] = s.T
    return y


def ragged_130():
    """130 images (nc = 3, A = 203): nms_mask's tile prefix carries across two 64-image chunks, and the
    images with more than one tile (5, 63, 64, 65, 127, 128, 129) sit on both sides of the chunk
    borders. Every 13th image is empty, the next has one candidate."""
    rng = np.random.default_rng(35)
    B, A, nc = 130, 203, 3
    y = np.zeros((B, 4 + nc, A), np.float32)
    y[:, 0:2] = rng.uniform(0, 300, size=(B, 2, A))
    y[:, 2:4] = rng.uniform(10, 120, size=(B, 2, A))
    y[:, 4:] = _below(rng, (B, nc, A))
    for n in range(B):
        k = 0 if n % 13 == 0 else 1 if n % 13 == 1 else int(rng.integers(2, 41))
        if n in (5, 63, 64, 65, 127, 128, 129):
            k = int(rng.integers(65, 400))
        idx = rng.permutation(A * nc)[:k]
        y[n, 4:].reshape(-1)[idx] = rng.uniform(0.01, 0.99, k).astype(np.float32)
    return y


def small_shape(A, nc, seed):
    """Random boxes and scores at a shape whose anchors are no multiple of 8 (nms_emit's and
    for_pairs' element-wise tail) or fewer than 8, and whose classes do not fill nms_emit's 8 groups."""
    rng = np.random.default_rng(seed)
    y = np.empty((2, 4 + nc, A), np.float32)
    y[:, 0:2] = rng.uniform(0, 320, size=(2, 2, A))
    y[:, 2:4] = rng.uniform(10, 150, size=(2, 2, A))
    y[:, 4:] = (rng.uniform(0, 1, size=(2, nc, A)) ** 3).astype(np.float32)
    return y


# The hand-built inputs of tests/test_gpu_nms.py, byte for byte as they were written there.
def cross_class_overlap(case):
    rng = np.random.default_rng(7 if case == "huge_boxes" else 8)
    B, A, nc = 2, 2500, 80
    y = np.empty((B, 4 + nc, A), np.float32)
    y[:, 0:2] = rng.uniform(0, 640, size=(B, 2, A))
    y[:, 2:4] = rng.uniform(8, 200, size=(B, 2, A))
    if case == "huge_boxes":
        y[:, 2:4, ::97] = rng.uniform(4000, 20000, size=(B, 2, y[:, 2:4, ::97].shape[-1]))
    y[:, 4:] = (1 / (1 + np.exp(-rng.normal(-5, 2.5, size=(B, nc, A))))).astype(np.float32)
    return y, (40.0 if case == "small_max_wh" else 7680.0)


def negative_iou():
    rng = np.random.default_rng(11)
    B, A, nc = 2, 900, 80
    y = np.empty((B, 4 + nc, A), np.float32)
    y[:, 0:2] = rng.uniform(0, 640, size=(B, 2, A))
    y[:, 2:4] = rng.uniform(8, 60, size=(B, 2, A))
    y[:, 2:4, ::50] = 0.0   # zero-area boxes: 0 / 0 union, NaN IoU never suppresses
    y[:, 4:] = (1 / (1 + np.exp(-rng.normal(-5, 2.5, size=(B, nc, A))))).astype(np.float32)
    return y


def few_kept(scores):
    """-> y, the kwargs the continuation test runs it with"""
    if scores == "spread_then_tied":
        rng = np.random.default_rng(23)
        B, A, nc = 2, 1050, 8   # A: not a multiple of 8
    else:
        rng = np.random.default_rng(21)
        B, A, nc = 2, 8400, 8
    y = np.empty((B, 4 + nc, A), np.float32)
    y[:, 0:2] = 320.0 + rng.uniform(-2, 2, size=(B, 2, A))
    y[:, 2:4] = 100.0 + rng.uniform(-2, 2, size=(B, 2, A))
    kws = (dict(), dict(max_nms=50000, max_det=5))
    if scores == "spread":
        y[:, 4:] = rng.uniform(0.01, 0.99, size=(B, nc, A)).astype(np.float32)
    elif scores == "tied":
        y[:, 4:] = 0.5
    else:
        k = np.arange(11)
        lone = 7 + 100 * k
        y[:, 0, lone] = 10.0 + 6.0 * k
        y[:, 1, lone] = 600.0
        y[:, 2:4, lone] = 4.0
        y[:, 4:] = 0.25
        for b in range(B):
            idx = rng.permutation(nc * A)[:1500]
            y[b, 4:].reshape(-1)[idx] = rng.uniform(0.6, 0.99, 1500)
        kws = (dict(max_det=300, max_nms=30000), dict(max_det=40, max_nms=30000), dict(max_det=300, max_nms=5000))
    return y, kws


# ---------------------------------------------------------------- the case list
SIZES = (1, 64, 65, 1024, 1025, 1216, 1217, 2048, 2049, 4096, 4097)
HALF_SIZES = (65, 1217, 4097)
F16, BF16 = torch.float16, torch.bfloat16
_DT = {"f16": F16, "bf16": BF16}


def _size_labels(N, max_det):
    lab = {"first:overflow" if N > CAP else f"first:<={min(c for c in SIZE_CLASSES if c >= N)}", "separable"}
    if LDS_ENTRIES < N <= CAP:
        lab.add("mask_from_workspace")
    if N > CAP:
        lab |= {"later_radix:1", "radix_select:1", "radix_distinct_scores"}
    return lab


# name -> (builder thunk -> y, kwargs, dtype, labels the case must produce in some image)
CASES = {}
for _N in SIZES:
    for _md in (1024, 300):
        CASES[f"bin{_N}_md{_md}"] = (functools.partial(one_bin, _N), dict(iou_threshold=0.5, max_det=_md), None,
                                     _size_labels(_N, _md))
for _N in HALF_SIZES:
    for _d in _DT:   # a bf16 bin is one value: every bin is fully tied
        CASES[f"bin{_N}_{_d}"] = (functools.partial(one_bin, _N, "pair"), dict(iou_threshold=0.5, max_det=1024), _DT[_d],
                                  _size_labels(_N, 1024) - {"radix_distinct_scores"})
for _N in (1217, 2049, 4096):   # one of five kept: the greedy reaches the last row block
    CASES[f"bin{_N}_stacked"] = (functools.partial(one_bin, _N, stacked=True), dict(iou_threshold=0.5, max_det=1024), None,
                                 _size_labels(_N, 1024) | {"resolve_from_workspace", "stop:exhausted"})
CASES["bin4097_stacked"] = (functools.partial(one_bin, 4097, stacked=True), dict(iou_threshold=0.5, max_det=1024), None,
                            (_size_labels(4097, 1024) - {"later_radix:1"}) | {"later_radix:2", "stop:exhausted"})
CASES["bin2049_stacked_bf16"] = (functools.partial(one_bin, 2049, "pair", stacked=True), dict(iou_threshold=0.5, max_det=1024),
                                 BF16, _size_labels(2049, 1024) | {"resolve_from_workspace", "stop:exhausted"})
CASES.update({
    # overflow at the first selection (want == 0): 4096 + 4096 by radix select, then the 808 left
    "radix_first": (functools.partial(radix_bin, True), dict(max_det=1024), None,
                    {"first:overflow", "later_radix:3", "radix_select:2", "radix_distinct_scores", "stop:exhausted"}),
    "radix_first_max_nms": (functools.partial(radix_bin, True), dict(max_det=1024, max_nms=6000), None,
                            {"first:overflow", "later_radix:2", "radix_select:2", "stop:max_nms"}),
    "radix_first_max_det": (functools.partial(radix_bin, True), dict(max_det=150), None,
                            {"first:overflow", "later_radix:2", "stop:max_det"}),
    "radix_after_fast": (functools.partial(radix_bin, False), dict(max_det=1024), None,
                         {"first:<=1024", "later_fast:1", "later_radix:3", "radix_select:2", "radix_distinct_scores"}),
    "radix_after_fast_max_nms": (functools.partial(radix_bin, False), dict(max_det=1024, max_nms=7500), None,
                                 {"later_fast:1", "later_radix:2", "radix_select:2", "stop:max_nms"}),
    "conf_zero": (conf_zero, dict(confidence_threshold=0.0, max_det=1024), None,
                  {"first:<=1024", "later_radix:2", "radix_select:1", "radix_distinct_scores", "stop:exhausted"}),
    "ge_one": (functools.partial(scores_ge_one, 900), dict(), None, {"stop:max_det"}),
    "ge_one_conf_zero": (functools.partial(scores_ge_one, 4600), dict(confidence_threshold=0.0, iou_threshold=0.3), None,
                         {"first:overflow", "radix_distinct_scores"}),
    "ge_one_f16": (functools.partial(scores_ge_one, 900, 2.0 - 2.0 ** -10), dict(), F16, set()),
    "ragged_130": (ragged_130, dict(), None, {"first:0", "first:<=64", "first:<=1024", "stop:exhausted"}),
    "ragged_130_f16": (ragged_130, dict(), F16, {"first:0", "first:<=64", "first:<=1024"}),
    "ragged_130_bf16": (ragged_130, dict(), BF16, {"first:0", "first:<=64", "first:<=1024"}),
    "A5_nc1": (functools.partial(small_shape, 5, 1, 41), dict(), None, {"first:<=64"}),
    "A7_nc11": (functools.partial(small_shape, 7, 11, 42), dict(), None, {"first:<=1024"}),
    "A1001_nc13": (functools.partial(small_shape, 1001, 13, 43), dict(max_det=17), None, {"stop:max_det"}),
    "A1001_nc13_bf16": (functools.partial(small_shape, 1001, 13, 43), dict(), BF16, set()),
    # the hand-built inputs (their own tests run every setting; the label is of the one named here)
    "cross_class_small_max_wh": (lambda: cross_class_overlap("small_max_wh")[0], dict(max_wh=40.0), None, {"not_separable"}),
    "cross_class_huge_boxes": (lambda: cross_class_overlap("huge_boxes")[0], dict(), None, {"not_separable"}),
    "negative_iou": (negative_iou, dict(iou_threshold=-0.1), None, {"not_separable", "degenerate_union"}),
    "few_kept_spread": (lambda: few_kept("spread")[0], dict(max_det=300, max_nms=5000), None,
                        {"first:<=1216", "later_fast:5", "stop:max_nms"}),
    "few_kept_tied": (lambda: few_kept("tied")[0], dict(max_det=300, max_nms=9000), None,
                      {"first:overflow", "later_radix:3", "stop:max_nms"}),
    "few_kept_spread_then_tied": (lambda: few_kept("spread_then_tied")[0], dict(max_det=300, max_nms=30000), None,
                                  {"later_fast:1", "later_radix:2", "stop:exhausted"}),
})
ALL = list(CASES)
LARGEST = "radix_first"     # B = 1: fits the workspace of every case; overflow, radix, every section written
LABELS = {k: v[3] for k, v in CASES.items()}

# every label the census can produce that the list must cover
REQUIRED = ({"first:overflow", "first:0", "mask_from_workspace", "resolve_from_workspace", "radix_distinct_scores", "separable",
             "not_separable", "degenerate_union", "stop:max_det", "stop:max_nms", "stop:exhausted"}
            | {f"first:<={c}" for c in SIZE_CLASSES[1:]})
REQUIRED_PREFIXES = ("later_fast:", "later_radix:", "radix_select:")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (y float32 CPU tensor (read-only), kwargs, dtype)"""
    build, kw, dtype, _ = CASES[name]
    y = np.ascontiguousarray(build(), np.float32)
    if dtype is not None:
        y = onms._round_to(y, dtype)
    y.setflags(write=False)
    return y, dict(kw), dtype


def tensor(name):
    """the case's input as engine.nms / engine.nms_host take it"""
    y, _, dtype = case(name)
    t = torch.from_numpy(y.copy())
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def want(name):
    """the oracle's kept rows per image"""
    y, kw, dtype = case(name)
    return onms.non_max_suppression(y, half=dtype, **kw)


@functools.lru_cache(maxsize=None)
def labels(name):
    y, kw, dtype = case(name)
    return census(y, dtype, **kw)


def assert_same(got, wanted, what=""):
    assert len(got) == len(wanted)
    for i, (a, b) in enumerate(zip(got, wanted)):
        assert a.shape == b.shape, f"{what} image {i}: kept {a.shape[0]} vs {b.shape[0]}"
        np.testing.assert_array_equal(a, b, err_msg=f"{what} image {i}")
