"""Inputs and oracle shared by the yh_match / yh_match_host tests (CPU and GPU).

The oracle is yolo_hip.metrics.compute_metric, per image, on the same tensors
(its rule for exact label-IoU ties - the lower label wins - is the project's).
Cases are built once per process and never modified.
"""
import functools

import numpy as np
import torch

from conftest import load_golden
from yolo_hip.metrics import compute_metric

# name -> (batch, max_det, thresholds, detections per image, labels per image, grid)
#   detections / labels per image: an int (every image) or (lo, hi) drawn per image
#   grid: corners on multiples of 8 in a 48-pixel square, two classes -> many exact IoU
#         ties, duplicate boxes and IoUs of exactly 0 and 1; else jittered float boxes
T10 = tuple(np.linspace(0.5, 0.95, 10).astype(np.float32).tolist())
T32 = tuple(np.linspace(0.0, 1.0, 32).astype(np.float32).tolist())      # includes 0.0 and 1.0
CASES = {
    "no_dets": (2, 32, T10, 0, (1, 6), False),
    "no_labels": (2, 32, T10, (1, 32), 0, False),
    "nothing": (1, 32, T10, 0, 0, False),
    "full_one_label": (1, 300, T10, 300, 1, "same"),       # D = max_det, L = 1, one class, identical boxes
    "many_labels": (1, 70, T10, 70, 1000, True),           # L spans several label chunks on the device
    "odd_max_det_t1": (3, 70, (0.5,), (0, 70), (0, 12), True),
    "t32_b33_grid": (33, 70, T32, (0, 70), (0, 12), True),
    "t32_b1_float": (1, 70, T32, 70, 9, False),
    "t10_b33_float": (33, 32, T10, (0, 32), (0, 9), False),
    "two_det_rounds": (2, 300, T10, (257, 300), (0, 90), True),   # more detections than threads in a block
    "cap_max_det": (1, 4096, T10, 700, 60, True),          # YH_MATCH_MAX_DET: the largest LDS carve
}


def _grid_boxes(rng, n):
    a = rng.integers(0, 6, size=(n, 2)) * 8
    span = rng.integers(1, 4, size=(n, 2)) * 8
    return np.concatenate([a, np.minimum(a + span, 48)], 1).astype(np.float32)


def _float_boxes(rng, n):
    xy = rng.uniform(0, 500, size=(n, 2))
    wh = rng.uniform(8, 140, size=(n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _draw(rng, spec):
    return int(spec) if isinstance(spec, int) else int(rng.integers(spec[0], spec[1] + 1))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict of CPU tensors: dets (B, md, 6), counts (B,), labels (N, 5), offsets (B + 1,),
    iou_v (T,), want (B, md, T) uint8 (the oracle; 0 beyond counts). Padding rows of dets
    are duplicates of valid rows (or of a foreign box when the image has none)."""
    if name == "golden":
        return _golden()
    B, md, thr, nd, nl, grid = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    dets = np.zeros((B, md, 6), np.float32)
    counts = np.zeros((B,), np.int32)
    labels, offsets = [], [0]
    for b in range(B):
        D, L = _draw(rng, nd), _draw(rng, nl)
        if grid == "same":
            box = np.tile(np.array([[8, 8, 40, 32]], np.float32), (max(D, 1), 1))
            cls = np.ones((max(D, 1),), np.float32)
            lab = np.concatenate([np.ones((L, 1), np.float32), np.tile(box[:1], (L, 1))], 1)
        elif grid:
            box = _grid_boxes(rng, max(D, 1))
            cls = rng.integers(0, 2, size=(max(D, 1),)).astype(np.float32)
            lab = np.concatenate([rng.integers(0, 2, size=(L, 1)).astype(np.float32), _grid_boxes(rng, L)], 1)
        else:
            box = _float_boxes(rng, max(D, 1))
            cls = rng.integers(0, 4, size=(max(D, 1),)).astype(np.float32)
            # labels: jittered copies of detections (some share a detection), a few strays
            src = rng.integers(0, max(D, 1), size=(L,))
            lb = box[src] + rng.normal(0, 6, size=(L, 4)).astype(np.float32)
            lc = np.where(rng.uniform(size=(L,)) < 0.8, cls[src], rng.integers(0, 4, size=(L,))).astype(np.float32)
            lab = np.concatenate([lc[:, None], lb], 1).astype(np.float32)
        score = np.sort(rng.uniform(0.001, 1, size=(max(D, 1),)).astype(np.float32))[::-1]
        rows = np.concatenate([box, score[:, None], cls[:, None]], 1)
        dets[b] = rows[np.arange(md) % len(rows)]          # valid rows first, then duplicates
        counts[b] = D
        labels.append(lab)
        offsets.append(offsets[-1] + L)
    labels = np.concatenate(labels, 0).reshape(-1, 5).astype(np.float32)
    return _finish(dets, counts, labels, np.asarray(offsets, np.int32), np.asarray(thr, np.float32))


def _golden():
    """The 24 images of metrics_synth.npz as one batch with max_det = 32."""
    g = load_golden("metrics_synth.npz")
    n, md = int(g["n_img"]), 32
    dets = np.zeros((n, md, 6), np.float32)
    counts = np.zeros((n,), np.int32)
    labels, offsets = [], [0]
    for i in range(n):
        out = g[f"out_{i}"]
        src = out if len(out) else g["out_0"]
        dets[i] = src[np.arange(md) % len(src)]
        counts[i] = len(out)
        labels.append(g[f"tgt_{i}"].reshape(-1, 5))
        offsets.append(offsets[-1] + len(labels[-1]))
    c = _finish(dets, counts, np.concatenate(labels, 0).astype(np.float32), np.asarray(offsets, np.int32),
                np.linspace(0.5, 0.95, 10).astype(np.float32))
    c["iou_v"] = torch.linspace(0.5, 0.95, 10)            # the thresholds tests/test_metrics.py uses
    c["want"] = _oracle(c)
    for i in range(n):                                      # and the reference's own answer
        d = int(counts[i])
        assert np.array_equal(c["want"][i, :d].numpy().astype(bool), g[f"correct_{i}"]), i
    return c


def _oracle(c):
    B, md = c["dets"].shape[:2]
    T = c["iou_v"].shape[0]
    want = torch.zeros((B, md, T), dtype=torch.uint8)
    for b in range(B):
        d = int(c["counts"][b])
        lo, hi = int(c["offsets"][b]), int(c["offsets"][b + 1])
        want[b, :d] = compute_metric(c["dets"][b, :d], c["labels"][lo:hi], c["iou_v"]).to(torch.uint8)
    return want


def _finish(dets, counts, labels, offsets, thr):
    c = dict(dets=torch.from_numpy(dets), counts=torch.from_numpy(counts), labels=torch.from_numpy(labels),
             offsets=torch.from_numpy(offsets), iou_v=torch.from_numpy(thr))
    c["want"] = _oracle(c)
    return c


def oracle_on(c, device):
    """compute_metric per image on `device` copies of the case -> (B, md, T) uint8 on the CPU."""
    on = {k: c[k].to(device) for k in ("dets", "labels", "iou_v")}
    on["counts"], on["offsets"] = c["counts"], c["offsets"]       # host ints for the slicing
    return _oracle(on)


ALL = ["golden"] + list(CASES)
