"""Detection metrics of the reference's eval loop, on the device.

  compute_metric  utils/util.py:99-120   IoU matching of one image's detections to its labels
  match_batch     the same for a whole batch in one HIP launch (yh_match / yh_match_host),
                  straight from the fixed-size NMS output
  compute_ap      utils/util.py:225-300  PR curves, AP@0.5 and AP@0.5:0.95 over the dataset
  smooth          utils/util.py:172-177  box filter used to pick the max-F1 confidence

main.py:test (264-300) calls them per batch after non_max_suppression. The
reference moves every image's IoU matrix to the host and loops in numpy; here
the matching is vectorised over all IoU thresholds at once on the tensor's
device, and compute_ap's sort / cumulative sums / 1000- and 101-point
interpolations run in float64 torch (device of choice), so the eval loop never
leaves the GPU until the final scalars.

Matching semantics (util.py:108-119), reproduced exactly: a (label, detection)
pair is a candidate at threshold t when IoU >= t and the classes are equal; each
detection keeps its highest-IoU candidate label; then each label keeps, among
the detections that kept it, the one with the LOWEST detection index (the
reference's second numpy.unique runs over matches ordered by detection, not by
IoU). Exact IoU ties between two labels of one detection are ordered by
numpy's unstable argsort in the reference; here the lower label index wins
(parity unpinned for such ties only).

match_batch states the same rule in one pass over all thresholds: best[d] is the
equal-class label with the highest IoU (lower label on ties), biou[d] that IoU,
and tp[d, t] holds iff biou[d] >= iou_v[t] and no earlier detection e < d with
best[e] == best[d] has biou[e] >= iou_v[t]. (At threshold t a detection's best
candidate is its overall best label whenever that one is a candidate at all, so
the per-threshold argmax of compute_metric never picks another label.)
"""
import ctypes
import os

import numpy
import torch


def _iou(target, output):
    """(L, 5) [cls, x1, y1, x2, y2] x (D, >=4) boxes -> (L, D) IoU, util.py:101-105 arithmetic."""
    a1, a2 = target[:, 1:3].unsqueeze(1), target[:, 3:5].unsqueeze(1)
    b1, b2 = output[:, 0:2].unsqueeze(0), output[:, 2:4].unsqueeze(0)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + 1e-7)


def compute_metric(output, target, iou_v):
    """output (D, 6) [x1, y1, x2, y2, score, cls], target (L, 5) [cls, x1, y1, x2, y2],
    iou_v (T,) thresholds -> (D, T) bool: detection d is a true positive at threshold t."""
    iou = _iou(target, output)                                   # (L, D)
    same = target[:, 0:1] == output[:, 5]                        # (L, D)
    L, D = iou.shape
    T = iou_v.shape[0]
    if L == 0 or D == 0:
        return torch.zeros((D, T), dtype=torch.bool, device=output.device)
    cand = (iou.unsqueeze(0) >= iou_v.view(T, 1, 1).to(iou.dtype)) & same.unsqueeze(0)   # (T, L, D)
    # per (threshold, detection): the best candidate label (highest IoU, lower label on ties)
    score = torch.where(cand, iou.unsqueeze(0), torch.full_like(iou, -1.0).unsqueeze(0))
    best = score.argmax(dim=1, keepdim=False)                    # (T, D) first max = lowest label
    has = cand.any(dim=1)                                        # (T, D)
    # per (threshold, label): the lowest detection index among the detections that kept it
    big = torch.full((T, L), D, dtype=torch.long, device=iou.device)
    det = torch.arange(D, device=iou.device).expand(T, D)
    best_or_sink = torch.where(has, best, torch.full_like(best, L))   # unmatched detections -> row L (dropped)
    first = torch.cat([big, big[:, :1]], dim=1).scatter_reduce(1, best_or_sink, det, reduce="amin")[:, :L]
    correct = torch.zeros((T, D + 1), dtype=torch.bool, device=iou.device)
    correct.scatter_(1, first, True)
    return correct[:, :D].t().contiguous()


def _check(name, t, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"yolo_hip.match_batch: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"yolo_hip.match_batch: {name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"yolo_hip.match_batch: {name} is on {t.device}, expected {device}")
    if len(shape) != t.dim() or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        want = tuple("*" if w is None else w for w in shape)
        raise ValueError(f"yolo_hip.match_batch: {name} has shape {tuple(t.shape)}, expected {want}")
    if not t.is_contiguous():
        raise ValueError(f"yolo_hip.match_batch: {name} must be contiguous")


def match_batch(dets, counts, labels, offsets, iou_v, out=None, score_cls=None, counts_out=None, threads=0):
    """compute_metric for a whole batch in one launch, from the NMS output as it stands.

    dets (B, max_det, 6) f32 and counts (B,) i32 as `nms` returns them (rows at or beyond
    counts[b] are never read); labels (N, 5) f32 [cls, x1, y1, x2, y2] in pixels grouped by
    image; offsets (B + 1,) i32 ascending within [0, N] - image b owns labels
    offsets[b]:offsets[b + 1]; iou_v (T,) f32, 1 <= T <= 32. All on one device, all contiguous.
    -> tp (B, max_det, T) uint8 (`out` if given; every byte written, 0 beyond counts[b]).

    cuda tensors run the HIP kernel (yh_match) asynchronously on the current stream, CPU
    tensors the host twin (yh_match_host, `threads` <= 0: every hardware thread). Optional
    score_cls (B, max_det, 2) f32 receives columns 4, 5 of the valid rows (0 beyond) and
    counts_out (B,) i32 the counts clamped to [0, max_det]."""
    from ._lib import check, lib
    if not isinstance(dets, torch.Tensor) or dets.dim() != 3:
        raise ValueError("yolo_hip.match_batch: dets must be a (B, max_det, 6) tensor")
    dev = dets.device
    B, md = dets.shape[0], dets.shape[1]
    _check("dets", dets, (B, md, 6), torch.float32, dev)
    _check("counts", counts, (B,), torch.int32, dev)
    _check("labels", labels, (None, 5), torch.float32, dev)
    _check("offsets", offsets, (B + 1,), torch.int32, dev)
    _check("iou_v", iou_v, (None,), torch.float32, dev)
    T = iou_v.shape[0]
    if out is None:
        out = torch.empty((B, md, T), dtype=torch.uint8, device=dev)
    else:
        _check("out", out, (B, md, T), torch.uint8, dev)
    if score_cls is not None:
        _check("score_cls", score_cls, (B, md, 2), torch.float32, dev)
    if counts_out is not None:
        _check("counts_out", counts_out, (B,), torch.int32, dev)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    args = (ptr(dets), ptr(counts), B, md, ptr(labels), ptr(offsets), ptr(iou_v), T, ptr(out), ptr(score_cls),
            ptr(counts_out))
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            check(lib().yh_match(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "match")
    elif dev.type == "cpu":
        check(lib().yh_match_host(*args, int(threads)), "match_host")
    else:
        raise ValueError(f"yolo_hip.match_batch: unsupported device {dev}")
    return out


def smooth(y, f=0.1):
    """Box filter of fraction f with edge padding (util.py:172-177); y: 1-D float64 tensor."""
    nf = round(len(y) * f * 2) // 2 + 1
    p = nf // 2
    yp = torch.cat([y[:1].expand(p), y, y[-1:].expand(p)])
    k = torch.full((nf,), 1.0 / nf, dtype=y.dtype, device=y.device)
    return torch.nn.functional.conv1d(yp.view(1, 1, -1), k.view(1, 1, -1)).view(-1)


def _interp(x, xp, fp, left=None):
    """numpy.interp for increasing xp (duplicates allowed), evaluated like numpy's C loop."""
    j = torch.searchsorted(xp, x, right=True) - 1                # last j with xp[j] <= x
    n = xp.shape[0]
    jc = j.clamp(0, max(n - 2, 0))
    if n == 1:
        res = fp[0].expand_as(x).clone()
    else:
        x0, x1, y0, y1 = xp[jc], xp[jc + 1], fp[jc], fp[jc + 1]
        slope = (y1 - y0) / (x1 - x0)
        res = slope * (x - x0) + y0
        bad = torch.isnan(res)
        res = torch.where(bad, slope * (x - x1) + y1, res)
        res = torch.where(torch.isnan(res) & (y0 == y1), y0, res)
    res = torch.where(x >= xp[-1], fp[-1], res)                  # at / past the last point
    res = torch.where(x < xp[0], fp[0] if left is None else torch.as_tensor(left, dtype=fp.dtype,
                                                                             device=fp.device), res)
    return res


def _plot_curves(path, px, curves, mean, mean_label, names, labels, x_label, y_label, title):
    """One 9 x 6 in figure at 250 dpi (util.py:180-222): the per-class curves with a legend entry
    each when 0 < len(names) < 21, thin grey lines otherwise, and the thick mean curve."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg   # Agg canvas directly: no pyplot state
    from matplotlib.figure import Figure
    fig = Figure(figsize=(9, 6), tight_layout=True)
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    per_class = 0 < len(names) < 21
    for i, y in enumerate(curves):
        if per_class:
            ax.plot(px, y, linewidth=1, label=labels[i] if i < len(labels) else None)
        else:
            ax.plot(px, y, linewidth=1, color="grey")
    ax.plot(px, mean, linewidth=3, color="blue", label=mean_label)
    ax.set_xlabel(x_label)
    ax.set_ylabel(y_label)
    ax.set_xlim(0, 1)
    ax.set_ylim(0, 1)
    ax.legend(bbox_to_anchor=(1.04, 1), loc="upper left")
    ax.set_title(title)
    fig.savefig(path, dpi=250)


def _plot_all(save_dir, px, py, ap, f1, p, r, names, classes):
    """PR_curve / F1_curve / P_curve / R_curve .png of util.py:286-292 into save_dir."""
    os.makedirs(save_dir, exist_ok=True)
    present = set(float(c) for c in classes)
    items = names.items() if isinstance(names, dict) else enumerate(names)
    names = [v for k, v in items if float(k) in present]                 # only classes that have data
    px = px.cpu().numpy()
    ap = ap.cpu().numpy()
    if py:
        pr = numpy.stack([y.cpu().numpy() for y in py], axis=0)          # one row per class with data
        pr_mean = pr.mean(0)
    else:
        pr, pr_mean = numpy.zeros((0, px.shape[0])), numpy.zeros_like(px)
    pr_labels = [f"{names[i]} {ap[i, 0]:.3f}" for i in range(min(len(names), len(pr)))]
    _plot_curves(os.path.join(save_dir, "PR_curve.png"), px, pr, pr_mean,
                 "all classes %.3f mAP@0.5" % (ap[:, 0].mean() if ap.shape[0] else 0.0), names, pr_labels,
                 "Recall", "Precision", "Precision-Recall Curve")
    for fname, curve, label in (("F1_curve.png", f1, "F1"), ("P_curve.png", p, "Precision"),
                                ("R_curve.png", r, "Recall")):
        y = smooth(curve.mean(0), 0.05).cpu().numpy()
        mean_label = f"all classes {y.max():.3f} at {px[y.argmax()]:.3f}"
        _plot_curves(os.path.join(save_dir, fname), px, curve.cpu().numpy(), y, mean_label, names,
                     [str(n) for n in names], "Confidence", label, f"{label}-Confidence Curve")


def compute_ap(tp, conf, output, target, plot=False, names=(), eps=1e-16, device=None, save_dir="./weights"):
    """util.py:225-300: -> (tp, fp, m_pre, m_rec, map50, mean_ap).

    Inputs as the reference takes them (numpy, from the concatenated per-image
    metrics) or tensors; computed in float64 on `device` (default: the tensors'
    device, else CUDA when available).

    plot=True also writes PR_curve.png, F1_curve.png, P_curve.png and R_curve.png
    (util.py:180-222; 9 x 6 in at 250 dpi, Agg backend) into save_dir, created if
    missing; `names` (class index -> name) is filtered to the classes present in
    `target`. The returned values do not depend on `plot`."""
    if device is None:
        device = tp.device if isinstance(tp, torch.Tensor) else ("cuda" if torch.cuda.is_available() else "cpu")
    f64 = dict(dtype=torch.float64, device=device)
    tp = torch.as_tensor(numpy.asarray(tp) if not isinstance(tp, torch.Tensor) else tp).to(**f64)
    conf = torch.as_tensor(numpy.asarray(conf) if not isinstance(conf, torch.Tensor) else conf).to(**f64)
    output = torch.as_tensor(numpy.asarray(output) if not isinstance(output, torch.Tensor) else output).to(**f64)
    target = torch.as_tensor(numpy.asarray(target) if not isinstance(target, torch.Tensor) else target).to(**f64)
    if tp.dim() == 1:
        tp = tp[:, None]
    order = torch.argsort(-conf, stable=True)
    tp, conf, output = tp[order], conf[order], output[order]
    classes, nt = torch.unique(target, return_counts=True)
    nc = classes.shape[0]
    # numpy's linspace grid, bit for bit: the 101 COCO points land exactly on recall
    # steps (0.28, 0.72, ...) where m_pre jumps, so a 1-ulp different grid (torch.linspace
    # fills from both ends) picks the other side of the jump
    px = torch.from_numpy(numpy.linspace(0, 1, 1000)).to(**f64)
    x101 = torch.from_numpy(numpy.linspace(0, 1, 101)).to(**f64)
    p = torch.zeros((nc, 1000), **f64)
    r = torch.zeros((nc, 1000), **f64)
    ap = torch.zeros((nc, tp.shape[1]), **f64)
    py = []                                                      # precision at mAP@0.5 on px (plots)
    for ci in range(nc):
        sel = output == classes[ci]
        nl = nt[ci].item()
        no = int(sel.sum().item())
        if no == 0 or nl == 0:
            continue
        tps = tp[sel]
        fpc = (1 - tps).cumsum(0)
        tpc = tps.cumsum(0)
        recall = tpc / (nl + eps)
        xs = -conf[sel]                                          # increasing (conf sorted descending)
        r[ci] = _interp(-px, xs, recall[:, 0], left=0.0)
        precision = tpc / (tpc + fpc)
        p[ci] = _interp(-px, xs, precision[:, 0], left=1.0)
        one = torch.ones(1, **f64)
        zero = torch.zeros(1, **f64)
        for j in range(tp.shape[1]):
            m_rec = torch.cat([zero, recall[:, j], one])
            m_pre = torch.cat([one, precision[:, j], zero])
            m_pre = torch.flip(torch.cummax(torch.flip(m_pre, [0]), 0).values, [0])
            y = _interp(x101, m_rec, m_pre)
            ap[ci, j] = torch.trapezoid(y, x101)
            if plot and j == 0:
                py.append(_interp(px, m_rec, m_pre))
    f1 = 2 * p * r / (p + r + eps)
    if plot:
        _plot_all(save_dir, px, py, ap, f1, p, r, names, classes.cpu().tolist())
    i = int(smooth(f1.mean(0), 0.1).argmax().item())
    p, r, f1 = p[:, i], r[:, i], f1[:, i]
    tp_n = (r * nt.to(torch.float64)).round()
    fp_n = (tp_n / (p + eps) - tp_n).round()
    ap50, apm = ap[:, 0], ap.mean(1)
    return (tp_n.cpu().numpy(), fp_n.cpu().numpy(), p.mean().item(), r.mean().item(),
            ap50.mean().item(), apm.mean().item())
