"""Tracking evaluation on the device (yh_mot_eval): the CLEAR-MOT counts (TP, FP, FN, identity
switches, MOTA, MOTP) and IDF1 of tracked sequences against ground truth, for a batch of sequences
and a list of IoU thresholds in one launch. `mot_eval` is the call on stacked tensors,
`TrackEvaluator` collects the frames a `Tracker` returns and computes the scores, `mot_workspace`
sizes the kernel's workspace. The rules are stated in include/yolo_hip.h.
"""
import numpy as np
import torch

from ._call import host_stream_ids, run, tensor

MAX_ROWS, MAX_IDS, MAX_THR, MAX_FRAMES = 256, 1024, 16, 65535   # YH_MOT_MAX_*
COLUMNS = ("tp", "fp", "fn", "idsw", "siou", "idtp", "gt", "hyp")
_WHO = "yolo_hip.mot_eval"


def mot_workspace(sequences, num_thr, n_gt_ids, n_tr_ids, device="cpu"):
    """The workspace `mot_eval` needs on a cuda device (a uint8 tensor; the overlap counts of every
    sequence and threshold)."""
    from ._lib import lib
    need = lib().yh_mot_workspace_bytes(int(sequences), int(num_thr), int(n_gt_ids), int(n_tr_ids))
    return torch.empty((need,), dtype=torch.uint8, device=device)


def mot_eval(tr, tr_ids, tr_counts, gt, gt_ids, gt_counts, thr, n_gt_ids, n_tr_ids, frames=None, class_aware=True,
             out=None, workspace=None, threads=0):
    """tr (S, F, max_out, 6) f32, tr_ids (S, F, max_out) i32, tr_counts (S, F) i32: the rows `track`
    wrote, stacked frame-major; gt (S, F, max_gt, 5) f32 = x1, y1, x2, y2, class, gt_ids (S, F, max_gt)
    i32, gt_counts (S, F) i32; thr (num_thr,) f32; frames (S,) i32 or None: the live frames of each
    sequence. Rows whose id is outside [0, n_gt_ids) / [0, n_tr_ids) take part in nothing.
    -> (counts (S, num_thr, 8) int64: TP, FP, FN, IDSW, SIOU, IDTP, GT rows, hypothesis rows;
    ignored (S, 2) int32); out=(counts, ignored) reuses buffers, every byte is written.
    cuda tensors run the kernel on the current stream (workspace: `mot_workspace`'s, allocated when
    not given), CPU tensors the host twin: the same bytes. Nothing is read back."""
    if not isinstance(tr, torch.Tensor) or tr.dim() != 4 or not isinstance(gt, torch.Tensor) or gt.dim() != 4:
        raise ValueError(f"{_WHO}: tr must be (S, F, max_out, 6) and gt (S, F, max_gt, 5)")
    dev = tr.device
    S, F, mo = tr.shape[:3]
    mg = gt.shape[2]
    tensor(_WHO, "tr", tr, (S, F, mo, 6), torch.float32, dev)
    tensor(_WHO, "tr_ids", tr_ids, (S, F, mo), torch.int32, dev)
    tensor(_WHO, "tr_counts", tr_counts, (S, F), torch.int32, dev)
    tensor(_WHO, "gt", gt, (S, F, mg, 5), torch.float32, dev)
    tensor(_WHO, "gt_ids", gt_ids, (S, F, mg), torch.int32, dev)
    tensor(_WHO, "gt_counts", gt_counts, (S, F), torch.int32, dev)
    tensor(_WHO, "thr", thr, (None,), torch.float32, dev)
    if frames is not None:
        tensor(_WHO, "frames", frames, (S,), torch.int32, dev)
    nt = thr.shape[0]
    if out is None:
        out = (torch.empty((S, nt, len(COLUMNS)), dtype=torch.int64, device=dev),
               torch.empty((S, 2), dtype=torch.int32, device=dev))
    else:
        tensor(_WHO, "out counts", out[0], (S, nt, len(COLUMNS)), torch.int64, dev)
        tensor(_WHO, "out ignored", out[1], (S, 2), torch.int32, dev)
    tail = ()
    if dev.type == "cuda":
        if workspace is None:
            workspace = mot_workspace(S, nt, n_gt_ids, n_tr_ids, dev)
        tensor(_WHO, "workspace", workspace, (None,), torch.uint8, dev)
        tail = (workspace, workspace.numel())
    args = (tr, tr_ids, tr_counts, mo, gt, gt_ids, gt_counts, mg, S, F, frames, thr, nt, int(n_gt_ids), int(n_tr_ids),
            int(bool(class_aware)), out[0], out[1])
    run(_WHO, "mot_eval", dev, args, threads, device_tail=tail, keep=() if workspace is None else (workspace,))
    return out[0], out[1]


def ratios(counts):
    """MOTA, MOTP and IDF1 (float64, nan where nothing was there to count) of counts (..., 8)."""
    c = {k: counts[..., i].astype(np.float64) for i, k in enumerate(COLUMNS)}
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"mota": 1.0 - (c["fn"] + c["fp"] + c["idsw"]) / c["gt"],
                "motp": c["siou"] / (65535.0 * c["tp"]),
                "idf1": 2.0 * c["idtp"] / (c["gt"] + c["hyp"])}


HOTA_MAX_THR, HOTA_MAX_FRAMES = 32, 65535   # YH_HOTA_MAX_*
HOTA_COLUMNS = ("hota_tp", "hota_fp", "hota_fn", "loc", "assa_sum", "assre_sum", "asspr_sum", "pairs")
HOTA_THR = tuple(np.float32(k) * np.float32(0.05) for k in range(1, 20))
_HWHO = "yolo_hip.hota_eval"


def hota_workspace(sequences, num_thr, n_gt_ids, n_tr_ids, device="cpu"):
    """The workspace `hota_eval` needs on a cuda device (a uint8 tensor: the alignment sums and the
    matches of every threshold level over the identity pairs, and the counters)."""
    from ._lib import lib
    need = lib().yh_hota_workspace_bytes(int(sequences), int(num_thr), int(n_gt_ids), int(n_tr_ids))
    return torch.empty((need,), dtype=torch.uint8, device=device)


def hota_eval(tr, tr_ids, tr_counts, gt, gt_ids, gt_counts, n_gt_ids, n_tr_ids, thr=None, frames=None,
              class_aware=True, out=None, workspace=None, threads=0):
    """HOTA's integer counts (yh_hota_eval) on `mot_eval`'s tensors; thr (num_thr,) f32 in any order,
    None: 0.05, 0.10, ..., 0.95.
    -> (counts (S, num_thr, 8) int64: TP, FP, FN, LOC, ASSA, ASSRE, ASSPR, PAIRS; rows (S, 2) int64: the
    ground-truth and hypothesis rows that took part; ignored (S, 2) int32); out=(counts, rows, ignored)
    reuses buffers, every byte is written. cuda tensors run the kernels on the current stream
    (workspace: `hota_workspace`'s, allocated when not given), CPU tensors the host twin: the same
    bytes. Nothing is read back; `hota_ratios` turns the counts into scores."""
    if not isinstance(tr, torch.Tensor) or tr.dim() != 4 or not isinstance(gt, torch.Tensor) or gt.dim() != 4:
        raise ValueError(f"{_HWHO}: tr must be (S, F, max_out, 6) and gt (S, F, max_gt, 5)")
    dev = tr.device
    S, F, mo = tr.shape[:3]
    mg = gt.shape[2]
    if thr is None:
        thr = torch.tensor(HOTA_THR, dtype=torch.float32).to(dev)
    tensor(_HWHO, "tr", tr, (S, F, mo, 6), torch.float32, dev)
    tensor(_HWHO, "tr_ids", tr_ids, (S, F, mo), torch.int32, dev)
    tensor(_HWHO, "tr_counts", tr_counts, (S, F), torch.int32, dev)
    tensor(_HWHO, "gt", gt, (S, F, mg, 5), torch.float32, dev)
    tensor(_HWHO, "gt_ids", gt_ids, (S, F, mg), torch.int32, dev)
    tensor(_HWHO, "gt_counts", gt_counts, (S, F), torch.int32, dev)
    tensor(_HWHO, "thr", thr, (None,), torch.float32, dev)
    if frames is not None:
        tensor(_HWHO, "frames", frames, (S,), torch.int32, dev)
    nt = thr.shape[0]
    if out is None:
        out = (torch.empty((S, nt, len(HOTA_COLUMNS)), dtype=torch.int64, device=dev),
               torch.empty((S, 2), dtype=torch.int64, device=dev), torch.empty((S, 2), dtype=torch.int32, device=dev))
    else:
        tensor(_HWHO, "out counts", out[0], (S, nt, len(HOTA_COLUMNS)), torch.int64, dev)
        tensor(_HWHO, "out rows", out[1], (S, 2), torch.int64, dev)
        tensor(_HWHO, "out ignored", out[2], (S, 2), torch.int32, dev)
    tail = ()
    if dev.type == "cuda":
        if workspace is None:
            workspace = hota_workspace(S, nt, n_gt_ids, n_tr_ids, dev)
        tensor(_HWHO, "workspace", workspace, (None,), torch.uint8, dev)
        tail = (workspace, workspace.numel())
    args = (tr, tr_ids, tr_counts, mo, gt, gt_ids, gt_counts, mg, S, F, frames, thr, nt, int(n_gt_ids), int(n_tr_ids),
            int(bool(class_aware)), out[0], out[1], out[2])
    run(_HWHO, "hota_eval", dev, args, threads, device_tail=tail, keep=() if workspace is None else (workspace, thr))
    return out[0], out[1], out[2]


def hota_ratios(counts):
    """DetA, DetRe, DetPr, AssA, AssRe, AssPr, LocA and HOTA per threshold ("hota_alpha") and its mean
    over the thresholds ("hota"), float64, nan where nothing was matched, of counts (..., num_thr, 8)."""
    c = {k: counts[..., i].astype(np.float64) for i, k in enumerate(HOTA_COLUMNS)}
    tp, one = c["hota_tp"], float(1 << 20)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = {"deta": tp / (tp + c["hota_fn"] + c["hota_fp"]), "detre": tp / (tp + c["hota_fn"]),
             "detpr": tp / (tp + c["hota_fp"]), "assa": c["assa_sum"] / (one * tp), "assre": c["assre_sum"] / (one * tp),
             "asspr": c["asspr_sum"] / (one * tp), "loca": c["loc"] / (65536.0 * tp)}
        r["hota_alpha"] = np.sqrt(r["deta"] * r["assa"])
    r["hota"] = r["hota_alpha"].mean(axis=-1)
    return r


class TrackEvaluator:
    """Scores the tracks of `sequences` streams over up to `frames` frames against ground truth.

    update(tracks, gt, gt_ids, gt_counts, stream_ids=None) takes the `Tracks` of one `Tracker.update`
    (or any (dets, ids, ..., counts) of that layout) and the frame's ground truth - gt (B, max_gt, 5)
    f32 = x1, y1, x2, y2, class, gt_ids (B, max_gt) i32, gt_counts (B,) i32 - and files row b as the
    next frame of stream stream_ids[b] (None: stream b; a host sequence is checked, a device tensor
    is not read). It copies into preallocated buffers on the current stream and synchronises nothing.
    compute() launches yh_mot_eval once and returns a dict of numpy arrays: the counts "tp", "fp",
    "fn", "idsw", "siou", "idtp", "gt", "hyp" (sequences, thresholds) int64, "ignored" (sequences, 2),
    and "mota", "motp", "idf1" float64. It is the only call that reads the device.
    hota=True adds a yh_hota_eval launch on the same buffers at the thresholds hota_thr (None: 0.05 ..
    0.95) and the keys "hota_tp", "hota_fp", "hota_fn", "loc", "assa_sum", "assre_sum", "asspr_sum",
    "pairs" (sequences, hota thresholds) int64, "deta", "detre", "detpr", "assa", "assre", "asspr",
    "loca", "hota_alpha" float64 of that shape and "hota" (sequences,); without it the result is unchanged.
    Track ids at or above n_tr_ids (a `Tracker` numbers its tracks from 1 upwards) and ground-truth
    ids outside [0, n_gt_ids) are left out and reported in "ignored"."""

    def __init__(self, sequences, frames, thr=(0.5,), max_out=MAX_ROWS, max_gt=MAX_ROWS, n_gt_ids=MAX_IDS,
                 n_tr_ids=MAX_IDS, class_aware=True, device="cpu", threads=0, hota=False, hota_thr=None):
        who = "yolo_hip.TrackEvaluator"
        thr = [float(t) for t in thr]
        if not 1 <= len(thr) <= MAX_THR:
            raise ValueError(f"{who}: between 1 and {MAX_THR} thresholds")
        hota_thr = list(HOTA_THR) if hota_thr is None else [float(t) for t in hota_thr]
        if hota and not 1 <= len(hota_thr) <= HOTA_MAX_THR:
            raise ValueError(f"{who}: between 1 and {HOTA_MAX_THR} HOTA thresholds")
        if not 0 <= int(frames) <= MAX_FRAMES or sequences < 0:
            raise ValueError(f"{who}: frames must be in [0, {MAX_FRAMES}] and sequences >= 0")
        if not (0 <= max_out <= MAX_ROWS and 0 <= max_gt <= MAX_ROWS):
            raise ValueError(f"{who}: at most {MAX_ROWS} rows per frame on either side")
        if not (0 <= n_gt_ids <= MAX_IDS and 0 <= n_tr_ids <= MAX_IDS):
            raise ValueError(f"{who}: at most {MAX_IDS} identities on either side")
        self.device = torch.device(device)
        S, F = int(sequences), int(frames)
        self.n_gt_ids, self.n_tr_ids, self.class_aware, self.threads = int(n_gt_ids), int(n_tr_ids), bool(class_aware), threads
        z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=self.device)
        self.tr, self.tr_ids, self.tr_counts = z(S, F, max_out, 6, dtype=torch.float32), z(S, F, max_out), z(S, F)
        self.gt, self.gt_ids, self.gt_counts = z(S, F, max_gt, 5, dtype=torch.float32), z(S, F, max_gt), z(S, F)
        self.device = self.tr.device               # "cuda" has become "cuda:0": the device tensors report
        self.thr = torch.tensor(thr, dtype=torch.float32).to(self.device)
        self._cursor = z(S, dtype=torch.int64)     # the next frame of each stream
        self._calls = 0
        self._workspace = mot_workspace(S, len(thr), n_gt_ids, n_tr_ids, self.device) if self.device.type == "cuda" else None
        self.hota_thr = torch.tensor(hota_thr, dtype=torch.float32).to(self.device) if hota else None
        self._hota_workspace = (hota_workspace(S, len(hota_thr), n_gt_ids, n_tr_ids, self.device)
                                if hota and self.device.type == "cuda" else None)

    def reset(self):
        self._cursor.zero_()
        self._calls = 0

    def update(self, tracks, gt, gt_ids, gt_counts, stream_ids=None):
        who = "yolo_hip.TrackEvaluator"
        dets, ids, counts = tracks[0], tracks[1], tracks[-1]
        S, F, mo = self.tr.shape[:3]
        B = dets.shape[0]
        tensor(who, "tracks dets", dets, (B, mo, 6), torch.float32, self.device)
        tensor(who, "tracks ids", ids, (B, mo), torch.int32, self.device)
        tensor(who, "tracks counts", counts, (B,), torch.int32, self.device)
        tensor(who, "gt", gt, (B, self.gt.shape[2], 5), torch.float32, self.device)
        tensor(who, "gt_ids", gt_ids, (B, self.gt.shape[2]), torch.int32, self.device)
        tensor(who, "gt_counts", gt_counts, (B,), torch.int32, self.device)
        if self._calls >= F:     # a stream gets at most one frame per call: no cursor is beyond F - 1 here
            raise ValueError(f"{who}: more than {F} frames")
        if not isinstance(stream_ids, torch.Tensor):
            stream_ids = host_stream_ids(who, stream_ids, S, B, self.device, "rows")
        sid = torch.arange(B, device=self.device) if stream_ids is None else stream_ids.long()
        at = self._cursor[sid]
        for buf, src in ((self.tr, dets), (self.tr_ids, ids), (self.tr_counts, counts), (self.gt, gt),
                         (self.gt_ids, gt_ids), (self.gt_counts, gt_counts)):
            buf[sid, at] = src
        self._cursor[sid] = at + 1
        self._calls += 1

    def compute(self):
        frames = self._cursor.to(torch.int32)
        counts, ignored = mot_eval(self.tr, self.tr_ids, self.tr_counts, self.gt, self.gt_ids, self.gt_counts, self.thr,
                                   self.n_gt_ids, self.n_tr_ids, frames=frames,
                                   class_aware=self.class_aware, workspace=self._workspace, threads=self.threads)
        if self.hota_thr is not None:    # queued behind the first launch: one read of the device below
            hc = hota_eval(self.tr, self.tr_ids, self.tr_counts, self.gt, self.gt_ids, self.gt_counts, self.n_gt_ids,
                           self.n_tr_ids, thr=self.hota_thr, frames=frames, class_aware=self.class_aware,
                           workspace=self._hota_workspace, threads=self.threads)[0]
        counts = counts.cpu().numpy()
        res = {k: counts[..., i] for i, k in enumerate(COLUMNS)}
        res["ignored"] = ignored.cpu().numpy()
        res.update(ratios(counts))
        if self.hota_thr is not None:
            hc = hc.cpu().numpy()
            res.update({k: hc[..., i] for i, k in enumerate(HOTA_COLUMNS)})
            res.update(hota_ratios(hc))
        return res
