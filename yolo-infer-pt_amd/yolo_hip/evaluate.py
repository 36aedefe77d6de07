"""Batched mAP evaluation that keeps up with the detection pipeline.

main.py:test (264-304) evaluates one image at a time: after the NMS it slices the
batch's targets per image, calls compute_metric on each (a chain of small launches)
and concatenates everything for compute_ap. `Evaluator` is the same evaluation for
whole batches: one yh_match launch (csrc/match.hip) per batch matches every
image's detections to its labels, straight from the fixed-size NMS output
dets (B, max_det, 6) / counts (B,), and writes the true-positive bytes, the
(score, class) pairs and the clamped counts into storage the evaluator owns. The
NMS buffers are not referenced afterwards, so a DetectPipeline result ring may
overwrite them.

    ev = Evaluator(device)
    pipe = DetectPipeline(engines, B, H, W, post=ev.post, result_ring=True)
    for x, targets in loader:
        ev.stage(targets, (H, W))     # before the submit it belongs to
        pipe.submit(x)
    pipe.drain()                      # metrics() / result() read on the caller's stream
    m_pre, m_rec, map50, mean_ap = ev.result()[2:]

update() / stage() / post() never synchronise the host with the device: no
.item(), no .tolist(), no boolean-mask indexing of device tensors. Everything of
data-dependent size happens in metrics(), the one place that compacts.
"""
from collections import deque

import numpy
import torch

from .metrics import compute_ap, match_batch


class Evaluator:
    """Accumulates the eval loop's per-detection records for a dataset, on `device`.

    device: where the detections live ("cuda:0": yh_match on the current stream; "cpu":
    yh_match_host). max_det: the NMS's max_det (the middle dimension of dets).
    iou_v: (T,) thresholds, default main.py:255's linspace(0.5, 0.95, 10).
    chunk_images: images per storage block; a new block is allocated when the next
    batch does not fit (a batch never straddles two blocks, so it is one launch).
    """

    def __init__(self, device, max_det=300, iou_v=None, chunk_images=4096):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_det = int(max_det)
        if iou_v is None:
            iou_v = torch.linspace(0.5, 0.95, 10)
        self.iou_v = torch.as_tensor(iou_v, dtype=torch.float32).to(self.device).contiguous()
        if self.iou_v.dim() != 1 or not 1 <= self.iou_v.shape[0] <= 32:
            raise ValueError("yolo_hip.Evaluator: iou_v must hold 1..32 thresholds")
        self.chunk_images = int(chunk_images)
        if self.chunk_images < 1:
            raise ValueError("yolo_hip.Evaluator: chunk_images must be positive")
        self.reset()

    def reset(self):
        self._chunks = []          # [tp (n, max_det, T) u8, score_cls (n, max_det, 2) f32, counts (n,) i32, used]
        self._targets = []         # per update: (label classes (N,), keep mask (N,)) on the device
        self._staged = deque()     # stage() -> post(), submission order
        self._merged = None        # gather()'s result
        self._marked = set()       # (tensor, stream) pairs metrics() has record_stream'ed
        self.images = 0

    # ------------------------------------------------------------------ labels
    def _labels(self, targets, hw, batch):
        """main.py:276-291 for the whole batch: -> (labels (N, 5), offsets (batch + 1,) i32,
        keep (N,) bool) on self.device, labels sorted stably by image index. `keep` marks the
        labels of images 0 .. batch - 1. No host sync."""
        h, w = int(hw[0]), int(hw[1])
        cls, box, idx = targets["cls"], targets["box"], targets["idx"]
        src = cls.device
        n = cls.shape[0]
        cls = cls.reshape(n, 1).to(torch.float32)
        box = box.reshape(n, 4).to(torch.float32)
        idx = idx.reshape(n).to(torch.int64)
        order = torch.argsort(idx, stable=True)
        idx, cls, box = idx[order], cls[order], box[order]
        # util.wh2xy(box) * scale, elementwise in fp32 (main.py:269, 291)
        half_w, half_h = box[:, 2] / 2, box[:, 3] / 2
        # (the scale is applied per column as a Python scalar: a device tensor made from a tuple
        # would be a synchronous upload; the products are the same fp32 values)
        corners = torch.stack(((box[:, 0] - half_w) * w, (box[:, 1] - half_h) * h,
                               (box[:, 0] + half_w) * w, (box[:, 1] + half_h) * h), 1)
        offsets = torch.searchsorted(idx, torch.arange(batch + 1, device=src)).to(torch.int32)
        keep = (idx >= 0) & (idx < batch)
        if src == self.device:
            return torch.cat((cls, corners), 1).contiguous(), offsets, keep
        # one staging buffer, one copy: [labels N x 5 f32 | offsets (batch + 1) i32 | keep N as i32].
        # Pinned staging comes from torch's caching host allocator, which hands a block out again
        # only after the copies queued from it have run: nothing here rewrites a buffer in flight.
        pin = self.device.type == "cuda" and src.type == "cpu"
        stage = torch.empty(5 * n + batch + 1 + n, dtype=torch.float32, pin_memory=pin)
        stage[:5 * n].view(n, 5).copy_(torch.cat((cls, corners), 1))
        stage[5 * n:5 * n + batch + 1].view(torch.int32).copy_(offsets)
        stage[5 * n + batch + 1:].view(torch.int32).copy_(keep)
        on = stage.to(self.device, non_blocking=True)
        return (on[:5 * n].view(n, 5), on[5 * n:5 * n + batch + 1].view(torch.int32),
                on[5 * n + batch + 1:].view(torch.int32) != 0)

    # ------------------------------------------------------------------ accumulate
    def update(self, dets, counts, targets, hw, valid=None):
        """One batch: dets (B, max_det, 6) f32 / counts (B,) i32 as `nms` returns them (on
        self.device), targets = main.py's dict {'cls' (N, 1), 'box' (N, 4) normalised cxcywh,
        'idx' (N,) image index in the batch} on the CPU or the device, hw = (height, width) of
        the network input. valid: only the first `valid` images count (a padded last batch).
        Runs on the current stream; never synchronises."""
        if dets.dim() != 3 or dets.shape[1] != self.max_det:
            raise ValueError(f"yolo_hip.Evaluator: dets must be (B, {self.max_det}, 6), got {tuple(dets.shape)}")
        B = dets.shape[0]
        nb = B if valid is None else int(valid)
        if not 0 <= nb <= B:
            raise ValueError(f"yolo_hip.Evaluator: valid={valid} outside [0, {B}]")
        self._merged = None
        if nb == 0:
            return
        labels, offsets, keep = self._labels(targets, hw, nb)
        if not self._chunks or self._chunks[-1][3] + nb > self._chunks[-1][0].shape[0]:
            n = max(self.chunk_images, nb)
            T = self.iou_v.shape[0]
            self._chunks.append([torch.empty((n, self.max_det, T), dtype=torch.uint8, device=self.device),
                                 torch.empty((n, self.max_det, 2), dtype=torch.float32, device=self.device),
                                 torch.empty((n,), dtype=torch.int32, device=self.device), 0])
        chunk = self._chunks[-1]
        at = chunk[3]
        # With nms_on_lane=True successive updates run on different lane streams and write into a
        # block allocated on whichever stream came first. That is safe because the block stays
        # referenced here (the allocator never hands it out again) and each update writes its own
        # slice [at, at + nb), disjoint from every other's.
        match_batch(dets[:nb], counts[:nb], labels, offsets, self.iou_v, out=chunk[0][at:at + nb],
                    score_cls=chunk[1][at:at + nb], counts_out=chunk[2][at:at + nb])
        chunk[3] = at + nb
        self._targets.append((labels[:, 0], keep))
        self.images += nb

    # ------------------------------------------------------------------ DetectPipeline hook
    def stage(self, targets, hw, valid=None):
        """Queue the labels of the batch the next pipe.submit(x) carries. Call it before each
        submit; post() consumes the queue in submission order."""
        ready = None
        if self.device.type == "cuda" and any(t.is_cuda for t in targets.values()):
            ready = torch.cuda.Event()     # device-side targets: whatever produced them comes first
            ready.record(torch.cuda.current_stream(self.device))
        self._staged.append((targets, hw, valid, ready))

    def post(self, dets, counts):
        """DetectPipeline(post=ev.post): called on the NMS stream right after each batch's NMS.
        Uploads the staged labels and matches the batch there, so the ring's dets / counts are
        consumed before a later batch's NMS can overwrite them. Returns None."""
        if not self._staged:
            raise RuntimeError("yolo_hip.Evaluator.post: no staged targets - call stage() before each submit()")
        targets, hw, valid, ready = self._staged.popleft()
        if ready is not None:
            ns = torch.cuda.current_stream(self.device)
            ns.wait_event(ready)
            for t in targets.values():
                if t.is_cuda:
                    t.record_stream(ns)
        self.update(dets, counts, targets, hw, valid)
        return None

    # ------------------------------------------------------------------ results
    def metrics(self):
        """-> (tp (n, T) bool, conf (n,), cls (n,), target_cls (m,)) on self.device: what
        main.py:297 concatenates - image-major, then detection order; an image without
        detections still contributes its label classes. After gather(): the merged tensors.

        Reads on the current stream: with a DetectPipeline call pipe.drain() first (the
        updates ran on its NMS stream)."""
        if self._merged is not None:
            return self._merged
        T = self.iou_v.shape[0]
        tps, confs, clss = [], [], []
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None

        def mark(t):    # allocated on the stream of an update, read on this one; once per tensor and stream
            key = (t.data_ptr(), cur.cuda_stream)
            if key not in self._marked:
                self._marked.add(key)
                t.record_stream(cur)

        for tp, sc, cnt, used in self._chunks:
            if cur is not None:
                for t in (tp, sc, cnt):
                    mark(t)
            mask = torch.arange(self.max_det, device=self.device)[None, :] < cnt[:used, None]
            tps.append(tp[:used][mask].to(torch.bool))
            confs.append(sc[:used, :, 0][mask])
            clss.append(sc[:used, :, 1][mask])
        if cur is not None:
            for c, k in self._targets:
                mark(c)
                mark(k)
        tgt = [c[k] for c, k in self._targets]
        f32 = dict(dtype=torch.float32, device=self.device)
        return (torch.cat(tps, 0) if tps else torch.zeros((0, T), dtype=torch.bool, device=self.device),
                torch.cat(confs, 0) if confs else torch.zeros((0,), **f32),
                torch.cat(clss, 0) if clss else torch.zeros((0,), **f32),
                torch.cat(tgt, 0) if tgt else torch.zeros((0,), **f32))

    def result(self, plot=False, names=(), save_dir="./weights"):
        """main.py:298-304: compute_ap over metrics() when any true positive exists ->
        (tp, fp, m_pre, m_rec, map50, mean_ap); otherwise the four scalars are 0 (and the
        per-class arrays empty). Needs pipe.drain() first, like metrics()."""
        tp, conf, cls, tgt = self.metrics()
        if tp.shape[0] and bool(tp.any()):
            return compute_ap(tp, conf, cls, tgt, plot=plot, names=names, save_dir=save_dir)
        return numpy.zeros(0), numpy.zeros(0), 0.0, 0.0, 0.0, 0.0

    def gather(self, group=None):
        """Data-parallel merge: every rank's metrics() tensors, padded to a common length,
        all_gather'ed and concatenated in rank order; afterwards metrics() / result() on every
        rank describe the whole dataset. With yolo_hip.dist.shard's contiguous image ranges rank
        order is dataset order, so the result equals a single-process run. Works with gloo
        (device "cpu") and nccl (device "cuda"). A later update() drops the merged state."""
        import torch.distributed as td
        self._merged = None
        tp, conf, cls, tgt = self.metrics()
        if not (td.is_available() and td.is_initialized()) or td.get_world_size(group) == 1:
            self._merged = (tp, conf, cls, tgt)
            return self._merged
        world = td.get_world_size(group)
        T = self.iou_v.shape[0]
        lens = torch.tensor([tp.shape[0], tgt.shape[0]], dtype=torch.int64, device=self.device)
        all_lens = [torch.zeros_like(lens) for _ in range(world)]
        td.all_gather(all_lens, lens, group=group)
        all_lens = [x.tolist() for x in all_lens]
        n_max = max(x[0] for x in all_lens)
        m_max = max(x[1] for x in all_lens)

        def exchange(t, length, dtype):
            pad = torch.zeros((length,) + tuple(t.shape[1:]), dtype=dtype, device=self.device)
            pad[:t.shape[0]] = t.to(dtype)
            got = [torch.empty_like(pad) for _ in range(world)]
            td.all_gather(got, pad, group=group)
            return got

        tps = exchange(tp.reshape(-1, T), n_max, torch.uint8)
        confs = exchange(conf, n_max, torch.float32)
        clss = exchange(cls, n_max, torch.float32)
        tgts = exchange(tgt, m_max, torch.float32)
        self._merged = (torch.cat([t[:x[0]] for t, x in zip(tps, all_lens)], 0).to(torch.bool),
                        torch.cat([t[:x[0]] for t, x in zip(confs, all_lens)], 0),
                        torch.cat([t[:x[0]] for t, x in zip(clss, all_lens)], 0),
                        torch.cat([t[:x[1]] for t, x in zip(tgts, all_lens)], 0))
        return self._merged
