"""Second stage: a YOLO11-cls classifier over the crops of `crop_rois` (yh_classify).

    det = Detector(engine)                              # an Engine of nets.nn.yolo_v11_n(80)
    trk = Tracker(len(frames), device)
    cls = Classifier(nets.nn.yolo_v11_cls_n(10), device)
    d = det.predict(frames, keep_frames=True)
    t = trk.update(d)                                   # Tracks: dets (B, max_out, 6), ids (B, max_out)
    crops = crop_rois(d.frames, t.dets, t.counts, (128, 64))
    c = cls.predict(crops, embed=True)                  # Classified, one row per crop slot
    ids = crops.gather(t.ids)                           # (capacity,): the track id of every slot
    # slot i < total: track ids[i] has class c.top1[i] with confidence c.conf[i], embedding c.embed[i]

Everything stays on the device and on the current stream: `Crops.total` masks the rows beyond the
crops that exist without being read on the host.
"""
from typing import NamedTuple, Optional

import torch

from .engine import CLS_EMBED, Engine


class Classified(NamedTuple):
    """Result of `Classifier.predict`, one row per crop slot: probs (N, nc) f32, top1 (N,) i32 (-1 at
    or beyond total), conf (N,) f32 (the top-1 probability, 0 beyond total), embed (N, 1280) f32 or
    None, total (1,) i32. Rows at or beyond total are zero."""
    probs: torch.Tensor
    top1: torch.Tensor
    conf: torch.Tensor
    embed: Optional[torch.Tensor]
    total: torch.Tensor


class Classifier:
    """A nets.nn.YOLOCls on crops. On a cuda device the network runs on the HIP engine in `dtype`
    (crops go in as uint8, / 255 inside the stem); on the CPU device the torch module runs (there is
    no host twin of the network, as for the detector).

    N crops are processed in chunks of at most `max_batch`; a tail chunk runs at its own batch size,
    which costs the engine a second plan (tuning and a captured graph) - a `crop_rois` capacity that
    is a multiple of max_batch avoids it."""

    def __init__(self, model, device, dtype=torch.bfloat16, max_batch=256):
        self.device = torch.device(device)
        self.model = model.eval()
        self.dtype = dtype
        self.max_batch = int(max_batch)
        if self.max_batch < 1:
            raise ValueError("yolo_hip.Classifier: max_batch must be positive")
        self.num_classes = int(model._yh_arch[3])
        self.engine = None
        if self.device.type == "cuda":
            width, depth, csp, nc = model._yh_arch
            self.engine = Engine(width, depth, csp, nc, self.device, dtype, task="classify")
            self.engine.load_module(model)

    def predict(self, crops, embed=False):
        """crops: a `Crops` (its total masks the rows) or a (N, 3, h, w) tensor, uint8 RGB or the
        classifier's dtype in [0, 1]; h and w multiples of 32 -> Classified. Asynchronous on the
        current stream; nothing is read on the host."""
        data, total = (crops.data, crops.total) if hasattr(crops, "rois") else (crops, None)
        if not isinstance(data, torch.Tensor) or data.dim() != 4 or data.shape[1] != 3:
            raise ValueError("yolo_hip.Classifier: crops must be (N, 3, h, w)")
        dev = self.device
        if data.device != dev:
            data = data.to(dev, non_blocking=True)
        N, nc = data.shape[0], self.num_classes
        if total is None:
            total = torch.full((1,), N, dtype=torch.int32, device=dev)
        else:
            total = total.to(dev, non_blocking=True)
        probs = torch.empty((N, nc), dtype=torch.float32, device=dev)
        emb = torch.empty((N, CLS_EMBED), dtype=torch.float32, device=dev) if embed else None
        if dev.type == "cuda":
            stream = torch.cuda.current_stream(dev)
            with torch.cuda.device(dev):
                for s in range(0, N, self.max_batch):
                    n = min(self.max_batch, N - s)
                    count = (total - s).clamp_(0, n)
                    self.engine.classify(data[s:s + n], count=count, embed=embed,
                                         out=(probs[s:s + n], None, emb[s:s + n] if embed else None))
                    count.record_stream(stream)
            for t in (data, total):   # inputs made on another stream stay alive for the queued kernels
                t.record_stream(stream)
        else:
            mdt = next(self.model.parameters()).dtype
            x = data.to(mdt) / 255 if data.dtype == torch.uint8 else data.to(mdt)
            live = (torch.arange(N, device=dev) < total.clamp(0, N)).to(torch.float32)[:, None]
            with torch.no_grad():
                for s in range(0, N, self.max_batch):
                    p, _, e = self.model.features(x[s:s + self.max_batch])
                    probs[s:s + p.shape[0]] = p.float() * live[s:s + p.shape[0]]
                    if embed:
                        emb[s:s + p.shape[0]] = e.float() * live[s:s + p.shape[0]]
        if N == 0 or nc == 0:
            conf = torch.zeros((N,), dtype=torch.float32, device=dev)
            top1 = torch.full((N,), -1, dtype=torch.int32, device=dev)
        else:
            conf, idx = probs.max(1)
            valid = torch.arange(N, device=dev) < total.clamp(0, N)
            top1 = torch.where(valid, idx, torch.full_like(idx, -1)).to(torch.int32)
        return Classified(probs, top1, conf, emb, total)
