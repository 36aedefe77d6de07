"""Two handles on two devices in one process compute the same bits. Marked gpu; skipped on a
machine with one device.

The opt-in to more than 64 KB of dynamic LDS is a per-device function attribute, so every
(device, kernel) pair needs it (common.h lds_optin). Device 0 runs first: whatever a process-wide
"already set" state would remember is set by the time device 1 launches the same kernels. The
shapes: batch 2 at 96 x 160 (small maps, clipped tiles) and batch 1 at 640 x 640, the smallest at
which all three C3k blocks, the wide head_cls level, the pointwise chains and the whole-K/V
attention kernel run.
"""
import pytest
import torch

from _util import make_model
from yolo_hip import synth

pytestmark = pytest.mark.gpu


def test_second_device_equals_first(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    from yolo_hip.engine import Engine, nms
    dtype = torch.bfloat16
    model = make_model("n")
    engines = []
    for i in (0, 1):
        eng = Engine(*model._yh_arch, torch.device("cuda", i), dtype)
        eng.load_module(model)
        engines.append(eng)
    for batch, h, w in ((2, 96, 160), (1, 640, 640)):
        x = synth.synth_scenes(batch, h, w, seed=71)
        res = []
        for i, eng in enumerate(engines):   # device 0 first
            dev = torch.device("cuda", i)
            with torch.cuda.device(dev):
                y = eng.forward(x.to(dev, dtype)).clone()
                dets, counts = nms(y)
                torch.cuda.synchronize(dev)
            res.append((y.cpu(), dets.cpu(), counts.cpu()))
        if (batch, h, w) == (1, 640, 640):
            cls = [u["cls"] for u in engines[1].units(batch, h, w)]
            assert cls.count("c3k") == 3 and "head_cls" in cls and "pw_chain" in cls, cls
        (y0, d0, c0), (y1, d1, c1) = res
        assert torch.isfinite(y0.float()).all()
        assert torch.equal(y0, y1), (y0.float() - y1.float()).abs().max().item()
        assert torch.equal(c0, c1), (c0.tolist(), c1.tolist())
        for b, n in enumerate(c0.tolist()):
            assert torch.equal(d0[b, :n], d1[b, :n]), b
