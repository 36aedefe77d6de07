"""yh_match (csrc/match.hip) and yolo_hip.evaluate.Evaluator on the device. Marked gpu.

* The golden set and the random case list of tests/_match_cases.py on the device,
  against compute_metric per image on the device and against yh_match_host on the
  copied inputs, both exactly. The padding rows of dets are NaN in one run and
  duplicates of valid rows in the other; the output buffers are pre-filled.
* Evaluator against main.py's per-image loop (the setup of test_gpu_eval_loop.py).
* Evaluator as DetectPipeline's `post` with result_ring=True, never reading dets, for
  both nms_on_lane values, against sequential forward + nms + compute_metric.
"""
import numpy as np
import pytest
import torch

import _match_cases as mc
from yolo_hip import synth
from yolo_hip.metrics import compute_ap, compute_metric, match_batch

pytestmark = pytest.mark.gpu


def _device_run(c, gpu, padding):
    B, md = c["dets"].shape[:2]
    T = c["iou_v"].shape[0]
    dets = c["dets"].clone()
    if padding == "nan":
        beyond = torch.arange(md)[None, :] >= c["counts"].clamp(0, md)[:, None]
        dets[beyond] = float("nan")
    on = {k: c[k].to(gpu) for k in ("counts", "labels", "offsets", "iou_v")}
    tp = torch.full((B, md, T), 0xFF, dtype=torch.uint8, device=gpu)
    sc = torch.full((B, md, 2), -7.0, device=gpu)
    co = torch.full((B,), -7, dtype=torch.int32, device=gpu)
    got = match_batch(dets.to(gpu), on["counts"], on["labels"], on["offsets"], on["iou_v"], out=tp, score_cls=sc,
                      counts_out=co)
    assert got is tp
    return tp.cpu(), sc.cpu(), co.cpu()


@pytest.mark.parametrize("name", mc.ALL)
def test_match_device_equals_compute_metric_and_host(gpu, name):
    c = mc.case(name)
    md = c["dets"].shape[1]
    host_tp = match_batch(c["dets"], c["counts"], c["labels"], c["offsets"], c["iou_v"])
    dev_oracle = mc.oracle_on(c, gpu)
    cnt = c["counts"].clamp(0, md)
    valid = torch.arange(md)[None, :] < cnt[:, None]
    want_sc = torch.where(valid[..., None], c["dets"][:, :, 4:6], torch.zeros(()))
    for padding in ("nan", "dup"):
        tp, sc, co = _device_run(c, gpu, padding)
        assert np.array_equal(tp.numpy(), dev_oracle.numpy()), padding
        assert np.array_equal(tp.numpy(), host_tp.numpy()), padding
        assert np.array_equal(tp.numpy(), c["want"].numpy()), padding
        assert torch.equal(sc, want_sc) and torch.equal(co, cnt), padding


def test_match_device_argument_errors(gpu):
    c = mc.case("t10_b33_float")
    on = {k: c[k].to(gpu) for k in ("dets", "counts", "labels", "offsets", "iou_v")}
    with pytest.raises(RuntimeError, match="num_iou"):
        match_batch(on["dets"], on["counts"], on["labels"], on["offsets"], torch.zeros((33,), device=gpu))
    with pytest.raises(ValueError, match="contiguous"):
        match_batch(on["dets"], torch.zeros((66,), dtype=torch.int32, device=gpu)[::2], on["labels"], on["offsets"],
                    on["iou_v"])
    with pytest.raises(ValueError):          # mixed devices
        match_batch(on["dets"], c["counts"], on["labels"], on["offsets"], on["iou_v"])


# ---------------------------------------------------------------------------- Evaluator
def _model():
    from nets import nn
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    return model.eval()


def _engine(model, gpu):
    from yolo_hip.engine import Engine
    eng = Engine(*model._yh_arch, gpu, torch.float16)
    eng.load_module(model)
    return eng


def _synthetic_targets(dets, counts, S, g):
    """main.py's collated CPU targets: jittered copies of up to 5 detections per image."""
    cls, box, idx = [], [], []
    for i, k in enumerate(counts.tolist()):
        k = min(5, k)
        c = dets[i, :k, :4].cpu() + torch.randn((k, 4), generator=g) * 2.0
        cls.append(dets[i, :k, 5:6].cpu())
        box.append(torch.stack(((c[:, 0] + c[:, 2]) / 2 / S, (c[:, 1] + c[:, 3]) / 2 / S,
                                (c[:, 2] - c[:, 0]) / S, (c[:, 3] - c[:, 1]) / S), 1))
        idx.append(torch.full((k,), float(i)))
    return {"cls": torch.cat(cls), "box": torch.cat(box), "idx": torch.cat(idx)}


def _loop(batches, S, gpu):
    """main.py:264-297 for [(dets, counts, targets)]: the per-image tuples, concatenated."""
    from utils import util
    iou_v = torch.linspace(0.5, 0.95, 10).to(gpu)
    scale = torch.tensor((S, S, S, S)).to(gpu)
    metrics = []
    for dets, counts, targets in batches:
        for i, k in enumerate(counts.tolist()):
            output = dets[i, :k]
            sel = targets["idx"] == i
            cls, box = targets["cls"][sel].to(gpu), targets["box"][sel].to(gpu)
            metric = torch.zeros(output.shape[0], 10, dtype=torch.bool).to(gpu)
            if output.shape[0] == 0:
                if cls.shape[0]:
                    metrics.append((metric, *torch.zeros((2, 0)).to(gpu), cls.squeeze(-1)))
                continue
            if cls.shape[0]:
                target = torch.cat((cls, util.wh2xy(box) * scale), 1)
                metric = compute_metric(output[:, :6], target, iou_v)
            metrics.append((metric, output[:, 4], output[:, 5], cls.squeeze(-1)))
    return [torch.cat(x, 0) for x in zip(*metrics)]


def _same(got, want):
    for g, w in zip(got, want):
        assert g.device == w.device and g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


def test_evaluator_equals_the_reference_eval_loop(gpu):
    from yolo_hip import Evaluator
    from yolo_hip.engine import nms
    B, S = 4, 320
    eng = _engine(_model(), gpu)
    scenes = synth.synth_scenes(B, S, S, seed=21)
    samples = (scenes * 255).round().clamp(0, 255).to(torch.uint8).to(gpu)
    dets, counts = nms(eng.forward(samples))
    counts_h = counts.cpu()
    targets = _synthetic_targets(dets, counts_h, S, torch.Generator().manual_seed(3))
    want = _loop([(dets, counts_h, targets)], S, gpu)
    assert want[0].any()                                           # the jittered labels are found

    ev = Evaluator(gpu)
    ev.update(dets, counts, targets, (S, S))
    _same(ev.metrics(), want)
    ref = compute_ap(*want)
    got = ev.result()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and tuple(got[2:]) == tuple(ref[2:])

    on_dev = Evaluator(gpu)                                        # targets already on the device
    on_dev.update(dets, counts, {k: v.to(gpu) for k, v in targets.items()}, (S, S))
    _same(on_dev.metrics(), want)


@pytest.mark.parametrize("nms_on_lane", [False, True])
def test_evaluator_as_pipeline_post_with_result_ring(gpu, nms_on_lane):
    from yolo_hip import Evaluator
    from yolo_hip.engine import nms
    from yolo_hip.pipeline import DetectPipeline
    B, S, N = 2, 256, 6
    model = _model()
    lanes = [_engine(model, gpu), _engine(model, gpu)]
    xs = [synth.synth_scenes(B, S, S, seed=400 + i).to(gpu, torch.float16) for i in range(N)]
    g = torch.Generator().manual_seed(9)
    seq = []
    for x in xs:                                                   # sequential forward + nms
        d, c = nms(lanes[0].forward(x))
        c = c.cpu()
        seq.append((d, c, _synthetic_targets(d, c, S, g)))
    want = _loop(seq, S, gpu)
    assert want[0].any()

    ev = Evaluator(gpu)
    pipe = DetectPipeline(lanes, B, S, S, post=ev.post, nms_on_lane=nms_on_lane, result_ring=True)
    assert len(pipe.dets) < N                                      # later batches overwrite earlier slots
    for x, (_, _, targets) in zip(xs, seq):
        ev.stage(targets, (S, S))
        pipe.submit(x)                                             # dets / counts are never read here
    pipe.drain()
    assert ev.images == B * N
    _same(ev.metrics(), want)
    ref = compute_ap(*want)
    got = ev.result()
    assert tuple(got[2:]) == tuple(ref[2:])
