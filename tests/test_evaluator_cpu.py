"""yolo_hip.evaluate.Evaluator on the CPU device (yh_match_host) over the reference's
golden detection set (tests/golden/metrics_synth.npz), against main.py's per-image loop
as tests/test_metrics.py::_run restates it, and its gloo rank merge.

The golden stores label corners in pixels; the evaluator takes main.py's normalised
cxcywh targets and converts them as main.py:291 does (wh2xy(box) * scale, fp32). That
round trip moves a corner by an ulp, so the oracle loop here runs compute_metric on the
labels converted by the reference's own formula (utils.util.wh2xy), and the end result
is checked against the golden's AP numbers as well.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import load_golden
from utils import util
from yolo_hip import Evaluator, dist
from yolo_hip.metrics import compute_ap, compute_metric

MD, H, W = 32, 640, 640


def _images(lo=0, hi=None):
    g = load_golden("metrics_synth.npz")
    hi = int(g["n_img"]) if hi is None else hi
    return [(torch.from_numpy(g[f"out_{i}"]), torch.from_numpy(g[f"tgt_{i}"]).reshape(-1, 5)) for i in range(lo, hi)]


def _targets(tgts):
    """main.py's collated targets of one batch from pixel-corner labels."""
    cls = torch.cat([t[:, 0:1] for t in tgts], 0)
    c = torch.cat([t[:, 1:5] for t in tgts], 0)
    box = torch.stack(((c[:, 0] + c[:, 2]) / 2 / W, (c[:, 1] + c[:, 3]) / 2 / H,
                       (c[:, 2] - c[:, 0]) / W, (c[:, 3] - c[:, 1]) / H), 1)
    idx = torch.cat([torch.full((len(t),), float(i)) for i, t in enumerate(tgts)], 0)
    return {"cls": cls, "box": box, "idx": idx}


def _batches(images, per, shuffle_seed=None):
    """-> [(dets (per, MD, 6), counts (per,), targets, valid)], the last batch padded."""
    out = []
    for s in range(0, len(images), per):
        part = images[s:s + per]
        dets = torch.full((per, MD, 6), float("nan"))
        counts = torch.full((per,), 7, dtype=torch.int32)           # padding images claim detections
        for i, (o, _) in enumerate(part):
            dets[i, :len(o)] = o
            counts[i] = len(o)
        t = _targets([x[1] for x in part])
        if shuffle_seed is not None:
            # interleave the images' labels; each image's own labels keep their order (the tie rule
            # and target_cls follow the label order within an image)
            perm = torch.randperm(len(t["idx"]), generator=torch.Generator().manual_seed(shuffle_seed + s))
            pos = torch.argsort(t["idx"][perm], stable=True)
            mixed = {k: torch.empty_like(v) for k, v in t.items()}
            for k, v in t.items():
                mixed[k][pos] = v
            assert len(part) < 2 or not torch.equal(mixed["idx"], t["idx"])
            t = mixed
        out.append((dets, counts, t, len(part)))
    return out


def _loop(images):
    """main.py:275-297 on the labels as main.py:291 converts them."""
    iou_v = torch.linspace(0.5, 0.95, 10)
    scale = torch.tensor((W, H, W, H))
    metrics = []
    for out, tgt in images:
        t = _targets([tgt])
        cls, box = t["cls"], t["box"]
        metric = torch.zeros(out.shape[0], 10, dtype=torch.bool)
        if out.shape[0] == 0:
            if cls.shape[0]:
                metrics.append((metric, *torch.zeros((2, 0)), cls.squeeze(-1)))
            continue
        if cls.shape[0]:
            target = torch.cat((cls, util.wh2xy(box) * scale), 1)
            metric = compute_metric(out[:, :6], target, iou_v)
        metrics.append((metric, out[:, 4], out[:, 5], cls.squeeze(-1)))
    return [torch.cat(x, 0) for x in zip(*metrics)]


def _feed(ev, batches):
    for dets, counts, t, valid in batches:
        ev.update(dets, counts, t, (H, W), valid=valid)
    return ev


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


@pytest.fixture(scope="module")
def want():
    return _loop(_images())


def test_metrics_equal_the_per_image_loop(want):
    ev = _feed(Evaluator("cpu", max_det=MD), _batches(_images(), 5))      # 24 = 4 x 5 + 4: valid = 4
    assert ev.images == 24
    _same(ev.metrics(), want)


def test_metrics_equal_the_loop_of_test_metrics_run():
    """What tests/test_metrics.py::_run concatenates, from the golden's own pixel-corner labels and
    the reference's `correct_i`: the one-ulp label round trip flips no threshold decision."""
    g = load_golden("metrics_synth.npz")
    metrics = []
    for i, (out, tgt) in enumerate(_images()):
        if out.shape[0] == 0:
            if tgt.shape[0]:
                metrics.append((torch.zeros((0, 10), dtype=torch.bool), *torch.zeros((2, 0)), tgt[:, 0]))
            continue
        metrics.append((torch.from_numpy(g[f"correct_{i}"]), out[:, 4], out[:, 5], tgt[:, 0]))
    ev = _feed(Evaluator("cpu", max_det=MD), _batches(_images(), 5))
    _same(ev.metrics(), [torch.cat(x, 0) for x in zip(*metrics)])


def test_result_reproduces_the_golden_ap(want):
    g = load_golden("metrics_synth.npz")
    ev = _feed(Evaluator("cpu", max_det=MD, chunk_images=7), _batches(_images(), 5))   # several storage blocks
    tp, fp, m_pre, m_rec, map50, mean_ap = ev.result()
    assert np.array_equal(tp, g["ap_tp"]) and np.array_equal(fp, g["ap_fp"])
    np.testing.assert_allclose([m_pre, m_rec, map50, mean_ap], g["ap_scalars"], rtol=0, atol=1e-12)
    ref = compute_ap(*want)
    assert np.array_equal(tp, ref[0]) and np.array_equal(fp, ref[1]) and (m_pre, m_rec, map50, mean_ap) == ref[2:]


def test_unsorted_idx_gives_the_same(want):
    ev = _feed(Evaluator("cpu", max_det=MD), _batches(_images(), 5, shuffle_seed=4))
    _same(ev.metrics(), want)


def test_stage_and_post_consume_in_submission_order(want):
    ev = Evaluator("cpu", max_det=MD)
    batches = _batches(_images(), 5)
    for _, _, t, valid in batches[:2]:
        ev.stage(t, (H, W), valid)
    for dets, counts, _, _ in batches[:2]:
        assert ev.post(dets, counts) is None
    for dets, counts, t, valid in batches[2:]:
        ev.stage(t, (H, W), valid)
        ev.post(dets, counts)
    _same(ev.metrics(), want)
    with pytest.raises(RuntimeError, match="stage"):
        ev.post(batches[0][0], batches[0][1])


def test_all_miss_dataset_gives_zeros():
    images = [(o, torch.cat((t[:, :1] + 100.0, t[:, 1:]), 1)) for o, t in _images()]     # no class ever matches
    ev = _feed(Evaluator("cpu", max_det=MD), _batches(images, 5))
    tp, conf, cls, tgt = ev.metrics()
    assert tp.shape[0] == sum(len(o) for o, _ in images) and not tp.any()
    assert tgt.shape[0] == sum(len(t) for _, t in images)
    assert ev.result()[2:] == (0.0, 0.0, 0.0, 0.0)
    assert Evaluator("cpu", max_det=MD).result()[2:] == (0.0, 0.0, 0.0, 0.0)


def test_exported_from_the_package():
    import yolo_hip
    from yolo_hip.evaluate import Evaluator as E
    assert yolo_hip.Evaluator is E


# ---------------------------------------------------------------------------- gather, gloo world 2
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = dist.shard(24, rank, world)                        # 12 / 12, contiguous
        ev = _feed(Evaluator("cpu", max_det=MD), _batches(_images(lo, hi), 5))
        merged = ev.gather()
        torch.save(dict(metrics=[t.clone() for t in merged], same=all(a is b for a, b in zip(merged, ev.metrics())),
                        result=ev.result()), os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        torch.distributed.destroy_process_group()


def test_gather_world2_gloo_equals_single_process(tmp_path, want):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = compute_ap(*want)
    for rank in range(2):
        got = torch.load(str(tmp_path / f"rank{rank}.pt"), weights_only=False)
        _same(got["metrics"], want)
        assert got["same"]
        r = got["result"]
        assert np.array_equal(r[0], single[0]) and np.array_equal(r[1], single[1]) and tuple(r[2:]) == single[2:]


def test_gather_without_process_group_is_the_local_result(want):
    ev = _feed(Evaluator("cpu", max_det=MD), _batches(_images(), 5))
    _same(ev.gather(), want)
