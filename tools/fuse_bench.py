"""What the weighted boxes fusion costs (yh_fuse, csrc/fuse.hip), on one GPU.

  python tools/fuse_bench.py [--out DIR] [--launches 200] [--predicts 20]

 (a) yh_fuse per launch, HIP events: 32 images x 3 and x 8 groups of 300 rows each, on scenes whose
     300 objects per image are spread over 80 classes (every group sees every object, moved by a
     few pixels) and on the worst input, the same rows all of one class - one wave then walks the
     image's whole candidate list;
 (b) the host twin (yh_fuse_host) on 16 threads on the same inputs, host clock;
 (c) Detector.predict on 32 frames of 640 x 640 (v11_n bf16, synthetic weights, one engine), host
     clock around a device synchronise: tta=None against tta = plain + mirror + 0.83 scale.

Prints one JSON object and writes it to DIR/fuse_bench.json (default: profiles). The tool sets no
time limit of its own: run it under `timeout`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

from yolo_hip import fuse_boxes, synth  # noqa: E402
from yolo_hip.detect import Detector  # noqa: E402

N, ROWS, SIDE = 32, 300, 1920


def scenes(groups, classes, seed):
    """N images x `groups` groups x ROWS rows: every group sees the image's ROWS objects, each moved
    by up to 3 px, with a confidence near the object's. CPU tensors in fuse_boxes' order."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, SIDE - 200, size=(N, 1, ROWS, 2))
    wh = rng.uniform(20, 200, size=(N, 1, ROWS, 2))
    box = np.concatenate([xy, xy + wh], 3) + rng.uniform(-3, 3, size=(N, groups, ROWS, 4))
    score = np.clip(rng.uniform(0.05, 0.95, size=(N, 1, ROWS, 1)) + rng.uniform(-0.05, 0.05, size=(N, groups, ROWS, 1)), 0.01, 1)
    cls = np.broadcast_to(rng.integers(0, classes, size=(N, 1, ROWS, 1)), score.shape)
    dets = np.concatenate([box, score, cls], 3).astype(np.float32)
    order = np.argsort(-dets[..., 4], axis=2)                       # each group by confidence, as an NMS writes it
    dets = np.take_along_axis(dets, order[..., None], 2).reshape(N * groups, ROWS, 6)
    G = N * groups
    return (torch.from_numpy(dets), torch.full((G,), ROWS, dtype=torch.int32),
            torch.tensor([[1, 1, 0, 0, 0, 0]], dtype=torch.float32).repeat(G, 1), torch.ones(G),
            torch.arange(0, G + 1, groups, dtype=torch.int32), torch.full((N, 2), float(SIDE)))


def stats(us):
    us = sorted(us)
    return dict(n=len(us), median_us=round(us[len(us) // 2], 1), min_us=round(us[0], 1), p90_us=round(us[int(len(us) * 0.9)], 1))


def device_launches(args, groups, n):
    out = (torch.empty((N, 300, 6), device=args[0].device), torch.empty((N,), dtype=torch.int32, device=args[0].device))
    for _ in range(10):
        fuse_boxes(*args, groups, out=out)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fuse_boxes(*args, groups, out=out)
        b.record()
    torch.cuda.synchronize()
    return dict(stats([a.elapsed_time(b) * 1e3 for a, b in ev]), mean_clusters=round(out[1].float().mean().item(), 1))


def host_calls(args, groups, n):
    us = []
    for _ in range(n + 2):
        t0 = time.perf_counter()
        fuse_boxes(*args, groups, threads=16)
        us.append((time.perf_counter() - t0) * 1e6)
    return stats(us[2:])


def predicts(dev, n):
    from nets import nn
    from yolo_hip.engine import Engine
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    eng = Engine(*model._yh_arch, dev, torch.bfloat16)
    eng.load_module(model)
    x = synth.synth_scenes(N, 640, 640, seed=100)
    frames = [(f.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous().to(dev) for f in x]
    res = {}
    for name, tta in (("tta_none", None), ("tta_plain_mirror_083", ((1.0, False), (1.0, True), (0.83, False)))):
        det = Detector(eng, size=640, batch=N, tta=tta)
        ms = []
        for k in range(n + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = det.predict(frames)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[3:])
        res[name] = dict(n=n, median_ms=round(statistics.median(ms), 2), min_ms=round(ms[0], 2), max_ms=round(ms[-1], 2),
                         mean_detections=round(r.counts.float().mean().item(), 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--predicts", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(shape=f"{N} images, groups of {ROWS} rows, {SIDE} px", device=torch.cuda.get_device_name(0), fuse={}, host_16_threads={})
    for groups in (3, 8):
        for name, classes in (("80_classes", 80), ("one_class", 1)):
            args = scenes(groups, classes, seed=groups)
            key = f"{groups}_groups_{name}"
            res["fuse"][key] = device_launches([t.to(dev) for t in args], groups, a.launches)
            res["host_16_threads"][key] = host_calls(args, groups, 10)
    res["predict"] = predicts(dev, a.predicts)
    line = json.dumps(res)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "fuse_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
