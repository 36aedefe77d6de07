"""What the tracking evaluation costs (yh_mot_eval, csrc/mot.hip), on one GPU.

  python tools/mot_bench.py [--out DIR] [--launches 20]

8 sequences of 600 frames at 10 IoU thresholds (0.5 .. 0.95), with 64 and with 256 objects per
frame: every object is ground truth in every frame, the hypotheses are the objects moved by a few
pixels, a twentieth of them missing per frame, and now and then two tracks trade ids.
 (a) yh_mot_eval per launch, HIP events;
 (b) the host twin (yh_mot_eval_host) on 16 threads on the same inputs, host clock.
Prints one JSON object and writes it to DIR/mot_bench.json (default: profiles). The tool sets no
time limit of its own: run it under `timeout`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

from yolo_hip import mot_eval, mot_workspace  # noqa: E402

S, F = 8, 600
THR = np.linspace(0.5, 0.95, 10).astype(np.float32)


def scenes(rows, seed, S=S, F=F):
    rng = np.random.default_rng(seed)
    o = np.arange(rows)
    base = np.stack([70.0 * (o % 16), 90.0 * (o // 16)], 1)                   # neighbours overlap a little
    step = rng.uniform(-1, 1, (S, 1, rows, 2)) * np.arange(F)[None, :, None, None]
    xy = base[None, None] + step
    gt = np.concatenate([xy, xy + 80.0, np.broadcast_to((o % 3)[None, None, :, None], (S, F, rows, 1))], 3)
    jit = rng.uniform(-4, 4, (S, F, rows, 4))
    tr = np.concatenate([gt[..., :4] + jit, rng.uniform(0.3, 0.9, (S, F, rows, 1)), gt[..., 4:5]], 3)
    ids = np.broadcast_to(o, (S, F, rows)).copy()
    for s in range(S):                                                       # a trade every 50 frames
        for f in range(50, F, 50):
            a, b = rng.choice(rows, 2, replace=False)
            ids[s, f:, [a, b]] = ids[s, f:, [b, a]]
    keep = rng.random((S, F, rows)) >= 0.05                                   # the misses: the rest moves up
    order = np.argsort(~keep, axis=2, kind="stable")
    tr = np.take_along_axis(tr, order[..., None], 2)
    tr_ids = np.take_along_axis(ids, order, 2)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt)))
    return (t(tr, np.float32), t(tr_ids, np.int32), t(keep.sum(2), np.int32), t(gt, np.float32),
            t(np.broadcast_to(o, (S, F, rows)), np.int32), torch.full((S, F), rows, dtype=torch.int32), torch.from_numpy(THR))


def stats(us):
    us = sorted(us)
    return dict(n=len(us), median_us=round(us[len(us) // 2], 1), min_us=round(us[0], 1), max_us=round(us[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(shape=f"{S} sequences x {F} frames, {len(THR)} thresholds", device=torch.cuda.get_device_name(0),
               kernel={}, host_16_threads={}, counts={})
    for rows in (64, 256):
        args = scenes(rows, rows)
        t0 = time.perf_counter()
        want = mot_eval(*args, rows, rows, threads=16)
        host_us = [(time.perf_counter() - t0) * 1e6]
        for _ in range(2):
            t0 = time.perf_counter()
            mot_eval(*args, rows, rows, threads=16)
            host_us.append((time.perf_counter() - t0) * 1e6)
        dargs = [t.to(dev) for t in args]
        ws = mot_workspace(S, len(THR), rows, rows, dev)
        out = (torch.empty((S, len(THR), 8), dtype=torch.int64, device=dev), torch.empty((S, 2), dtype=torch.int32, device=dev))
        for _ in range(2):
            mot_eval(*dargs, rows, rows, out=out, workspace=ws)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for x, y in ev:
            x.record()
            mot_eval(*dargs, rows, rows, out=out, workspace=ws)
            y.record()
        torch.cuda.synchronize()
        assert torch.equal(out[0].cpu(), want[0]) and torch.equal(out[1].cpu(), want[1]), "device and host differ"
        key = f"{rows}_rows"
        res["kernel"][key] = stats([x.elapsed_time(y) * 1e3 for x, y in ev])
        res["host_16_threads"][key] = stats(host_us)
        res["counts"][key] = dict(zip(("tp", "fp", "fn", "idsw", "siou", "idtp", "gt", "hyp"), want[0][0, 0].tolist()))
    line = json.dumps(res)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "mot_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
