"""What the HOTA evaluation costs (yh_hota_eval, csrc/hota.hip), on one GPU.

  python tools/hota_bench.py [--out DIR] [--launches 20] [--trace]

tools/mot_bench.py's scenes (8 sequences of 600 frames with 64 and with 256 objects per frame, 5 %
misses, a trade every 50 frames) and one that fills the card (512 sequences of 150 frames, 64
objects), at HOTA's 19 thresholds:
 (a) yh_hota_eval per call (its four launches), HIP events;
 (b) the host twin (yh_hota_eval_host) on 16 threads on the same inputs, host clock;
 (c) yh_mot_eval on the same tensors at its 10 thresholds, HIP events.
Prints one JSON object and writes it to DIR/hota_bench.json (default: profiles). --trace only runs
the 8-sequence shapes' calls a few times, for a `rocprofv3 --kernel-trace --stats` run of its own. The
tool sets no time limit of its own: run it under `timeout`.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mot_bench  # noqa: E402
from yolo_hip import hota_eval, hota_workspace, mot_eval, mot_workspace  # noqa: E402

SHAPES = ((8, 600, 64), (8, 600, 256), (512, 150, 64))
COLUMNS = ("tp", "fp", "fn", "loc", "assa", "assre", "asspr", "pairs")


def events(n, call):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for x, y in ev:
        x.record()
        call()
        y.record()
    torch.cuda.synchronize()
    return mot_bench.stats([x.elapsed_time(y) * 1e3 for x, y in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(thresholds=19, device=torch.cuda.get_device_name(0), hota={}, hota_host_16_threads={}, mot_eval_10_thresholds={},
               counts={})
    for S, F, rows in SHAPES[:2] if a.trace else SHAPES:
        *args, mot_thr = mot_bench.scenes(rows, seed=rows, S=S, F=F)   # the seeds of tools/mot_bench.py
        dargs = [t.to(dev) for t in args]
        ws = hota_workspace(S, 19, rows, rows, dev)
        out = (torch.empty((S, 19, 8), dtype=torch.int64, device=dev), torch.empty((S, 2), dtype=torch.int64, device=dev),
               torch.empty((S, 2), dtype=torch.int32, device=dev))
        thr = torch.tensor([np.float32(k) * np.float32(0.05) for k in range(1, 20)], dtype=torch.float32, device=dev)
        call = lambda: hota_eval(*dargs, rows, rows, thr=thr, out=out, workspace=ws)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        if a.trace:
            continue
        key = f"{S}x{F}_frames_{rows}_rows"
        res["hota"][key] = events(a.launches, call)
        host_us = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = hota_eval(*args, rows, rows, threads=16)
            host_us.append((time.perf_counter() - t0) * 1e6)
        assert all(torch.equal(o.cpu(), w) for o, w in zip(out, want)), "device and host differ"
        res["hota_host_16_threads"][key] = mot_bench.stats(host_us)
        mws, mthr = mot_workspace(S, len(mot_thr), rows, rows, dev), mot_thr.to(dev)
        mcall = lambda: mot_eval(*dargs, mthr, rows, rows, workspace=mws)
        mcall()
        torch.cuda.synchronize()
        res["mot_eval_10_thresholds"][key] = events(max(3, a.launches // 4), mcall)
        res["counts"][key] = dict(zip(COLUMNS, want[0][0, 9].tolist()))   # sequence 0 at 0.5
    if a.trace:
        return
    line = json.dumps(res)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "hota_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
