"""What source-coordinate detections and tiled inference cost (yolo_hip.detect), v11_n bf16.

  python tools/detect_bench.py [--out DIR] [--launches 200] [--repeats 3] [--calls 12]

 (a) yh_merge alone, HIP events per launch, median: the worst case (8 images of
     MERGE_MAX_CAND candidates each, no two boxes overlapping; with max_out 300 and with
     max_out = MERGE_MAX_CAND, i.e. the whole walk) and a typical one (8 images x 16 tiles x
     ~40 rows, every object seen by about two tiles);
 (b) the merge kernel's time in a `rocprofv3 --kernel-trace --stats` run of its own (a fresh
     child process of this script with --trace-child) beside the nms_* kernels of the tile
     batches it merges: Detector.predict on 3840x2160 frames, one frame = one batch of 32 tiles;
 (c) end to end: 3840x2160 frames resident on the device, tile 640, overlap 0.2, batch 32,
     three lanes, 8 frames per predict(): frames/s and tiles/s, alternating with the plain
     DetectPipeline (the bench's forward + NMS per 640x640 input, three lanes, result ring) on
     the same engines, `repeats` runs each: both means and both spreads.

Prints one JSON object; --out also keeps it (detect_bench.json) and the trace's CSV files.
Parts (a) and (c) set no time limit of their own: run the tool under `timeout`.
"""
import argparse
import csv
import glob
import json
import os
import re
import signal
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

from yolo_hip import _lib, synth  # noqa: E402
from yolo_hip.detect import Detector, merge, tile_transform, tiles  # noqa: E402
from yolo_hip.engine import Engine  # noqa: E402
from yolo_hip.pipeline import DetectPipeline  # noqa: E402

B, S, DT = 32, 640, torch.bfloat16
FH, FW = 2160, 3840
CAP = _lib.MERGE_MAX_CAND


def engines(n, dev):
    from nets import nn
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    out = []
    for _ in range(n):
        e = Engine(*model._yh_arch, dev, DT)
        e.load_module(model)
        e.reserve(B, S, S)
        out.append(e)
    return out


def frames(n, dev):
    """n uint8 HWC BGR 3840x2160 frames on the device (a 540x960 synthetic scene, upscaled 4x)."""
    out = []
    for i in range(n):
        x = synth.synth_scenes(1, FH // 4, FW // 4, seed=700 + i, shapes=96)[0]
        x = (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8)
        out.append(x.repeat_interleave(4, 0).repeat_interleave(4, 1).contiguous().to(dev))
    return out


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(launches=n, median_us=round(us[n // 2], 2), mean_us=round(sum(us) / n, 2), min_us=round(us[0], 2),
                p90_us=round(us[int(n * 0.9)], 2))


def _case(images, crops, md, rows_of, dev):
    """rows_of(image, tile, crop) -> (k, 6) source-space rows; crops are 640x640, so the scale is 1."""
    ntiles = len(crops)
    T = images * ntiles
    dets = np.zeros((T, md, 6), np.float32)
    counts = np.zeros((T,), np.int32)
    xf = np.zeros((T, 6), np.float32)
    for i in range(images):
        for t, c in enumerate(crops):
            r = rows_of(i, t, c)
            f = tile_transform(c, S)
            r = r.copy()
            r[:, [0, 2]] -= c[0]
            r[:, [1, 3]] -= c[1]
            dets[i * ntiles + t, :len(r)] = r
            counts[i * ntiles + t] = len(r)
            xf[i * ntiles + t] = f
    off = np.arange(images + 1, dtype=np.int32) * ntiles
    wh = np.tile(np.float32([[FW, FH]]), (images, 1))
    return [torch.from_numpy(a).to(dev) for a in (dets, counts, xf, off, wh)], ntiles


def part_a(dev, n):
    rng = np.random.default_rng(0)
    md = CAP // 16

    def disjoint(i, t, c):          # md boxes on a grid inside the tile: no two overlap, all scores differ
        g = int(np.ceil(np.sqrt(md)))
        k = np.arange(md)
        cell = S / g
        x = c[0] + (k % g) * cell
        y = c[1] + (k // g) * cell
        score = np.sort(rng.uniform(0.01, 1, md))[::-1]
        return np.stack((x + 1, y + 1, x + cell - 1, y + cell - 1, score, np.zeros(md)), 1).astype(np.float32)

    objs = [np.concatenate([rng.uniform(0, [FW - 80, 1152 - 80], (520, 2)), rng.uniform(20, 80, (520, 2)),
                            rng.integers(0, 5, (520, 1))], 1) for _ in range(8)]

    def typical(i, t, c):           # the objects this tile sees wholly, jittered: ~40 rows, each in ~2 tiles
        o = objs[i]
        see = (o[:, 0] >= c[0]) & (o[:, 1] >= c[1]) & (o[:, 0] + o[:, 2] <= c[0] + S) & (o[:, 1] + o[:, 3] <= c[1] + S)
        o = o[see]
        j = rng.normal(0, 0.5, (len(o), 4))
        score = np.sort(rng.uniform(0.01, 1, len(o)))[::-1]
        return np.stack((o[:, 0] + j[:, 0], o[:, 1] + j[:, 1], o[:, 0] + o[:, 2] + j[:, 2], o[:, 1] + o[:, 3] + j[:, 3],
                         score, o[:, 4]), 1).astype(np.float32)

    res = {}
    # 16 crops that do not overlap, so nothing is suppressed across tiles either
    worst, mt = _case(8, [((k % 6) * S, (k // 6) * S, S, S) for k in range(16)], md, disjoint, dev)
    for name, mo in (("worst_max_out_300", 300), ("worst_whole_walk", CAP)):
        out = (torch.empty((8, mo, 6), device=dev), torch.empty((8,), dtype=torch.int32, device=dev))
        res[name] = timed(lambda: merge(*worst, mt, max_out=mo, out=out), n, 20)
        res[name].update(candidates_per_image=CAP, kept=out[1].tolist())
    typ, mt = _case(8, tiles(FH, FW, S, 0.2)[:16], 300, typical, dev)      # the two top rows of the frame's tiling
    out = (torch.empty((8, 300, 6), device=dev), torch.empty((8,), dtype=torch.int32, device=dev))
    res["typical"] = timed(lambda: merge(*typ, mt, max_out=300, out=out), n, 20)
    res["typical"].update(rows_per_tile=round(float(typ[1].float().mean().item()), 1), kept=out[1].tolist())
    return res


def trace_child():
    dev = torch.device("cuda", 0)
    det = Detector(engines(1, dev), size=S, batch=B, tile=S, overlap=0.2)
    fr = frames(4, dev)
    for _ in range(6):
        det.predict(fr)
    torch.cuda.synchronize()


def part_b(out_dir):
    d = os.path.join(out_dir, "detect_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "db", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child"]
    # a session of its own: on a timeout the whole group goes (rocprofv3 and the traced python),
    # so nothing is left holding the GPU; any failure here ends the tool (main() stops on "error")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=280)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        return dict(error="rocprofv3 run exceeded 280 s; process group killed")
    if proc.returncode != 0:
        return dict(error=f"rocprofv3 exit {proc.returncode}", tail=out[-600:])
    stats = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                m = re.search(r"merge_kernel|letterbox[a-z_]*|nms_[a-z]+", row["Kernel_Name"])
                if m:
                    stats.setdefault(m.group(0), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    res = {k: dict(calls=len(v), avg_us=round(sum(v) / len(v) / 1e3, 2), median_us=round(sorted(v)[len(v) // 2] / 1e3, 2))
           for k, v in sorted(stats.items())}
    res["note"] = "4 frames per predict: one merge_kernel launch (4 workgroups) per 4 tile batches of 32 (4 x each nms_* kernel)"
    return res


def part_c(dev, repeats, calls):
    engs = engines(3, dev)
    fr = frames(8, dev)
    det = Detector(engs, size=S, batch=B, tile=S, overlap=0.2)
    ntiles = sum(len(c) for c in det.plan([(FH, FW)] * len(fr))[0])
    xs = [synth.synth_scenes(B, S, S, seed=100 + 1000 * k).to(dev, DT) for k in range(4)]
    pipe = DetectPipeline(engs, B, S, S, result_ring=True)

    def tiled():
        for _ in range(2):
            det.predict(fr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            res = det.predict(fr)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return calls * len(fr) / dt, calls * ntiles / dt, res

    def plain():
        steps = calls * ntiles // B
        for k in range(10):
            pipe.submit(xs[k % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            pipe.submit(xs[k % 4])
        torch.cuda.synchronize()
        return B * steps / (time.perf_counter() - t0)

    tiled(), plain()               # first-use costs outside the repeats
    fps, tps, ips = [], [], []
    for _ in range(repeats):       # alternating
        f, t, res = tiled()
        fps.append(f)
        tps.append(t)
        ips.append(plain())

    def summary(v):
        return dict(runs=[round(t, 1) for t in v], mean=round(statistics.mean(v), 1), spread=round(max(v) - min(v), 1))

    return dict(frames_per_call=len(fr), tiles_per_frame=ntiles // len(fr), tile_max_det=det.plan([(FH, FW)])[1],
                detections_per_frame=res.counts.tolist(), frames_s=summary(fps), tiles_s=summary(tps),
                pipeline_images_s=summary(ips),
                tiles_vs_images=round(statistics.mean(tps) / statistics.mean(ips), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    dev = torch.device("cuda", 0)
    out_dir = args.out or os.path.join(ROOT, "build", "detect_bench")
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=f"v11_n bf16 b{B} {S}x{S}, frames {FW}x{FH}", merge_max_cand=CAP,
               a=part_a(dev, max(100, args.launches)))
    res["c"] = part_c(dev, max(3, args.repeats), args.calls)
    torch.cuda.synchronize()
    res["b"] = part_b(out_dir)     # the traced child runs while this process is idle
    line = json.dumps(res)
    print(line)
    with open(os.path.join(out_dir, "detect_bench.json"), "w") as f:
        f.write(line + "\n")
    if "error" in res["b"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
