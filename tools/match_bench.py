"""What the batched evaluator costs, at the bench's C2 shape (v11_n bf16, batch 32, 640x640,
up to 300 detections per image, 0-90 labels per image with a mean of about 7).

  python tools/match_bench.py [--out DIR] [--batches 200] [--repeats 3] [--steps 50]

 (a) per batch, HIP events: the parent's way (counts.tolist() + per-image slicing +
     compute_metric, main.py:275-294) against one yh_match launch on resident labels and
     against the whole Evaluator.update (label conversion, upload and launch);
 (b) the match kernel's time in a `rocprofv3 --kernel-trace --stats` run of its own (a fresh
     child process of this script with --trace-child), beside the nms_* kernels;
 (c) DetectPipeline img/s, 3 lanes, result_ring=True, with and without post=ev.post,
     alternating, `repeats` runs each: both means and both spreads.

Prints one JSON object; --out also keeps it (match_bench.json) and the trace's CSV files.
Parts (a) and (c) set no time limit of their own: run the tool under `timeout`. A failed or
timed-out trace ends the tool with a non-zero status after the results so far are written.
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

from yolo_hip import synth  # noqa: E402
from yolo_hip.engine import Engine, nms  # noqa: E402
from yolo_hip.evaluate import Evaluator  # noqa: E402
from yolo_hip.metrics import compute_metric, match_batch  # noqa: E402
from yolo_hip.pipeline import DetectPipeline  # noqa: E402

B, S, DT = 32, 640, torch.bfloat16


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


def make_targets(dets, counts, seed):
    """main.py's collated CPU targets: per image L ~ min(90, geometric with mean 7) labels,
    jittered copies of that image's detections."""
    g = torch.Generator().manual_seed(seed)
    dets, counts = dets.cpu(), counts.cpu().tolist()
    cls, box, idx = [], [], []
    for i, k in enumerate(counts):
        n = min(90, int(torch.empty(1).exponential_(1 / 7.0, generator=g).item()))
        if k == 0 or n == 0:
            continue
        src = torch.randint(0, k, (n,), generator=g)
        c = dets[i, src, :4] + torch.randn((n, 4), generator=g) * 3.0
        cls.append(dets[i, src, 5:6])
        box.append(torch.stack(((c[:, 0] + c[:, 2]) / 2 / S, (c[:, 1] + c[:, 3]) / 2 / S,
                                (c[:, 2] - c[:, 0]) / S, (c[:, 3] - c[:, 1]) / S), 1))
        idx.append(torch.full((n,), float(i)))
    if not cls:
        return {"cls": torch.zeros((0, 1)), "box": torch.zeros((0, 4)), "idx": torch.zeros((0,))}
    return {"cls": torch.cat(cls), "box": torch.cat(box), "idx": torch.cat(idx)}


def old_way(dets, counts, targets, iou_v, scale, dev):
    """The parent commit's path for one batch (main.py:275-294 on the fixed-size NMS output)."""
    from utils import util
    metrics = []
    for i, k in enumerate(counts.tolist()):                 # host sync
        output = dets[i, :k]
        sel = targets["idx"] == i
        cls, box = targets["cls"][sel].to(dev), targets["box"][sel].to(dev)
        metric = torch.zeros(output.shape[0], iou_v.shape[0], dtype=torch.bool, device=dev)
        if output.shape[0] == 0:
            continue
        if cls.shape[0]:
            metric = compute_metric(output[:, :6], torch.cat((cls, util.wh2xy(box) * scale), 1), iou_v)
        metrics.append((metric, output[:, 4], output[:, 5], cls.squeeze(-1)))
    return metrics


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
    return dict(batches=n, median_us=round(us[n // 2], 2), mean_us=round(sum(us) / n, 2), min_us=round(us[0], 2),
                p90_us=round(us[int(n * 0.9)], 2))


def part_a(dev, n):
    eng = engines(1, dev)[0]
    x = synth.synth_scenes(B, S, S, seed=100).to(dev, DT)
    dets, counts = nms(eng.forward(x))
    targets = make_targets(dets, counts, 1)
    iou_v = torch.linspace(0.5, 0.95, 10).to(dev)
    scale = torch.tensor((S, S, S, S)).to(dev)
    ev = Evaluator(dev)
    labels, offsets, _ = ev._labels(targets, (S, S), B)
    tp = torch.empty((B, 300, 10), dtype=torch.uint8, device=dev)
    res = dict(mean_detections=float(counts.float().mean().item()), labels_in_batch=int(targets["idx"].shape[0]))
    res["parent_tolist_compute_metric"] = timed(lambda: old_way(dets, counts, targets, iou_v, scale, dev), n, 5)
    res["yh_match_launch"] = timed(lambda: match_batch(dets, counts, labels, offsets, iou_v, out=tp), n, 20)
    res["evaluator_update"] = timed(lambda: ev.update(dets, counts, targets, (S, S)), n, 20)
    return res


def trace_child():
    dev = torch.device("cuda", 0)
    eng = engines(1, dev)[0]
    x = synth.synth_scenes(B, S, S, seed=100).to(dev, DT)
    y = eng.forward(x)
    dets, counts = nms(y)
    targets = make_targets(dets, counts, 1)
    ev = Evaluator(dev)
    for _ in range(50):
        dets, counts = nms(y)
        ev.update(dets, counts, targets, (S, S))
    torch.cuda.synchronize()


def part_b(out_dir):
    d = os.path.join(out_dir, "match_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "mb", "--",
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
                m = re.search(r"match_kernel|nms_[a-z]+", row["Kernel_Name"])   # mangled or demangled names
                if m:
                    c = stats.setdefault(m.group(0), [])
                    c.append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {k: dict(calls=len(v), avg_us=round(sum(v) / len(v) / 1e3, 2), median_us=round(sorted(v)[len(v) // 2] / 1e3, 2))
            for k, v in sorted(stats.items())}


def part_c(dev, repeats, steps):
    engs = engines(3, dev)
    xs = [synth.synth_scenes(B, S, S, seed=100 + 1000 * k).to(dev, DT) for k in range(4)]
    y = torch.empty((B, 84, engs[0].num_anchors(S, S)), dtype=DT, device=dev)
    tg = []
    for e in engs:
        e.forward(xs[0], out=y)
        torch.cuda.synchronize()
    for x in xs:
        d, c = nms(engs[0].forward(x))
        tg.append(make_targets(d, c, 7))
    torch.cuda.synchronize()

    def run(with_post):
        ev = Evaluator(dev) if with_post else None
        pipe = DetectPipeline(engs, B, S, S, post=ev.post if ev else None, result_ring=True)

        def step(k):
            if ev:
                ev.stage(tg[k % 4], (S, S))
            pipe.submit(xs[k % 4])
        for k in range(10):
            step(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if ev:
            pipe.drain()
            assert ev.images == B * (steps + 10)
        return B * steps / dt

    run(True), run(False)          # first-use costs (storage blocks, pinned staging) outside the repeats
    got = {"without_post": [], "with_post": []}
    for _ in range(repeats):       # alternating
        got["without_post"].append(run(False))
        got["with_post"].append(run(True))
    out = {}
    for k, v in got.items():
        out[k] = dict(img_s=[round(t, 1) for t in v], mean=round(statistics.mean(v), 1),
                      spread=round(max(v) - min(v), 1))
    out["difference_of_means"] = round(out["without_post"]["mean"] - out["with_post"]["mean"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    dev = torch.device("cuda", 0)
    out_dir = args.out or os.path.join(ROOT, "build", "match_bench")
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=f"v11_n bf16 b{B} {S}x{S}", a=part_a(dev, max(200, args.batches)))
    res["c"] = part_c(dev, max(3, args.repeats), args.steps)
    torch.cuda.synchronize()
    res["b"] = part_b(out_dir)     # the traced child runs while this process is idle
    line = json.dumps(res)
    print(line)
    with open(os.path.join(out_dir, "match_bench.json"), "w") as f:
        f.write(line + "\n")
    if "error" in res["b"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
