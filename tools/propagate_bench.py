"""What track propagation costs (yh_propagate_remember, yh_propagate): 32 resident 1080 x 1920 frames,
BGR and NV12, 50 and 250 remembered tracks per stream with boxes of about 100 x 200 pixels (cells of
3 x 6), radius 8 and 16.

  python tools/propagate_bench.py [--out DIR] [--blocks 15] [--launches 10]

 (a) per call, HIP events around blocks of `launches` back-to-back calls, microseconds as median and
     min-max over the blocks: `remember` and `propagate` (its two launches together) per configuration.
     The objects stand still between the calls, so no entry is dropped and every call does the same work.
 (b) per kernel, from a `rocprofv3 --kernel-trace` run per configuration (a fresh child each):
     propagate_remember, propagate_search and propagate_emit apart, beside the bytes each must read
     (the footprint's pixels at 3 or 1 bytes, the entries) and that over the kernel's time.
 (c) the public loop end to end, frames per second with the detector on every batch and on every third
     (remember / propagate + tracker on the others), alternating `--rounds` times, with the ratio.

Every GPU step is a child process of this script under a time limit of its own; the first child that
fails or runs out of time ends the tool (its process group is killed). Prints one JSON object; --out
also keeps it (propagate_bench.json).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

B, FH, FW = 32, 1080, 1920
BOX, CELL, P, ENTRY = (100, 200), (3, 6), 32, 1088
CONFIGS = [(fmt, n, r) for fmt in ("bgr", "nv12") for n in (50, 250) for r in (8, 16)]


def _summary(v, nd=2):
    v = sorted(v)
    return dict(median=round(statistics.median(v), nd), min=round(v[0], nd), max=round(v[-1], nd), n=len(v))


def _case(name):
    """-> (remember call, propagate call) of a configuration, on resident frames and a filled table."""
    import torch
    from yolo_hip import propagate as yp
    from yolo_hip.preprocess import NV12
    fmt, n, r = name.split("_")
    n, r = int(n[1:]), int(r[1:])
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = torch.randint(0, 256, (FH, FW + B, 3), generator=g, dtype=torch.uint8)
    frames = [base[:, k:k + FW].contiguous().to(dev) for k in range(B)]
    if fmt == "nv12":
        uv = torch.randint(0, 256, (FH // 2, FW), generator=g, dtype=torch.uint8).to(dev)
        frames = [NV12(f[..., 1].contiguous(), uv) for f in frames]
    xy = torch.rand((B, n, 2), generator=g) * torch.tensor([FW - BOX[0], FH - BOX[1]])
    dets = torch.cat([xy, xy + torch.tensor(BOX), torch.full((B, n, 1), 0.9), torch.zeros((B, n, 1))], 2).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int32).repeat(B, 1).to(dev)
    tracks = (dets, ids, torch.full((B,), n, dtype=torch.int32, device=dev))
    prop = yp.Propagator(B, dev, max_tracks=256, radius=r, max_mad=-1)
    prop.remember(frames, tracks)
    out = prop.propagate(frames)
    torch.cuda.synchronize()
    assert out.counts.tolist() == [n] * B and int(out.sad.max()) == 0, "a still scene matches exactly and keeps every entry"
    return torch, (lambda: prop.remember(frames, tracks)), (lambda: prop.propagate(frames, out=out))


def events_child(name, blocks, launches):
    torch, rem, pro = _case(name)
    res = {}
    for what, fn in (("remember", rem), ("propagate", pro)):
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(blocks)]
        for a, b in ev:
            a.record()
            for _ in range(launches):
                fn()
            b.record()
        torch.cuda.synchronize()
        res[what] = dict(us_per_call=_summary([a.elapsed_time(b) * 1e3 / launches for a, b in ev]), blocks=blocks,
                         calls_per_block=launches)
    print(json.dumps(res))


def trace_child(name, calls):
    torch, rem, pro = _case(name)
    for _ in range(calls):
        rem()
        pro()
    torch.cuda.synchronize()


def loop_child(rounds, calls, period=3):
    """(c) frames per second of the public loop, detector + tracker on every batch against the detector
    on every `period`-th batch and remember / propagate + tracker on the others; v11_n bf16 at 640,
    three lanes, BGR frames of synthetic scenes (still, so every remembered track survives); the two
    loops alternate `rounds` times."""
    import time
    import torch
    from nets import nn
    from yolo_hip import synth
    from yolo_hip import propagate as yp
    from yolo_hip.detect import Detector
    from yolo_hip.engine import Engine
    from yolo_hip.track import Tracker
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    engs = []
    for _ in range(3):
        e = Engine(*model._yh_arch, dev, torch.bfloat16)
        e.load_module(model)
        e.reserve(B, 640, 640)
        engs.append(e)
    frames = []
    for i in range(B):
        x = synth.synth_scenes(1, FH // 4, FW // 4, seed=900 + i, shapes=48)[0]
        x = (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8)
        frames.append(x.repeat_interleave(4, 0).repeat_interleave(4, 1).contiguous().to(dev))
    det = Detector(engs, size=640, batch=B)
    entries = []

    def run(every):
        trk, prop = Tracker(B, dev), yp.Propagator(B, dev, radius=8)
        def batch(i):
            if i % every == 0:
                d = det.predict(frames, keep_frames=every > 1)
                t = trk.update(d)
                if every > 1:
                    prop.remember(d.frames, t)
                return t
            p = prop.propagate(frames)
            return trk.update(p.dets, p.counts)
        for i in range(2 * every):
            t = batch(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls * every):
            t = batch(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if every > 1:
            entries.append(round(float(prop.state[:, :4].contiguous().view(torch.int32).float().mean()), 1))
        return calls * every * B / dt

    fps = {1: [], period: []}
    for every in fps:                              # first-use costs outside the rounds
        run(every)
    for _ in range(rounds):
        for every in fps:
            fps[every].append(run(every))
    ratio = [b / a for a, b in zip(fps[1], fps[period])]
    print(json.dumps(dict(frames_per_batch=B, batches_per_run={1: calls, period: calls * period}, lanes=3, radius=8,
                          entries_per_stream=entries[-1],
                          frames_s={f"every_{k}": dict(runs=[round(x, 1) for x in v], mean=round(statistics.mean(v), 1),
                                                       spread=round(max(v) - min(v), 1)) for k, v in fps.items()},
                          ratio=dict(runs=[round(x, 3) for x in ratio], mean=round(statistics.mean(ratio), 3),
                                     spread=round(max(ratio) - min(ratio), 3)))))


def step(args, limit, prefix=()):
    """One GPU step: a fresh child of this script in a session of its own, killed as a group at `limit` s."""
    proc = subprocess.Popen(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise SystemExit(f"propagate_bench: step {args} exceeded {limit} s; process group killed")
    if proc.returncode != 0:
        raise SystemExit(f"propagate_bench: step {args} exit {proc.returncode}\n{(err or out)[-1500:]}")
    return out


def kernel_times(name, out_dir, calls):
    d = os.path.join(out_dir, "propagate_trace", name)
    step(["--child", "trace", "--case", name, "--calls", str(calls)], 200,
         prefix=["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "pb", "--"])
    stats = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                m = re.search(r"propagate_remember|propagate_search|propagate_emit", row["Kernel_Name"])
                if m:
                    stats.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    fmt, n, r = name.split("_")
    n, r, bpp = int(n[1:]), int(r[1:]), 3 if fmt == "bgr" else 1
    reads = dict(propagate_remember=B * n * P * P * CELL[0] * CELL[1] * bpp,
                 propagate_search=B * n * ((P + 2 * r) ** 2 * CELL[0] * CELL[1] * bpp + ENTRY),
                 propagate_emit=B * n * (64 + 32))
    # the first calls warm up: the median of the rest
    return {k: dict(us=_summary(v[len(v) // 4:]), launches=len(v), bytes_read=reads[k],
                    gb_s=round(reads[k] / statistics.median(v[len(v) // 4:]) / 1e3, 1)) for k, v in sorted(stats.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--match", default="", help="only the configurations whose name contains this (bgr, _r16, ...; "
                    "`loop`: none of them, (c) alone, which keeps the (a) and (b) of an earlier run in --out)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.child == "events":
        return events_child(args.case, args.blocks, args.launches)
    if args.child == "trace":
        return trace_child(args.case, args.calls)
    if args.child == "loop":
        return loop_child(args.rounds, args.calls)
    out_dir = args.out or os.path.join(ROOT, "build", "propagate_bench")
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=f"{B} frames {FW}x{FH}, boxes {BOX[0]}x{BOX[1]} (cells {CELL[0]}x{CELL[1]}), max_tracks 256", a={}, b={})
    for fmt, n, r in CONFIGS:
        name = f"{fmt}_n{n}_r{r}"
        if args.match not in name:
            continue
        res["a"][name] = json.loads(step(["--child", "events", "--case", name, "--blocks", str(args.blocks), "--launches",
                                          str(args.launches)], 200).strip().splitlines()[-1])
        res["b"][name] = kernel_times(name, out_dir, args.calls)
    kept = os.path.join(out_dir, "propagate_bench.json")
    if args.match == "loop" and os.path.exists(kept):
        with open(kept) as f:
            res = json.load(f)
    res["c"] = json.loads(step(["--child", "loop", "--rounds", str(args.rounds), "--calls", str(args.calls)], 300)
                          .strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    with open(os.path.join(out_dir, "propagate_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
