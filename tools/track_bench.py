"""What the tracker costs, at the bench's C2 shape (v11_n bf16, batch 32 = 32 video streams,
640x640, 300 NMS rows per stream).

  python tools/track_bench.py [--out DIR] [--launches 400] [--repeats 3] [--steps 50]

 (a) yh_track per launch, HIP events around blocks of 40 back-to-back launches: 32 streams x 300
     rows, of which about 50 and about 250 are objects that move and are tracked (the other rows
     are clutter below track_low, as an NMS at conf 0.001 returns it), max_tracks 256. The
     sequence plays forwards and backwards, so it has no end; the live tracks are counted from
     the state afterwards;
 (b) the host twin on the same frames, 16 threads, wall clock;
 (c) yh_nms of a forward of the same batch size, for scale;
 (d) DetectPipeline img/s, 3 lanes, result_ring=True, with and without post=Tracker.post,
     alternating, `repeats` runs each: both means and both spreads. The frames are the bench's
     four synthetic scenes in turn, so here the tracker mostly sees births and tentative tracks;
     with the host time of the hook per call and the kernel's time on exactly these frames.

Prints one JSON object; --out also keeps it (track_bench.json). The tool sets no time limit of
its own: run it under `timeout`.
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

from yolo_hip import synth  # noqa: E402
from yolo_hip import track as yt  # noqa: E402
from yolo_hip.engine import Engine, nms  # noqa: E402
from yolo_hip.pipeline import DetectPipeline  # noqa: E402

B, S, DT, MD, MT = 32, 640, torch.bfloat16, 300, 256
BLOCK = 40      # frames of the sequence = launches per event pair


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


def video(objects, seed):
    """BLOCK frames of (B, MD, 6) / (B,): `objects` boxes per stream on straight lines with jitter,
    classes 0..7, scores 0.3..0.95 with a fifth in the low band, clutter up to MD rows."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(60, S - 60, (B, objects, 2))
    vel = rng.uniform(-1.5, 1.5, (B, objects, 2))
    wh = rng.uniform(20, 90, (B, objects, 2))
    cls = rng.integers(0, 8, (B, objects)).astype(np.float64)
    frames = []
    for f in range(BLOCK):
        c = pos + vel * f + rng.normal(0, 0.7, pos.shape)
        score = np.where(rng.random((B, objects)) < 0.2, rng.uniform(0.1, 0.25, (B, objects)),
                         rng.uniform(0.3, 0.95, (B, objects)))
        obj = np.concatenate([c - wh / 2, c + wh / 2, score[..., None], cls[..., None]], 2)
        cc, cw = rng.uniform(30, S - 30, (B, MD - objects, 2)), rng.uniform(10, 120, (B, MD - objects, 2))
        clutter = np.concatenate([cc - cw / 2, cc + cw / 2, rng.uniform(0.001, 0.09, (B, MD - objects, 1)),
                                  rng.integers(0, 8, (B, MD - objects, 1)).astype(np.float64)], 2)
        rows = np.concatenate([obj, clutter], 1)
        order = np.argsort(-rows[..., 4], 1)                       # NMS output is in score order
        rows = np.take_along_axis(rows, order[..., None], 1)
        frames.append((torch.from_numpy(rows.astype(np.float32)), torch.full((B,), MD, dtype=torch.int32)))
    return frames


def live(state):
    st = state[:, 4:4 + MT].cpu()
    return dict(tracked=round(float((st == 2).sum()) / B, 1), lost=round(float((st == 3).sum()) / B, 1),
                tentative=round(float((st == 1).sum()) / B, 1))


def part_a(dev, objects, launches, frames=None):
    if frames is None:
        frames = [(d.to(dev), c.to(dev)) for d, c in video(objects, 1)]
        order = list(range(BLOCK)) + list(range(BLOCK - 2, 0, -1))    # there and back again
    else:
        order = list(range(len(frames)))
    trk = yt.Tracker(B, dev, max_tracks=MT)
    out = None
    at = 0

    def block():
        nonlocal out, at
        for _ in range(BLOCK):
            d, c = frames[order[at % len(order)]]
            at += 1
            out = yt.track(d, c, trk.state, trk.params, out=out)

    block()
    torch.cuda.synchronize()
    n = max(3, launches // BLOCK)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        block()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / BLOCK for a, b in ev)
    return dict(objects=objects, launches=n * BLOCK, us_per_launch_median=round(us[n // 2], 2),
                us_per_launch_min=round(us[0], 2), us_per_launch_max=round(us[-1], 2),
                out_rows_per_stream=round(float(out.counts.float().mean()), 1), slots=live(trk.state))


def part_b(objects, launches):
    frames = video(objects, 1)
    order = list(range(BLOCK)) + list(range(BLOCK - 2, 0, -1))
    trk = yt.Tracker(B, "cpu", max_tracks=MT)
    out = None
    ts = []
    for i in range(BLOCK + launches):
        d, c = frames[order[i % len(order)]]
        t0 = time.perf_counter()
        out = yt.track(d, c, trk.state, trk.params, out=out, threads=16)
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = sorted(ts[BLOCK:])
    return dict(objects=objects, threads=16, calls=launches, us_per_call_median=round(ts[len(ts) // 2], 1),
                us_per_call_min=round(ts[0], 1), slots=live(trk.state))


def part_c(dev, eng):
    x = synth.synth_scenes(B, S, S, seed=100).to(dev, DT)
    y = eng.forward(x)
    dets, counts = nms(y)
    out = (dets, counts)
    for _ in range(5):
        nms(y, out=out)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
    for a, b in ev:
        a.record()
        for _ in range(10):
            nms(y, out=out)
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / 10 for a, b in ev)
    return dict(us_per_call_median=round(us[5], 2), us_per_call_min=round(us[0], 2),
                mean_detections=round(float(counts.float().mean()), 1))


def part_d(dev, engs, repeats, steps):
    xs = [synth.synth_scenes(B, S, S, seed=100 + 1000 * k).to(dev, DT) for k in range(4)]
    slots = {}
    host = []

    def run(with_post):
        trk = yt.Tracker(B, dev, max_tracks=MT) if with_post else None

        def post(dets, counts):        # the hook, with the host time it takes
            t0 = time.perf_counter()
            r = trk.post(dets, counts)
            host.append((time.perf_counter() - t0) * 1e6)
            return r
        pipe = DetectPipeline(engs, B, S, S, post=post if trk else None, result_ring=True)
        for k in range(10):
            pipe.submit(xs[k % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            pipe.submit(xs[k % 4])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if trk:
            assert int(trk.state[0, 0]) == steps + 10           # every frame went through the tracker
            slots.update(live(trk.state))
        return B * steps / dt

    run(True), run(False)          # first-use costs outside the repeats
    got = {"without_post": [], "with_post": []}
    for _ in range(repeats):       # alternating
        got["without_post"].append(run(False))
        got["with_post"].append(run(True))
    out = {}
    for k, v in got.items():
        out[k] = dict(img_s=[round(t, 1) for t in v], mean=round(statistics.mean(v), 1),
                      spread=round(max(v) - min(v), 1))
    out["difference_of_means"] = round(out["without_post"]["mean"] - out["with_post"]["mean"], 1)
    out["slots"] = slots
    out["post_host_us_median"] = round(sorted(host)[len(host) // 2], 1)
    # the kernel alone on the frames the pipeline's tracker sees (the four scenes' detections in turn)
    frames = [nms(engs[0].forward(x)) for x in xs]
    out["kernel_on_these_frames"] = part_a(dev, None, 400, frames=frames)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out_dir = args.out or os.path.join(ROOT, "build", "track_bench")
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=f"{B} streams x {MD} rows, max_tracks {MT}")
    res["a"] = [part_a(dev, n, args.launches) for n in (50, 250)]
    res["b"] = [part_b(n, min(args.launches, 200)) for n in (50, 250)]
    engs = engines(3, dev)
    res["c"] = part_c(dev, engs[0])
    res["d"] = part_d(dev, engs, max(3, args.repeats), args.steps)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(out_dir, "track_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
