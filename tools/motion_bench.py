"""What camera-motion compensation costs (yh_motion, yh_track_warp): 32 resident 1080 x 1920 frames,
BGR and NV12, thumbnail 96 x 160, radius 8 and 16; 32 streams of 256 slots for the warp.

  python tools/motion_bench.py [--out DIR] [--blocks 15] [--launches 20]

 (a) per call, HIP events around blocks of `launches` back-to-back calls, microseconds as median and
     min-max over the blocks: yh_motion (its two launches together) per format and radius,
     yh_track_warp, and yh_letterbox_frames of the same frames to 384 x 640 for comparison.
 (b) per kernel, from a `rocprofv3 --kernel-trace` run per configuration (a fresh child each):
     motion_thumb and motion_search apart, track_warp_kernel, letterbox_frames_u8. For the thumbnail
     kernel the source-pixel rate beside the letterbox kernel's on the same frames, and its share of
     the HBM floor: the bytes it must read (3 per BGR pixel, 1 per NV12 pixel) / 8 TB/s over its time.

Every GPU step is a child process of this script under a time limit of its own; the first child that
fails or runs out of time ends the tool (its process group is killed). Prints one JSON object; --out
also keeps it (motion_bench.json).
"""
import argparse
import csv
import ctypes
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
THUMB = (96, 160)
RECT = (384, 640)
STREAMS, SLOTS = 32, 256
HBM_BYTES_S = 8e12
CONFIGS = [(fmt, r) for fmt in ("bgr", "nv12") for r in (8, 16)]


def _summary(v, nd=2):
    v = sorted(v)
    return dict(median=round(statistics.median(v), nd), min=round(v[0], nd), max=round(v[-1], nd), n=len(v))


def _setup():
    import torch
    from yolo_hip import motion as ym
    from yolo_hip import track as yt
    from yolo_hip.preprocess import NV12
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    base = torch.randint(0, 256, (FH + 64, FW + 64, 3), generator=g, dtype=torch.uint8)
    # two frames per stream, the camera 24 pixels apart: the search has something to find
    bgr = [[base[o:o + FH, o + k:o + k + FW].contiguous().to(dev) for k in range(B)] for o in (0, 24)]
    uv = torch.randint(0, 256, (FH // 2, FW), generator=g, dtype=torch.uint8).to(dev)
    nv = [[NV12(f[..., 1].contiguous(), uv) for f in fr] for fr in bgr]
    frames = dict(bgr=bgr, nv12=nv)
    tstate = yt.track_state(STREAMS, SLOTS, dev)
    tstate[:, 4:4 + SLOTS] = 2                              # every slot live
    motion = torch.tensor([[1.0, 3.5, -2.25]] * STREAMS, device=dev)
    return torch, ym, yt, dev, frames, tstate, motion


def _calls(torch, ym, yt, frames, tstate, motion):
    from yolo_hip import preprocess as pre
    cases = {}
    for fmt, r in CONFIGS:
        est = ym.MotionEstimator(B, tstate.device, thumb=THUMB, radius=r)
        est.estimate(frames[fmt][0])
        out = ym.Motion(torch.empty((B, 3), device=tstate.device), torch.empty((B, 2), dtype=torch.int32, device=tstate.device))
        cases[f"motion_{fmt}_r{r}"] = (lambda est=est, fr=frames[fmt][1], out=out: est.estimate(fr, out=out))
    cases["track_warp"] = lambda: yt.warp(tstate, motion, SLOTS)
    canvas = torch.empty((B, 3) + RECT, dtype=torch.uint8, device=tstate.device)
    for fmt in ("bgr", "nv12"):
        cases[f"letterbox_{fmt}_384x640"] = (lambda fr=frames[fmt][1]: pre.letterbox_frames(fr, RECT, out=canvas))
    return cases


def events_child(blocks, launches):
    torch, ym, yt, dev, frames, tstate, motion = _setup()
    res = {}
    for name, fn in _calls(torch, ym, yt, frames, tstate, motion).items():
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
        res[name] = dict(us_per_call=_summary([a.elapsed_time(b) * 1e3 / launches for a, b in ev]), blocks=blocks,
                         calls_per_block=launches)
    print(json.dumps(res))


def trace_child(name, calls):
    torch, ym, yt, dev, frames, tstate, motion = _setup()
    fn = _calls(torch, ym, yt, frames, tstate, motion)[name]
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def step(args, limit, prefix=()):
    """One GPU step: a fresh child of this script in a session of its own, killed as a group at `limit` s."""
    proc = subprocess.Popen(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise SystemExit(f"motion_bench: step {args} exceeded {limit} s; process group killed")
    if proc.returncode != 0:
        raise SystemExit(f"motion_bench: step {args} exit {proc.returncode}\n{(err or out)[-1500:]}")
    return out


def kernel_times(name, out_dir, calls):
    d = os.path.join(out_dir, "motion_trace", name)
    step(["--child", "trace", "--case", name, "--calls", str(calls)], 200,
         prefix=["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "mb", "--"])
    stats = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                m = re.search(r"motion_thumb|motion_search|track_warp_kernel|letterbox_frames_u8", row["Kernel_Name"])
                if m:
                    stats.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    # the first calls warm up: the median of the rest
    return {k: dict(us=_summary(v[len(v) // 4:]), launches=len(v)) for k, v in sorted(stats.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--child", default=None)
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.child == "events":
        return events_child(args.blocks, args.launches)
    if args.child == "trace":
        return trace_child(args.case, args.calls)
    out_dir = args.out or os.path.join(ROOT, "build", "motion_bench")
    os.makedirs(out_dir, exist_ok=True)
    res = dict(shape=f"{B} frames {FW}x{FH}, thumbnail {THUMB[0]}x{THUMB[1]}, warp {STREAMS} streams x {SLOTS} slots",
               a=json.loads(step(["--child", "events", "--blocks", str(args.blocks), "--launches", str(args.launches)],
                                 300).strip().splitlines()[-1]))
    kern = {}
    for name in [f"motion_{fmt}_r{r}" for fmt, r in CONFIGS] + ["track_warp", "letterbox_bgr_384x640", "letterbox_nv12_384x640"]:
        kern[name] = kernel_times(name, out_dir, args.calls)
    res["b"] = kern
    px = B * FH * FW
    rates = {}
    for fmt, bpp in (("bgr", 3), ("nv12", 1)):
        t = kern[f"motion_{fmt}_r8"]["motion_thumb"]["us"]["median"]
        lb = kern[f"letterbox_{fmt}_384x640"]["letterbox_frames_u8"]["us"]["median"]
        floor_us = px * bpp / HBM_BYTES_S * 1e6
        rates[fmt] = dict(thumb_us=t, thumb_gpx_s=round(px / t / 1e3, 2), letterbox_us=lb,
                          letterbox_source_gpx_s=round(px / lb / 1e3, 2), bytes_read=px * bpp,
                          hbm_floor_us=round(floor_us, 2), share_of_hbm_floor=round(floor_us / t, 3))
    res["thumbnail"] = rates
    line = json.dumps(res)
    print(line)
    with open(os.path.join(out_dir, "motion_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
