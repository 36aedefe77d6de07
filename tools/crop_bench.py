"""What yh_crop_rois costs (yolo_hip.preprocess.crop_rois) and what it replaces: 32 frames of
1080 x 1920 resident on the device, BGR and NV12, 16 and 100 boxes per frame, cropped to 128 x 64
(stretched) and to 224 x 224 (keep-aspect).

  python tools/crop_bench.py [--out DIR] [--blocks 15] [--launches 20] [--calls 2]

 (a) the kernel: HIP events around blocks of `launches` back-to-back calls of yh_crop_rois (one
     launch, 32 frames), per-call microseconds as median and min-max over the blocks. `bytes` is
     what the call moves by count: the crops written plus the source taps read (4 per resized
     pixel on the linear and the 2x area path, 1 on the copy path; 3 bytes a BGR tap, 3 bytes an
     NV12 tap: Y, U, V), and `of_8TBs` that count over the median time as a fraction of 8 TB/s.
     Taps overlap heavily, so this is a rate of requests, not of DRAM traffic.
 (b) the baseline, what a user does without the kernel: Detections.tolist() (a host
     synchronisation), a Python loop over the boxes, a float copy of the frame (an NV12 frame
     converted to BGR in full first, with torch ops) and torch.nn.functional.interpolate per
     box, stacked into one uint8 batch. Its rounding differs from the kernel's: it is a cost
     baseline only. Milliseconds per call over `calls` calls after one of warm-up.

Every GPU step is a child process of this script under a time limit of its own; the first child
that fails or runs out of time ends the tool (its process group is killed, nothing is left on
the GPU). Prints one JSON object; --out also keeps it (crop_bench.json).
"""
import argparse
import ctypes
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

B = 32
FH, FW = 1080, 1920
ROIS = (16, 100)
MODES = (("128x64_stretch", (128, 64), False), ("224x224_keep", (224, 224), True))
PEAK = 8e12


def _summary(v, nd=2):
    v = sorted(v)
    return dict(median=round(statistics.median(v), nd), min=round(v[0], nd), max=round(v[-1], nd), n=len(v))


def _workload(dev):
    """Frames and boxes: person-like boxes, 40..200 wide and 80..400 high, some over the frame's edge."""
    import torch
    from yolo_hip.preprocess import NV12
    g = torch.Generator(device="cpu").manual_seed(0)
    bgr = [torch.randint(0, 256, (FH, FW, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    nv = [NV12(torch.randint(0, 256, (FH, FW), generator=g, dtype=torch.uint8).to(dev),
               torch.randint(0, 256, (FH // 2, FW), generator=g, dtype=torch.uint8).to(dev)) for _ in range(B)]
    dets = {}
    for m in ROIS:
        w = 40 + 160 * torch.rand((B, m), generator=g)
        h = 80 + 320 * torch.rand((B, m), generator=g)
        x1 = -20 + (FW - 0.8 * w + 20) * torch.rand((B, m), generator=g)
        y1 = -20 + (FH - 0.8 * h + 20) * torch.rand((B, m), generator=g)
        d = torch.stack((x1, y1, x1 + w, y1 + h, torch.rand((B, m), generator=g), torch.zeros((B, m))), -1)
        dets[m] = (d.contiguous().to(dev), torch.full((B,), m, dtype=torch.int32).to(dev))
    return dict(bgr=bgr, nv12=nv), dets


def _bytes(rois, size, keep_aspect):
    """Crops written and source taps read by one call, by count (see the module docstring)."""
    from yolo_hip.preprocess import geometry
    oh, ow = size
    taps = 0
    for _, _, _, _, w, h in rois:
        if w == 0:
            continue
        nh, nw = geometry(h, w, size)[:2] if keep_aspect else (oh, ow)
        taps += nh * nw * (1 if (nh, nw) == (h, w) else 4)
    return len(rois) * 3 * oh * ow, 3 * taps


def kernel_child(blocks, launches):
    import torch
    from yolo_hip import _lib
    from yolo_hip import preprocess as pre
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    frames, dets = _workload(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res = {}
    for fmt, fr in frames.items():
        descs = (_lib.YhFrame * B)(*[f._desc() if isinstance(f, pre.NV12) else pre._bgr_desc(f) for f in fr])
        for m, (d, c) in dets.items():
            for name, size, keep in MODES:
                out = pre.crop_rois(fr, d, c, size, keep_aspect=keep)      # through the public call once
                args = (descs, B, ctypes.c_void_p(d.data_ptr()), 6, ctypes.c_void_p(c.data_ptr()), m, size[0], size[1],
                        int(keep), 0.0, B * m, ctypes.c_void_p(out.data.data_ptr()),
                        ctypes.c_void_p(out.rois.data_ptr()), ctypes.c_void_p(out.total.data_ptr()), stream)

                def run():
                    assert L.yh_crop_rois(*args) == 0
                for _ in range(launches):
                    run()
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(blocks)]
                for a, b in ev:
                    a.record()
                    for _ in range(launches):
                        run()
                    b.record()
                torch.cuda.synchronize()
                us = _summary([a.elapsed_time(b) * 1e3 / launches for a, b in ev])
                assert int(out.total.item()) == B * m
                written, read = _bytes(out.rois.cpu().tolist(), size, keep)
                res[f"{fmt}_{m}_{name}"] = dict(
                    us_per_call=us, rois=B * m, bytes_written=written, bytes_tapped=read,
                    of_8TBs=round((written + read) / (us["median"] * 1e-6) / PEAK, 4),
                    checksum=int(out.data.sum(dtype=torch.int64).item()))
    print(json.dumps(dict(blocks=blocks, launches_per_block=launches, frames_per_call=B, cases=res)))


def baseline_child(calls):
    import torch
    import torch.nn.functional as F
    from yolo_hip.detect import Detections
    from yolo_hip.preprocess import NV12
    dev = torch.device("cuda", 0)
    frames, dets = _workload(dev)

    def to_bgr(f):
        """Full-frame BT.601 conversion in float, as a user without the kernel writes it."""
        y = (f.y.float() - 16).clamp_(min=0) * 1.164
        uv = f.uv.float().view(FH // 2, FW // 2, 2) - 128
        uv = uv.repeat_interleave(2, 0).repeat_interleave(2, 1)
        u, v = uv[..., 0], uv[..., 1]
        return torch.stack((y + 2.018 * u, y - 0.391 * u - 0.813 * v, y + 1.596 * v), -1).clamp_(0, 255)

    def loop(fr, det, size):
        out = []
        for f, rows in zip(fr, det.tolist()):                              # synchronises
            img = to_bgr(f) if isinstance(f, NV12) else f.float()          # the float copy
            img = img.permute(2, 0, 1).flip(0)[None]                       # RGB, CHW
            for x1, y1, x2, y2 in rows[:, :4].tolist():
                x1, y1 = max(int(x1), 0), max(int(y1), 0)
                x2, y2 = min(int(x2) + 1, FW), min(int(y2) + 1, FH)
                out.append(F.interpolate(img[:, :, y1:y2, x1:x2], size=size, mode="bilinear", align_corners=False))
        return torch.cat(out).round_().to(torch.uint8)

    res = {}
    for fmt, fr in frames.items():
        for m, (d, c) in dets.items():
            det = Detections(d, c)
            for name, size, _ in MODES:      # the loop stretches in both modes: a letterbox would only add work
                loop(fr, det, size)
                torch.cuda.synchronize()
                ms = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    r = loop(fr, det, size)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert r.shape == (B * m, 3) + size
                res[f"{fmt}_{m}_{name}"] = dict(ms_per_call=_summary(ms), rois=B * m)
    print(json.dumps(dict(calls=calls, cases=res)))


def step(args, limit):
    """One GPU step: a fresh child of this script in a session of its own, killed as a group at `limit` s."""
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise SystemExit(f"crop_bench: step {args} exceeded {limit} s; process group killed")
    if proc.returncode != 0:
        raise SystemExit(f"crop_bench: step {args} exit {proc.returncode}\n{err[-1500:]}")
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child == "kernel":
        return kernel_child(args.blocks, args.launches)
    if args.child == "baseline":
        return baseline_child(args.calls)
    res = dict(shape=f"{B} frames {FW}x{FH}, rois per frame {list(ROIS)}",
               kernel=step(["--child", "kernel", "--blocks", str(args.blocks), "--launches", str(args.launches)], 180))
    if not args.skip_baseline:
        res["baseline"] = step(["--child", "baseline", "--calls", str(args.calls)], 420)
        res["baseline_over_kernel"] = {
            k: round(res["baseline"]["cases"][k]["ms_per_call"]["median"] * 1e3 / v["us_per_call"]["median"], 1)
            for k, v in res["kernel"]["cases"].items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "crop_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
