"""What the video front end costs and gains (yolo_hip.preprocess.letterbox_frames,
Detector(canvas=...)), v11_n bf16, 1080 x 1920 frames resident on the device.

  python tools/video_bench.py [--out DIR] [--parent-lib PATH] [--rounds 3] [--blocks 15]
                              [--launches 20] [--calls 10]

 (a) the letterbox kernel alone: HIP events around blocks of `launches` back-to-back launches,
     32 frames per launch, per-launch microseconds as median and min-max over the blocks:
       bgr_640       yh_letterbox, BGR to a 640 x 640 canvas
       bgr_384x640   yh_letterbox_frames, BGR to 384 x 640
       nv12_384x640  yh_letterbox_frames, NV12 (BT.601) to 384 x 640
     With --parent-lib (a libyolo_hip.so built from the parent commit) bgr_640 is measured
     through that library as well, parent and this tree alternating for `rounds` rounds, each
     in a fresh child process that loads one library only.
 (b) end to end: Detector.predict frames/s, tile=None, three lanes, batch 32, 32 frames per
     call, for the square 640 canvas with BGR, canvas=(384, 640) with BGR and with NV12;
     `rounds` alternating runs each, every run `calls` predict() calls after two of warm-up.

Every GPU step is a child process of this script under a time limit of its own; the first child
that fails or runs out of time ends the tool (its process group is killed, nothing is left on
the GPU). Prints one JSON object; --out also keeps it (video_bench.json).
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

B, DT_NAME = 32, "bf16"
FH, FW = 1080, 1920
RECT = (384, 640)


class _Frame(ctypes.Structure):          # yh_frame (include/yolo_hip.h)
    _fields_ = [("plane0", ctypes.c_void_p), ("plane1", ctypes.c_void_p), ("height", ctypes.c_int),
                ("width", ctypes.c_int), ("stride0", ctypes.c_int), ("stride1", ctypes.c_int),
                ("format", ctypes.c_int), ("matrix", ctypes.c_int)]


def _summary(v, nd=2):
    v = sorted(v)
    return dict(median=round(statistics.median(v), nd), min=round(v[0], nd), max=round(v[-1], nd), n=len(v))


def kernel_child(lib_path, blocks, launches):
    """Loads one library with plain ctypes (a parent build lacks the newer symbols)."""
    import torch
    L = ctypes.CDLL(lib_path)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    bgr = [torch.randint(0, 256, (FH, FW, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    ys = [torch.randint(0, 256, (FH, FW), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    uvs = [torch.randint(0, 256, (FH // 2, FW), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sq = torch.empty((B, 3, 640, 640), dtype=torch.uint8, device=dev)
    rc = torch.empty((B, 3) + RECT, dtype=torch.uint8, device=dev)
    ptrs = (ctypes.c_void_p * B)(*[t.data_ptr() for t in bgr])
    hs, ws, st = (ctypes.c_int * B)(*[FH] * B), (ctypes.c_int * B)(*[FW] * B), (ctypes.c_int * B)(*[3 * FW] * B)
    cases = {}

    def old():
        assert L.yh_letterbox(ptrs, hs, ws, st, B, 640, ctypes.c_void_p(sq.data_ptr()), stream) == 0
    cases["bgr_640"] = old
    if hasattr(L, "yh_letterbox_frames"):
        fb = (_Frame * B)(*[_Frame(t.data_ptr(), None, FH, FW, 0, 0, 0, 0) for t in bgr])
        fn = (_Frame * B)(*[_Frame(y.data_ptr(), uv.data_ptr(), FH, FW, 0, 0, 1, 0) for y, uv in zip(ys, uvs)])

        def frames(desc):
            def run():
                assert L.yh_letterbox_frames(desc, B, RECT[0], RECT[1], ctypes.c_void_p(rc.data_ptr()), stream) == 0
            return run
        cases["bgr_384x640"] = frames(fb)
        cases["nv12_384x640"] = frames(fn)
    res = {}
    for name, fn_ in cases.items():
        for _ in range(launches):
            fn_()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(blocks)]
        for a, b in ev:
            a.record()
            for _ in range(launches):
                fn_()
            b.record()
        torch.cuda.synchronize()
        res[name] = dict(us_per_launch=_summary([a.elapsed_time(b) * 1e3 / launches for a, b in ev]),
                         blocks=blocks, launches_per_block=launches, frames_per_launch=B)
    res["checksum_bgr_640"] = int(sq.sum(dtype=torch.int64).item())
    print(json.dumps(res))


def e2e_child(rounds, calls):
    import torch
    from nets import nn
    from yolo_hip import synth
    from yolo_hip.detect import Detector
    from yolo_hip.engine import Engine
    from yolo_hip.preprocess import NV12
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nn.yolo_v11_n(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()

    def engines(h, w):
        out = []
        for _ in range(3):
            e = Engine(*model._yh_arch, dev, torch.bfloat16)
            e.load_module(model)
            e.reserve(B, h, w)
            out.append(e)
        return out

    # 32 frames: a 270 x 480 synthetic scene each, upscaled 4x; the NV12 twin by a float BT.601 transform
    bgr, nv = [], []
    for i in range(B):
        x = synth.synth_scenes(1, FH // 4, FW // 4, seed=900 + i, shapes=48)[0]
        x = (x.flip(0).permute(1, 2, 0) * 255.0).round().to(torch.uint8)
        x = x.repeat_interleave(4, 0).repeat_interleave(4, 1).contiguous().to(dev)
        bgr.append(x)
        f = x.float()
        y = (16 + 0.098 * f[..., 0] + 0.504 * f[..., 1] + 0.257 * f[..., 2]).round().clamp(0, 255).to(torch.uint8)
        c = f[0::2, 0::2]
        u = (128 + 0.439 * c[..., 0] - 0.291 * c[..., 1] - 0.148 * c[..., 2]).round().clamp(0, 255).to(torch.uint8)
        v = (128 - 0.071 * c[..., 0] - 0.368 * c[..., 1] + 0.439 * c[..., 2]).round().clamp(0, 255).to(torch.uint8)
        nv.append(NV12(y.contiguous(), torch.stack((u, v), -1).reshape(FH // 2, FW).contiguous()))
    sq = Detector(engines(640, 640), size=640, batch=B)
    rect = Detector(engines(*RECT), batch=B, canvas=RECT)
    runs = {"square_640_bgr": (sq, bgr), "rect_384x640_bgr": (rect, bgr), "rect_384x640_nv12": (rect, nv)}

    def run(det, fr):
        for _ in range(2):
            det.predict(fr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            r = det.predict(fr)
        torch.cuda.synchronize()
        return calls * len(fr) / (time.perf_counter() - t0), r

    fps = {k: [] for k in runs}
    kept = {}
    for k, (det, fr) in runs.items():          # first-use costs outside the rounds
        run(det, fr)
    for _ in range(rounds):                     # alternating
        for k, (det, fr) in runs.items():
            f, r = run(det, fr)
            fps[k].append(f)
            kept[k] = int(r.counts.sum().item())
    print(json.dumps(dict(frames_per_call=B, calls=calls, lanes=3,
                          frames_s={k: dict(runs=[round(x, 1) for x in v], mean=round(statistics.mean(v), 1),
                                            spread=round(max(v) - min(v), 1)) for k, v in fps.items()},
                          detections_last_call=kept)))


def step(args, limit):
    """One GPU step: a fresh child of this script in a session of its own, killed as a group at `limit` s."""
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise SystemExit(f"video_bench: step {args} exceeded {limit} s; process group killed")
    if proc.returncode != 0:
        raise SystemExit(f"video_bench: step {args} exit {proc.returncode}\n{err[-1500:]}")
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.child == "kernel":
        return kernel_child(args.lib, args.blocks, args.launches)
    if args.child == "e2e":
        return e2e_child(args.rounds, args.calls)
    from yolo_hip import _lib
    libs = [("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else []
    libs.append(("this", _lib.LIB_PATH))
    kern = {name: [] for name, _ in libs}
    for _ in range(max(1, args.rounds)):        # alternating
        for name, path in libs:
            kern[name].append(step(["--child", "kernel", "--lib", path, "--blocks", str(args.blocks),
                                    "--launches", str(args.launches)], 120))
    res = dict(shape=f"v11_n {DT_NAME} b{B}, frames {FW}x{FH}", a=kern)
    sums = {r["checksum_bgr_640"] for v in kern.values() for r in v}
    res["bgr_640_same_bytes"] = len(sums) == 1
    if not args.skip_e2e:
        res["b"] = step(["--child", "e2e", "--rounds", str(max(1, args.rounds)), "--calls", str(args.calls)], 420)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "video_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
