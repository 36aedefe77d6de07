"""What the optimal assignment costs in the tracker, by tools/track_bench.py's procedure: 32 video
streams x 300 NMS rows, max_tracks 256, HIP events around blocks of 40 back-to-back launches,
median and min - max of the blocks.

  python tools/assign_bench.py [--parent-lib PATH] [--out DIR] [--launches 400]

On track_bench's synthetic video with about 50 and about 250 tracked objects per stream, and on the
benchmark's four unrelated synthetic scenes in turn (the tracker's worst input: births and
tentative tracks only), all in one run:
  greedy_parent   yh_track through the old entry point of the library at --parent-lib (the parent
                  commit's build; the row is left out without it)
  greedy          yh_track2 in YH_ASSIGN_GREEDY mode (yolo_hip.track's default)
  optimal         yh_track2 in YH_ASSIGN_OPTIMAL mode
  reid_greedy, reid_optimal   yh_track_reid2 at dim 1280, every row with a feature (the video only)
and yh_assign alone on 32 problems of the 256 x 300 sparse and of the 128 x 128 dense test case.

Prints one JSON object; --out also keeps it (assign_bench.json). The tool sets no time limit of its
own: run it under `timeout`.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import track_bench as tb  # noqa: E402
import yolo_hip  # noqa: E402
from yolo_hip import _lib  # noqa: E402
from yolo_hip import synth  # noqa: E402
from yolo_hip import track as yt  # noqa: E402
from yolo_hip.engine import nms  # noqa: E402

B, S, MD, MT, BLOCK, DIM = tb.B, tb.S, tb.MD, tb.MT, tb.BLOCK, 1280


def timed(block, launches):
    """block(): BLOCK launches. -> median / min / max microseconds per launch over the blocks."""
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
    return dict(launches=n * BLOCK, us_median=round(us[n // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2))


def parent_track(path):
    """yh_track of another build of the library, called with the arguments yolo_hip.track passes."""
    lib = ctypes.CDLL(path)
    v, i = ctypes.c_void_p, ctypes.c_int
    lib.yh_track.restype = i
    lib.yh_track.argtypes = [v, v, i, i, v, v, i, i, v, i, v, v, v, v, v]

    def call(d, c, state, p, out):
        rc = lib.yh_track(d.data_ptr(), c.data_ptr(), B, MD, None, state.data_ptr(), state.shape[0], MT,
                          ctypes.byref(p), MD, out.dets.data_ptr(), out.ids.data_ptr(), out.det_index.data_ptr(),
                          out.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return out
    return call


def tracker_rows(dev, frames, order, launches, parent, embeds=None):
    """One row per mode on the same frames; every row starts from an empty state."""
    p = yt.params()
    rows = {}

    def run(name, step, reid=False):
        state = yt.track_state(B, MT, dev, reid_dim=DIM if reid else None)
        out = yt.Tracks(torch.empty((B, MD, 6), device=dev), torch.empty((B, MD), dtype=torch.int32, device=dev),
                        torch.empty((B, MD), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
        at = [0]

        def block():
            for _ in range(BLOCK):
                k = order[at[0] % len(order)]
                at[0] += 1
                step(k, state, out)
        rows[name] = timed(block, launches)
        rows[name]["out_rows_per_stream"] = round(float(out.counts.float().mean()), 1)
        st = state[:, 4:4 + MT].cpu()
        rows[name]["tracked_per_stream"] = round(float((st == 2).sum()) / B, 1)

    if parent is not None:
        run("greedy_parent", lambda k, st, out: parent(frames[k][0], frames[k][1], st, p, out))
    for mode in ("greedy", "optimal"):
        run(mode, lambda k, st, out, mode=mode: yt.track(frames[k][0], frames[k][1], st, p, out=out, assign=mode))
    if parent is not None:                       # once more behind the others: the spread of one build
        run("greedy_parent_again", lambda k, st, out: parent(frames[k][0], frames[k][1], st, p, out))
    if embeds is not None:
        ws = yt.reid_workspace(B, MD, MT, DIM, dev)
        for mode in ("greedy", "optimal"):
            run("reid_" + mode, lambda k, st, out, mode=mode: yt.track_reid(
                frames[k][0], frames[k][1], st, embed=embeds[k], dim=DIM, p=p, out=out, workspace=ws, assign=mode),
                reid=True)
    g = rows["greedy"]["us_median"]
    rows["optimal_over_greedy"] = round(rows["optimal"]["us_median"] / g, 2)
    if embeds is not None:
        rows["reid_optimal_over_reid_greedy"] = round(rows["reid_optimal"]["us_median"] / rows["reid_greedy"]["us_median"], 2)
    return rows


def video_embeds(dev, frames, seed):
    """One feature per row: the prototype of the box's size bucket plus noise, so that neighbours
    often look alike; (B * MD, DIM) per frame, built on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    protos = torch.randn((64, DIM), device=dev, generator=g)
    out = []
    for d, _ in frames:
        bucket = ((d[..., 2] - d[..., 0]) / 8).long().clamp(0, 63).reshape(-1)
        out.append((protos[bucket] + 0.3 * torch.randn((B * MD, DIM), device=dev, generator=g)).contiguous())
    return out


def solver_rows(dev, launches):
    import _assign_cases as ac
    cases = ac.solver_cases()
    rng = np.random.default_rng(0)
    problems = {
        "sparse_256x300": np.stack([ac.sparse(256, 300, 100 + s) for s in range(32)]),
        "dense_128x128": np.stack([rng.choice([0, 10, 20, 30], (128, 128), p=[0.1, 0.3, 0.3, 0.3]).astype(np.int32)
                                   for _ in range(32)]),
        "dense_random_128x128": rng.integers(1, ac.M + 1, (32, 128, 128)).astype(np.int32),
    }
    assert cases["sparse_256x300"][0].shape[1:] == (256, 300) and cases["ties_128"][0].shape[1:] == (128, 128)
    rows = {}
    for name, w in problems.items():
        on = torch.from_numpy(w).to(dev)
        out = yolo_hip.assign(on)

        def block():
            for _ in range(BLOCK):
                yolo_hip.assign(on, out=out)
        rows[name] = timed(block, launches)
        rows[name]["matched_per_problem"] = round(float((out[0] >= 0).sum()) / 32, 1)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=400)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.lib()
    parent = parent_track(args.parent_lib) if args.parent_lib else None
    res = dict(shape=f"{B} streams x {MD} rows, max_tracks {MT}, blocks of {BLOCK} launches", video={})
    order = list(range(BLOCK)) + list(range(BLOCK - 2, 0, -1))
    for objects in (50, 250):
        frames = [(d.to(dev), c.to(dev)) for d, c in tb.video(objects, 1)]
        res["video"][str(objects)] = tracker_rows(dev, frames, order, args.launches, parent,
                                                  embeds=video_embeds(dev, frames, objects))
    eng = tb.engines(1, dev)[0]
    xs = [synth.synth_scenes(B, S, S, seed=100 + 1000 * k).to(dev, tb.DT) for k in range(4)]
    scenes = [nms(eng.forward(x)) for x in xs]
    res["unrelated_scenes"] = tracker_rows(dev, scenes, list(range(4)), args.launches, parent)
    res["yh_assign"] = solver_rows(dev, args.launches)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "assign_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
