"""What re-identification costs, at the tracker bench's shape (32 video streams x 300 NMS rows,
max_tracks 256) with 1280-element features (the classifier's embedding) on the high rows only.

  python tools/reid_bench.py [--out DIR] [--launches 400] [--limit 240]

Every GPU step runs in a child process of its own under a time limit (--limit seconds), and the
first step that fails ends the run: nothing more is started on the device after it.

  sim    yh_embed_similarity alone: the galleries where they lie in the tracker state (through
         stream ids) against the frame's quantised features, (32, 256, 1280) x (32, 300, 1280)
         int8 -> (32, 256, 300) int32; and, as a cost baseline from outside this project, torch
         eager bmm of the same operands in bf16;
  quant  yh_embed_quantize alone on one frame's features;
  track  yh_track_reid whole (quantise-and-scatter, similarity, track kernel, gallery update)
         against yh_track on the same frames, alternating blocks in the same process.
Each for about 50 and about 250 tracked objects per stream. Times are medians and min - max of
HIP-event pairs around blocks of 40 back-to-back launches, with the host's time to queue a call
beside them: where the two are close the device was waiting for the host.

Prints one JSON object; --out also keeps it (reid_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, MD, MT, DIM = 32, 640, 300, 256, 1280
BLOCK = 40      # frames of the sequence = launches per event pair


def video(objects, seed):
    """BLOCK frames of (dets (B, MD, 6), counts (B,), embed (sum of feat_counts, DIM), feat_counts
    (B,)): tools/track_bench.py's video - `objects` boxes per stream on straight lines, a fifth of
    the scores in the low band, clutter below track_low up to MD rows, rows in score order - where
    every object has a feature of its own (a random direction plus a fifth of noise per frame) and
    the rows with score >= 0.25 carry it."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    pos = rng.uniform(60, S - 60, (B, objects, 2))
    vel = rng.uniform(-1.5, 1.5, (B, objects, 2))
    wh = rng.uniform(20, 90, (B, objects, 2))
    cls = rng.integers(0, 8, (B, objects)).astype(np.float64)
    proto = rng.normal(0, 1, (B, objects, DIM)).astype(np.float32)
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
        fc = (rows[..., 4] >= 0.25).sum(1).astype(np.int32)         # a prefix: the rows are sorted
        feats = [proto[b, order[b, :fc[b]]] + rng.normal(0, 0.2, (fc[b], DIM)).astype(np.float32) for b in range(B)]
        frames.append((torch.from_numpy(rows.astype(np.float32)), torch.full((B,), MD, dtype=torch.int32),
                       torch.from_numpy(np.concatenate(feats)), torch.from_numpy(fc)))
    return frames


def timed(block, launches):
    """Medians of HIP-event pairs around `block` (BLOCK launches each) -> us per launch."""
    import torch
    block()
    torch.cuda.synchronize()
    n = max(3, launches // BLOCK)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    host = []
    for a, b in ev:
        a.record()
        t0 = time.perf_counter()
        block()
        host.append((time.perf_counter() - t0) * 1e6 / BLOCK)
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / BLOCK for a, b in ev)
    # host_us_median: what the host needs to queue one call; where it is close to us_median the
    # device waits for the host and us_median is not the kernels' time
    return dict(us_median=round(us[n // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2), launches=n * BLOCK,
                host_us_median=round(sorted(host)[n // 2], 2))


def warm_tracker(dev, frames):
    """A reid Tracker that has seen the sequence once: its galleries are full."""
    from yolo_hip import track as yt
    trk = yt.Tracker(B, dev, max_tracks=MT, reid_dim=DIM)
    for d, c, e, fc in frames:
        trk.update(d, c, embed=e, feat_counts=fc)
    return trk


def child(part, objects, launches):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))
    import yolo_hip
    from yolo_hip import track as yt
    dev = torch.device("cuda", 0)
    frames = [tuple(t.to(dev) for t in f) for f in video(objects, 1)]
    order = list(range(BLOCK)) + list(range(BLOCK - 2, 0, -1))        # there and back again
    res = dict(part=part, objects=objects, features_per_stream=round(float(frames[0][3].float().mean()), 1))
    if part == "quant":
        e = frames[0][2]
        out = torch.empty(e.shape, dtype=torch.int8, device=dev)
        res.update(timed(lambda: [yolo_hip.embed_quantize(e, out=out) for _ in range(BLOCK)], launches))
        res["rows"] = e.shape[0]
        res["gb_s"] = round(e.numel() * 5 / res["us_median"] / 1e3, 1)
    elif part == "sim":
        trk = warm_tracker(dev, frames)
        words = trk.state.shape[1]
        gal = trk.state.view(torch.int8)[:, 4 * (4 + 24 * MT):].view(B, MT, DIM)     # the galleries, in place
        assert gal.stride(0) == 4 * words and gal.data_ptr() == trk.state.data_ptr() + 4 * (4 + 24 * MT)
        d, c, e, fc = frames[-1]
        q = torch.zeros((B, MD, DIM), dtype=torch.int8, device=dev)
        qe = yolo_hip.embed_quantize(e)
        at = 0
        for b, n in enumerate(fc.tolist()):
            q[b, :n] = qe[at:at + n]
            at += n
        sid = torch.arange(B, dtype=torch.int32, device=dev)
        out = torch.empty((B, MT, MD), dtype=torch.int32, device=dev)
        res.update(timed(lambda: [yolo_hip.embed_similarity(gal, q, sid, out=out) for _ in range(BLOCK)], launches))
        res["live_gallery_rows_per_stream"] = round(float(gal.any(dim=2).float().sum(1).mean()), 1)
        ops = 2.0 * B * MT * MD * DIM
        byts = B * MT * DIM + B * MD * DIM + 4.0 * B * MT * MD
        res["int8_tops"] = round(ops / res["us_median"] / 1e6, 2)
        res["gb_s"] = round(byts / res["us_median"] / 1e3, 1)
        ga, qb = gal.to(torch.bfloat16).contiguous(), q.to(torch.bfloat16).transpose(1, 2).contiguous()
        ref = torch.empty((B, MT, MD), dtype=torch.bfloat16, device=dev)
        res["torch_bmm_bf16"] = timed(lambda: [torch.bmm(ga, qb, out=ref) for _ in range(BLOCK)], launches)
        exact = torch.bmm(gal.double().cpu(), q.double().cpu().transpose(1, 2))
        assert torch.equal(out.cpu().double(), exact)
    elif part == "track":
        trk = warm_tracker(dev, frames)
        plain = yt.Tracker(B, dev, max_tracks=MT)
        for d, c, e, fc in frames:
            plain.update(d, c)
        at = [0, 0]
        outs = [None, None]

        def block_reid():
            for _ in range(BLOCK):
                d, c, e, fc = frames[order[at[0] % len(order)]]
                at[0] += 1
                outs[0] = yt.track_reid(d, c, trk.state, embed=e, feat_counts=fc, p=trk.params, out=outs[0],
                                        workspace=trk._workspace)

        def block_plain():
            for _ in range(BLOCK):
                d, c, e, fc = frames[order[at[1] % len(order)]]
                at[1] += 1
                outs[1] = yt.track(d, c, plain.state, plain.params, out=outs[1])

        half = max(BLOCK * 3, launches // 2)
        a1, b1 = timed(block_reid, half), timed(block_plain, half)
        a2, b2 = timed(block_reid, half), timed(block_plain, half)
        res["track_reid"] = [a1, a2]
        res["track"] = [b1, b2]
        st = trk.state[:, 4:4 + MT].cpu()
        res["slots"] = dict(tracked=round(float((st == 2).sum()) / B, 1), lost=round(float((st == 3).sum()) / B, 1),
                            tentative=round(float((st == 1).sum()) / B, 1))
        res["out_rows_per_stream"] = round(float(outs[0].counts.float().mean()), 1)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--objects", type=int, default=50, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        return child(args.part, args.objects, args.launches)
    res = dict(shape=f"{B} streams x {MD} rows, max_tracks {MT}, dim {DIM}", steps=[])
    for part in ("quant", "sim", "track"):
        for objects in (50, 250):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--objects", str(objects),
                   "--launches", str(args.launches)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"reid_bench: step {part}/{objects} ran into its time limit; nothing more is started")
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"reid_bench: step {part}/{objects} ended with status {p.returncode}; nothing more is started")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["steps"].append(json.loads(line[7:]))
            sys.stderr.write(f"{part}/{objects} done\n")
    line = json.dumps(res)
    print(line)
    out_dir = args.out or os.path.join(ROOT, "build", "reid_bench")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "reid_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
