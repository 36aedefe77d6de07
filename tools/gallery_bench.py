"""What an identity search costs: yh_gallery_search over a gallery of 1280-element int8 features
(the classifier's embedding), capacity 65 536 and 1 048 576, 64 and 512 queries, k = 1 and 8.

  python tools/gallery_bench.py [--out DIR] [--launches 60] [--limit 240]

Every GPU step (one shape) runs in a child process of its own under a time limit (--limit
seconds), and the first step that fails ends the run: nothing more is started on the device after
it. A step times, alternating in the same process, blocks of back-to-back calls between HIP-event
pairs of
  ours         yolo_hip.gallery_search (search kernel + merge of the chunks), full gallery;
  torch_bf16   torch.topk(q_bf16 @ gallery_bf16.T, k): the same answer up to bf16's rounding of
               the products' sum, the (nq, capacity) matrix written and read back;
  torch_int_mm torch.topk(torch._int_mm(q, gallery.T), k) where this build has it: exact.
and writes beside each figure the two floors of the shape: the gallery's bytes at 6.3 TB/s (the
achievable HBM rate) and the products at 5 Pop/s (the dense int8 MFMA rate, twice bf16's 2.5).
The first 8 queries are checked against an fp32 product of the same operands (exact on this
data: every partial sum stays below 2^24).

The per-kernel split comes from a run of its own:
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- \
      python tools/gallery_bench.py --part trace --capacity 1048576 --nq 512 --k 8

Prints one JSON object; --out also keeps it (gallery_bench.json).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 1280
HBM_BPS, INT8_OPS = 6.3e12, 5.0e15
SHAPES = [(c, nq, k) for c in (65536, 1048576) for nq in (64, 512) for k in (1, 8)]


def timed(call, block, pairs):
    """HIP-event pairs around `block` back-to-back calls -> us per call, and the host's time to
    queue one (where the two are close the device was waiting for the host)."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(pairs)]
    host = []
    for a, b in ev:
        a.record()
        t0 = time.perf_counter()
        for _ in range(block):
            call()
        host.append((time.perf_counter() - t0) * 1e6 / block)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 / block for a, b in ev], host


def summary(us, host, block):
    us, host = sorted(us), sorted(host)
    return dict(us_median=round(us[len(us) // 2], 1), us_min=round(us[0], 1), us_max=round(us[-1], 1),
                calls=len(us) * block, host_us_median=round(host[len(host) // 2], 1))


def operands(capacity, nq, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(capacity + nq)
    g = torch.randint(-128, 128, (capacity, DIM), dtype=torch.int8, device=dev, generator=gen)
    q = torch.randint(-128, 128, (nq, DIM), dtype=torch.int8, device=dev, generator=gen)
    return g, q


def child(capacity, nq, k, launches, trace):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))
    import yolo_hip
    dev = torch.device("cuda", 0)
    g, q = operands(capacity, nq, dev)
    labels = torch.zeros((capacity,), dtype=torch.int32, device=dev)
    size = torch.full((1,), capacity, dtype=torch.int32, device=dev)
    ws = yolo_hip.gallery_workspace(capacity, nq, k, device=dev)
    out = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.int32, device=dev))
    ours = lambda: yolo_hip.gallery_search(g, q, k, labels=labels, size=size, out=out, workspace=ws)
    ours()
    torch.cuda.synchronize()
    if trace:
        for _ in range(5):
            ours()
        torch.cuda.synchronize()
        return
    exact = torch.topk(q[:8].float() @ g.float().T, k, dim=1).values
    assert torch.equal(out[0][:8].float(), exact), "gallery_search differs from the fp32 product"
    block = 4 if capacity > 100000 else 10
    pairs = max(3, launches // block // 2)
    gb, qb = g.to(torch.bfloat16), q.to(torch.bfloat16)
    arms = {"ours": ours, "torch_bf16": lambda: torch.topk(qb @ gb.T, k, dim=1)}
    res = dict(capacity=capacity, nq=nq, k=k, dim=DIM, workspace_bytes=ws.numel())
    if hasattr(torch, "_int_mm"):
        try:
            torch.topk(torch._int_mm(q, g.T), k, dim=1)
            torch.cuda.synchronize()
            arms["torch_int_mm"] = lambda: torch.topk(torch._int_mm(q, g.T), k, dim=1)
        except Exception as e:   # this build has the symbol but not the kernel for these operands
            res["torch_int_mm"] = "unavailable: " + str(e).splitlines()[0][:200]
    else:
        res["torch_int_mm"] = "unavailable: no torch._int_mm"
    for call in arms.values():
        call()
    torch.cuda.synchronize()
    runs = {name: ([], []) for name in arms}
    for _ in range(2):                                   # alternating: ours, torch, ours, torch
        for name, call in arms.items():
            us, host = timed(call, block, pairs)
            runs[name][0].extend(us)
            runs[name][1].extend(host)
    for name, (us, host) in runs.items():
        res[name] = summary(us, host, block)
    tiles = (nq + 63) // 64
    res["floor_us_hbm"] = round(capacity * DIM / HBM_BPS * 1e6, 1)
    res["floor_us_mfma"] = round(2.0 * tiles * 64 * capacity * DIM / INT8_OPS * 1e6, 1)
    bound = max(res["floor_us_hbm"], res["floor_us_mfma"])
    res["binding_floor"] = "hbm" if res["floor_us_hbm"] >= res["floor_us_mfma"] else "mfma"
    res["times_the_floor"] = round(res["ours"]["us_median"] / bound, 2)
    res["gallery_tb_s"] = round(capacity * DIM / res["ours"]["us_median"] / 1e6, 2)
    res["int8_pops"] = round(2.0 * nq * capacity * DIM / res["ours"]["us_median"] / 1e9, 3)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--capacity", type=int, default=65536, help=argparse.SUPPRESS)
    ap.add_argument("--nq", type=int, default=64, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        return child(args.capacity, args.nq, args.k, args.launches, args.part == "trace")
    res = dict(dim=DIM, hbm_tb_s=HBM_BPS / 1e12, int8_pops=INT8_OPS / 1e15, steps=[])
    for capacity, nq, k in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", "time", "--capacity", str(capacity), "--nq", str(nq),
               "--k", str(k), "--launches", str(args.launches)]
        what = f"{capacity}/{nq}/{k}"
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"gallery_bench: step {what} ran into its time limit; nothing more is started")
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"gallery_bench: step {what} ended with status {p.returncode}; nothing more is started")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["steps"].append(json.loads(line[7:]))
        sys.stderr.write(f"{what} done\n")
    line = json.dumps(res)
    print(line)
    out_dir = args.out or os.path.join(ROOT, "build", "gallery_bench")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "gallery_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
