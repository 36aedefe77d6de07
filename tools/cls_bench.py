"""What the second stage costs (yolo_hip.Classifier, yh_classify): v11_n classifier in bf16 on
device-resident uint8 crops - 512 and 3200 crops of 224 x 224 (max_batch 256), 512 crops of 128 x 64.

  python tools/cls_bench.py [--out DIR] [--blocks 7] [--calls 5] [--skip-baseline]

 (a) predict: crops per second of Classifier.predict, HIP events around blocks of `calls`
     back-to-back calls after warm-up (tuning and graph capture), median and min-max over the blocks.
 (b) baseline: the same torch module run by PyTorch eager in the same dtype on the same device
     (model.head(model.net(x)[2]) on crops.to(dtype) / 255, in the same chunks, bypassing the HIP
     dispatch). A cost baseline from outside this library.
 (c) head: per-op profiled microseconds of the fused head (cls_head) against head.conv + cls_pool
     (the default; the fused one is YH_CLSHEAD=1), two engines in one process, alternating, with the algorithmic bytes of both.

Every GPU step is a child process of this script under a time limit of its own; the first child
that fails or runs out of time ends the tool (its process group is killed, nothing is left on
the GPU). Prints one JSON object; --out also keeps it (cls_bench.json).
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORK = (("512x224x224", 512, 224, 224), ("3200x224x224", 3200, 224, 224), ("512x128x64", 512, 128, 64))
MAX_BATCH = 256
NC = 1000


def _summary(v, nd=1):
    v = sorted(v)
    return dict(median=round(statistics.median(v), nd), min=round(v[0], nd), max=round(v[-1], nd), n=len(v))


def _model():
    import _cls_cases as cc   # the tests' synthetic classifier weights
    return cc.make_model("n", NC)


def _crops(n, h, w, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(0)
    return torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)


def _timed(run, blocks, calls):
    import torch
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(blocks)]
    for a, b in ev:
        a.record()
        for _ in range(calls):
            run()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) / calls for a, b in ev]   # ms per call


def predict_child(blocks, calls):
    import torch
    from yolo_hip.classify import Classifier
    dev = torch.device("cuda", 0)
    cls = Classifier(_model(), dev, torch.bfloat16, max_batch=MAX_BATCH)
    res = {}
    for name, n, h, w in WORK:
        x = _crops(n, h, w, dev)
        ms = _timed(lambda: cls.predict(x), blocks, calls)
        out = cls.predict(x)
        res[name] = dict(ms_per_call=_summary(ms, 3), crops_per_s=_summary([n / (m * 1e-3) for m in ms], 0),
                         checksum=float(out.probs.sum().item()))
    print(json.dumps(dict(blocks=blocks, calls_per_block=calls, cases=res)))


def baseline_child(blocks, calls):
    import torch
    dev = torch.device("cuda", 0)
    model = _model().to(dev, torch.bfloat16)
    res = {}

    def run(x):
        with torch.no_grad():
            return torch.cat([model.head(model.net(x[s:s + MAX_BATCH].to(torch.bfloat16) / 255)[2])
                              for s in range(0, x.shape[0], MAX_BATCH)])
    for name, n, h, w in WORK:
        x = _crops(n, h, w, dev)
        ms = _timed(lambda: run(x), blocks, calls)
        res[name] = dict(ms_per_call=_summary(ms, 3), crops_per_s=_summary([n / (m * 1e-3) for m in ms], 0))
    print(json.dumps(dict(blocks=blocks, calls_per_block=calls, cases=res)))


def head_child(rounds, calls):
    import torch
    from yolo_hip.engine import Engine
    dev = torch.device("cuda", 0)
    model = _model()

    def engine(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            e = Engine(*model._yh_arch, dev, torch.bfloat16, task="classify")
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        e.load_module(model)
        return e
    engs = dict(fused=engine({"YH_CLSHEAD": "1"}), per_layer=engine({"YH_CLSHEAD": "0"}))
    res = {}
    for name, n, h, w in (("256x224x224", 256, 224, 224), ("512x224x224", 512, 224, 224), ("512x128x64", 512, 128, 64)):
        x = _crops(n, h, w, dev)
        us = {k: {} for k in engs}
        info = {k: {} for k in engs}
        for e in engs.values():
            e.classify(x)
            e.profile(True)
        for _ in range(rounds):
            for k, e in engs.items():
                e.profile_reset()
                for _ in range(calls):
                    e.classify(x)
                for o in e.ops(n, h, w):
                    if o["label"].startswith("head.") and o["calls"]:
                        us[k].setdefault(o["label"], []).append(o["ms"] * 1e3 / o["calls"])
                        info[k][o["label"]] = dict(kernel=o["kernel"], bytes=o["bytes"], flops=o["flops"])
        for e in engs.values():
            e.profile(False)
        res[name] = {k: {lab: dict(us=_summary(v, 2), **info[k][lab]) for lab, v in us[k].items()} for k in engs}
    print(json.dumps(dict(rounds=rounds, calls_per_round=calls, cases=res)))


def step(args, limit):
    """One GPU step: a fresh child of this script in a session of its own, killed as a group at `limit` s."""
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        raise SystemExit(f"cls_bench: step {args} exceeded {limit} s; process group killed")
    if proc.returncode != 0:
        raise SystemExit(f"cls_bench: step {args} exit {proc.returncode}\n{err[-1500:]}")
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child == "predict":
        return predict_child(args.blocks, args.calls)
    if args.child == "baseline":
        return baseline_child(args.blocks, args.calls)
    if args.child == "head":
        return head_child(args.blocks, args.calls)
    sub = ["--blocks", str(args.blocks), "--calls", str(args.calls)]
    res = dict(model="v11_n classifier, 1000 classes, bf16", max_batch=MAX_BATCH,
               predict=step(["--child", "predict"] + sub, 240), head=step(["--child", "head"] + sub, 180))
    if not args.skip_baseline:
        res["baseline"] = step(["--child", "baseline"] + sub, 240)
        res["predict_over_baseline"] = {
            k: round(v["crops_per_s"]["median"] / res["baseline"]["cases"][k]["crops_per_s"]["median"], 2)
            for k, v in res["predict"]["cases"].items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "cls_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
