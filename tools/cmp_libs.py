"""Two builds of the library on the same inputs: forward outputs bit for bit, the NMS of each (kept
rows and counts, bit for bit), and the host's view of the net (conv list, every op's description,
label, class, bytes, flops and kernel, the launch units).
usage: python tools/cmp_libs.py <libA> <libB> [i,j,..]   ('' = the in-tree library; i,j,..: indices
into SETTINGS, default all)

Each build runs in a child process, once per setting of SETTINGS, with YH_CONV=0 unless the caller
sets it (every conv on its first candidate plan: the kernel names then do not depend on the
autotuner's timings; the plans are bit-identical either way)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("n", "bf16", 4, 640), ("s", "fp16", 2, 320), ("n", "fp16", 2, 224), ("m", "bf16", 2, 480),
         ("n", "fp32", 2, 224), ("x", "bf16", 1, 256),
         ("n", "fp32", 1, 256)]   # 1344 anchors, a multiple of 8: head_decode<float, true> (224: 1029, ROWS = false)
SETTINGS = [{}, {"YH_FUSE": "0"}, {"YH_C3K": "0"}, {"YH_PWCHAIN": "0"}, {"YH_CSP_TAIL": "1"},
            # the attention kernels one by one (chunked, per wave, 16-wave full), the three max-pools
            {"YH_ATTN_FULL": "0"}, {"YH_ATTN_FULL": "0", "YH_ATTN_LDS": "0"},
            {"YH_ATTN_FULL": "1", "YH_ATTN_NW": "16", "YH_ATTN_QS": "1"}, {"YH_SPPF_FUSED": "0"}]
DTYPES = {"bf16": "bfloat16", "fp16": "float16", "fp32": "float32"}


def listing(eng, b, h, w):
    """What the library tells about the net at this shape, as plain data."""
    import ctypes
    from yolo_hip._lib import lib
    descs = []
    buf = ctypes.create_string_buffer(1 << 16)
    for i in range(lib().yh_op_count(eng._h)):
        n = lib().yh_debug_op_desc(eng._h, i, b, h, w, buf, len(buf))
        assert n >= 0, n
        descs.append(buf.value.decode())
    ops = [(o["label"], o["cls"], o["bytes"], o["flops"], o["kernel"]) for o in eng.ops(b, h, w)]
    units = []
    for i in range(lib().yh_unit_count(eng._h, b, h, w)):
        f, k, lv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = lib().yh_unit_info(eng._h, i, b, h, w, ctypes.byref(f), ctypes.byref(k), ctypes.byref(lv), None, None)
        assert rc == 0, rc
        units.append((f.value, k.value, lv.value))
    return {"convs": [tuple(c) for c in eng.convs], "descs": descs, "ops": ops, "units": units}


def child(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))
    import torch
    from yolo_hip import synth
    from yolo_hip.engine import Engine, nms
    from nets import nn
    res = {}
    for v, dt, b, sz in CASES:
        dtype = getattr(torch, DTYPES[dt])
        torch.manual_seed(0)
        model = getattr(nn, f"yolo_v11_{v}")(80)
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
        model.eval()
        dev = torch.device("cuda", 0)
        eng = Engine(*model._yh_arch, dev, dtype)
        eng.load_module(model)
        x = synth.synth_scenes(b, sz, sz, seed=34).to(dev, dtype)
        y = eng.forward(x)
        dets, counts = nms(y)
        torch.cuda.synchronize()
        dets = dets.cpu()
        for i, c in enumerate(counts.tolist()):
            dets[i, c:] = 0   # rows past the count are not written
        res[f"{v}_{dt}_{b}_{sz}"] = {"y": y.cpu(), "dets": dets, "counts": counts.cpu(),
                                     "listing": listing(eng, b, sz, sz)}
    torch.save(res, out)


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        return
    import torch
    bad = 0
    picked = [int(i) for i in sys.argv[3].split(",")] if len(sys.argv) > 3 else range(len(SETTINGS))
    for setting in (SETTINGS[i] for i in picked):
        print("setting:", " ".join(f"{k}={v}" for k, v in setting.items()) or "default", flush=True)
        outs = []
        for k, lib in enumerate(sys.argv[1:3]):
            env = dict(os.environ)
            env.pop("YH_LIB", None)
            if lib:
                env["YH_LIB"] = lib
            env.setdefault("YH_CONV", "0")
            env.update(setting)
            out = os.path.join(ROOT, "gpurun_out", f"cmp_{k}.pt")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run([sys.executable, __file__, "--child", out], env=env, check=True, timeout=600)
            outs.append(torch.load(out, weights_only=False))
        for key in outs[0]:
            a, b = outs[0][key], outs[1][key]
            same = torch.equal(a["y"], b["y"])
            diff = [f for f in a["listing"] if a["listing"][f] != b["listing"][f]]
            same_nms = torch.equal(a["counts"], b["counts"]) and torch.equal(a["dets"], b["dets"])
            bad += (not same) + bool(diff) + (not same_nms)
            la = a["listing"]
            print(" ", key, "bit-identical" if same else f"DIFFER max {(a['y'].float() - b['y'].float()).abs().max().item()}",
                  "|", f"nms {a['counts'].tolist()} kept:", "bit-identical" if same_nms else "DIFFER",
                  "|", f"{len(la['convs'])} convs, {len(la['ops'])} ops, {len(la['units'])} units:",
                  "listings equal" if not diff else f"LISTINGS DIFFER in {diff}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
