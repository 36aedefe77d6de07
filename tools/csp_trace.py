"""csp_fused phase stamps (YH_LIB=<library built with make EXTRA=-DYH_CSP_TRACE>).

python tools/csp_trace.py [variant] [batch] [size]

Runs graph-replayed forwards of the bench configuration (v11_n, bf16, batch 32, 640^2) and
prints, per fused C3k2 launch, the cycles wave 0 of a workgroup spends per stage of a tile
(median over workgroups and tiles; the first tile of a workgroup, which also waits for the
parameter image, is left out). YH_CSP_TILE / YH_CSP_TAIL apply as in the engine.
"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "yolo-infer-pt_amd"))

from yolo_hip import synth  # noqa: E402
from yolo_hip.engine import Engine  # noqa: E402

TR, TILES, WG, OPS = 12, 16, 256, 4
INST = ["(2,1,2)", "(4,2,4)", "(0,2,2)", "(0,2,4)"]   # YH_CSP_LIST order
COLS = ["topwait", "topbar", "P1", "P1bar", "P2", "P2bar", "P3", "P3bar", "P4", "tile"]


def main():
    v = sys.argv[1] if len(sys.argv) > 1 else "n"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 640
    from nets import nn
    torch.manual_seed(0)
    model = getattr(nn, f"yolo_v11_{v}")(80)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0))
    model.eval()
    dev = torch.device("cuda", 0)
    eng = Engine(*model._yh_arch, dev, torch.bfloat16)
    eng.load_module(model)
    x = synth.synth_scenes(B, size, size, seed=3).to(dev, torch.bfloat16)
    y = eng.forward(x)
    for _ in range(3):
        eng.forward(x, out=y)
    torch.cuda.synchronize()
    for o in eng.ops(B, size, size):
        if o["cls"] == "c3k2":
            print(f"op {o['label']:16s} {o['kernel']}")
    lib = ctypes.CDLL(os.environ["YH_LIB"])
    n = OPS * WG * TILES * TR
    buf = np.zeros(n, dtype=np.uint64)
    rc = lib.yh_debug_csp_trace(ctypes.c_void_p(buf.ctypes.data), ctypes.c_int(n))
    assert rc == 0, rc
    t = buf.reshape(OPS, WG, TILES, TR).astype(np.int64)
    print("cycles of wave 0 per tile, median (p90); *bar = wait at the barrier that ends the stage")
    print(f"{'inst':8s} {'tile':>6s} {'wgs':>4s} {'t/wg':>5s} " + " ".join(f"{c:>13s}" for c in COLS) + "   cyc/us")
    for k in range(OPS):
        r = t[k]
        used = r[:, :, 11] > 0
        if not used.any():
            continue
        th, tw = int(r[used][0, 11] & 0xffff), int((r[used][0, 11] >> 16) & 0xffff)
        per_wg = used.sum(axis=1)
        # tiles 1.. of a workgroup, and only those followed by another tile (its top stamp ends the tile)
        ok = used.copy()
        ok[:, 0] = False
        nxt = np.zeros_like(used)
        nxt[:, :-1] = used[:, 1:]
        ok &= nxt
        if not ok.any():   # one tile per workgroup: take what there is, without the tile total
            ok = used
        r = r.copy()
        for c in (3, 4):                                         # tail mode has no P1: zero-width columns
            r[:, :, c] = np.where(r[:, :, c] == 0, r[:, :, 2], r[:, :, c])
        d = np.diff(r[:, :, 0:10], axis=2)                       # 9 stage columns
        tile = np.zeros(r.shape[:2], dtype=np.int64)
        tile[:, :-1] = r[:, 1:, 0] - r[:, :-1, 0]                # top to next top
        cols = np.concatenate([d, tile[:, :, None]], axis=2)[ok]
        med, p90 = np.median(cols, axis=0), np.percentile(cols, 90, axis=0)
        cyc = (r[:, 1:, 0] - r[:, :-1, 0])[nxt[:, :-1] & used[:, :-1]].astype(np.float64)
        us = (r[:, 1:, 10] - r[:, :-1, 10])[nxt[:, :-1] & used[:, :-1]] * 1e-2
        clk = np.median(cyc[us > 0] / us[us > 0]) if (us > 0).any() else float("nan")
        print(f"{INST[k]:8s} {th:>3d}x{tw:<3d}{(per_wg > 0).sum():>4d} {per_wg.max():>5d} " +
              " ".join(f"{m:6.0f}({p:5.0f})" for m, p in zip(med, p90)) + f"   {clk:6.0f}")


if __name__ == "__main__":
    main()
