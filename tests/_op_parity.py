"""The op-by-op parity driver (TEST INFRASTRUCTURE ONLY), shared by tests/test_gpu_op_parity.py
(the bench configurations) and tests/test_gpu_op_parity_edges.py (small and rectangular maps).

run_op_parity() steps a forward one op at a time through the parity taps, hands each op's
device-produced operands to the interval oracle (tests/_opcheck.py) and asserts its bars; the
tables of those bars (OVER1_MAX, WIDTH_MAX) live here. The plain fp32 evaluations of single ops
(fp32_layer, fp32_attention, fp32_reference) are the oracle's own acceptance inputs in
tests/test_opcheck_cpu.py and the reference of the edge tests' over1 bar."""
import os

import torch
import torch.nn.functional as F

import _opcheck as oc
from _util import make_model
from yolo_hip import synth

IN_ROLES = ("in0", "in1", "res", "x0", "x1", "x2", "L0", "L1", "L2")
# kinds with a plain fp32 evaluation (fp32_reference): one layer, or layers the device
# materialises one by one
REF_KINDS = ("attention", "conv", "dwconv", "stem")


# ------------------------------------------------------------------ plain fp32 evaluations
def fp32_layer(x, desc, params, dtype, res=None):
    """Conv `desc` (+ SiLU, + Residual add) in torch's fp32 on the CPU, rounded to the dtype
    where the device rounds: the layer output and the residual sum."""
    w, b = params(desc)
    y = F.conv2d(x.float(), w.float(), b.float(), desc["s"], desc["k"] // 2, groups=desc["g"])
    if desc["act"]:
        y = F.silu(y)
    y = y.to(dtype)
    if res is not None:
        y = (y.float() + res.float()).to(dtype)
    return y


def fp32_attention(qkv, pe, params, dtype, heads, keys=None):
    """The attention op (qkv (B, heads * 128, H, W) -> (B, heads * 64, H, W)) in torch's fp32 on
    the CPU: exact softmax over all keys at once, the weights rounded to the dtype before P.V (as
    the device rounds them), the output rounded, + the positional DWConv `pe` of v, rounded.
    keys: optional (k, v) -> (k, v) applied to the keys and values the softmax sees (each
    (B, heads, c, T); the positional term keeps the map's own v): the mutations of
    tests/test_opcheck_cpu.py's sensitivity cases."""
    B, _, H, W = qkv.shape
    T = H * W
    t = qkv.float().reshape(B, heads, 128, T)
    q, k, v = t[:, :, :32], t[:, :, 32:64], t[:, :, 64:]
    ks, vs = (k, v) if keys is None else keys(k, v)
    s = torch.einsum("bhcq,bhck->bhqk", q, ks) * (32 ** -0.5)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = torch.einsum("bhqk,bhck->bhqc", p.to(dtype).float(), vs) / p.sum(-1, keepdim=True)
    o = o.to(dtype).float().permute(0, 1, 3, 2).reshape(B, heads * 64, H, W)
    pw, pb = params(pe)
    return (o + F.conv2d(v.reshape(B, heads * 64, H, W), pw.float(), pb.float(), 1, 1, groups=heads * 64)).to(dtype)


def fp32_reference(d, ins, x, params, dtype):
    """Op `d` (a kind of REF_KINDS) evaluated by the functions above on the operands the oracle
    gets: `ins` as in _check_op (the device's 16-bit values), x the input images."""
    kind = d["kind"]
    if kind == "stem":
        y = x
        for c in d["convs"]:
            y = fp32_layer(y, c, params, dtype)
        return y
    if kind == "dwconv":
        return fp32_layer(ins["in0"], d["convs"][0], params, dtype)
    if kind == "attention":
        return fp32_attention(ins["in0"], d["convs"][0], params, dtype, d["heads"])
    assert kind == "conv", kind
    conv = d["convs"][0]
    segs = []
    for o in d["operands"]:
        if o["role"].startswith("in"):
            t = ins[o["role"]][:, :o["logical"]]
            segs.append(t.repeat_interleave(2, 2).repeat_interleave(2, 3) if o["up"] else t)
    res = ins["res"][:, :conv["cout"]] if "res" in ins else None
    return fp32_layer(torch.cat(segs, 1), conv, params, dtype, res=res)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _anchor_off(l, H, W):
    return sum((H >> (3 + k)) * (W >> (3 + k)) for k in range(l))


def _bands(Ho):
    if Ho <= 24:
        return [(0, Ho)]
    m = Ho // 2 - 2
    return [(0, 4), (m, m + 4), (Ho - 4, Ho)]


def _check_op(d, ins, outs, x, y, H, W, nc, params, dtype, with_ref=False):
    """Stats of every output of op `d` (one entry per compared tensor): each output's interval
    and, with the error bounds dropped (oc.exact_values), its correctly rounded exact value.
    with_ref: for the kinds of REF_KINDS each entry also carries, under "ref", the stats of the
    plain fp32 evaluation of the op (fp32_reference) put through the same comparison."""
    kind = d["kind"]
    cases = []   # (what, device tensor, oracle function -> (lo, hi))
    refsel = {}  # what -> the compared part of the op's whole fp32 reference output
    if kind == "conv":
        conv = d["convs"][0]
        dev = _nchw(outs["out"])[:, :conv["cout"]]
        Ho = dev.shape[2]
        cost = dev.shape[0] * Ho * dev.shape[3] * conv["cout"] * conv["cin"] * conv["k"] ** 2
        if cost <= 3e9:
            cases.append(("out", dev, lambda: oc.conv_op(ins, d, params, dtype)))
        else:
            couts = None
            if conv["cout"] > 64:
                couts = torch.unique(torch.linspace(0, conv["cout"] - 1, 32).round().long())
            for r0, r1 in _bands(Ho):
                dv = dev[:, :, r0:r1]
                if couts is not None:
                    dv = dv[:, couts]
                cases.append((f"out rows {r0}-{r1}", dv,
                              lambda r0=r0, r1=r1: oc.conv_op(ins, d, params, dtype, rows=(r0, r1), couts=couts)))
                refsel[f"out rows {r0}-{r1}"] = lambda t, r0=r0, r1=r1: (t if couts is None else t[:, couts])[:, :, r0:r1]
    elif kind in ("stem", "stem_fused"):
        cases.append(("out", _nchw(outs["out"])[:, :d["convs"][-1]["cout"]],
                      lambda: oc.stem_op(x.double(), d, params, dtype)))
    elif kind == "dwconv":
        cases.append(("out", _nchw(outs["out"])[:, :d["convs"][0]["cout"]], lambda: oc.dw_op(ins, d, params, dtype)))
    elif kind == "sppf":
        cases.append(("out", _nchw(outs["out"]), lambda: oc.sppf_op(ins, d)))
    elif kind == "attention":
        cases.append(("out", _nchw(outs["out"]), lambda: oc.attention_op(ins, d, params, dtype, d["heads"])))
    elif kind == "c3k2":
        cases.append(("out", _nchw(outs["out"]), lambda: oc.csp_op(ins, d, params, dtype)))
    elif kind == "c3k":
        cases.append(("out", _nchw(outs["out"]), lambda: oc.c3k_op(ins, d, params, dtype)))
    elif kind == "head_cls":
        for l in range(3):
            if f"x{l}" not in ins:
                continue
            cv = d["convs"][5 * l:5 * l + 5]
            if d["direct"]:
                h, w = H >> (3 + l), W >> (3 + l)
                a0 = _anchor_off(l, H, W)
                dev = y[:, 4:4 + nc, a0:a0 + h * w].reshape(y.shape[0], nc, h, w)
                fn = lambda l=l, cv=cv: oc.rnd_iv(*oc.sigmoid_iv(*oc.head_cls_level(ins[f"x{l}"], cv, params, dtype)),
                                                  dtype)
                cases.append((f"level {l} scores", dev, fn))
            else:
                cases.append((f"level {l} logits", _nchw(outs[f"y{l}"])[:, :nc],
                              lambda l=l, cv=cv: oc.head_cls_level(ins[f"x{l}"], cv, params, dtype)))
    elif kind == "box_dfl":
        for l in range(3):
            h, w = H >> (3 + l), W >> (3 + l)
            a0 = _anchor_off(l, H, W)
            fn = lambda l=l: oc.dfl_box(*oc.layer(ins[f"x{l}"], ins[f"x{l}"], d["convs"][l], params, dtype), 8 << l,
                                        dtype)
            cases.append((f"level {l} boxes", y[:, 0:4, a0:a0 + h * w], fn))
    elif kind == "pw_chain":
        # stage by stage: inputs from the device operands (captured before the chain ran) or from
        # an earlier stage's output interval; compared where no later stage overwrote the output
        def chain_iv():
            iv = []
            for k, stg in enumerate(d["stages"]):
                conv = d["convs"][k]
                los, his = [], []
                for r in stg["runs"]:
                    if r["src"] < 0:
                        t = ins[f"s{k}.in{r['seg']}"][:, r["off"]:r["off"] + r["n"]]
                        los.append(t)
                        his.append(t)
                    else:
                        lo, hi = iv[r["src"]]
                        los.append(lo[:, r["soff"]:r["soff"] + r["n"]])
                        his.append(hi[:, r["soff"]:r["soff"] + r["n"]])
                res = None
                if stg["res"] == -1:
                    res = oc.exact(ins[f"s{k}.res"][:, :conv["cout"]])
                elif stg["res"] >= 0:
                    lo, hi = iv[stg["res"]]
                    o = stg["res_off"]
                    res = (lo[:, o:o + conv["cout"]], hi[:, o:o + conv["cout"]])
                iv.append(oc.layer(torch.cat(los, 1), torch.cat(his, 1), conv, params, dtype, res=res))
            return iv
        for k, stg in enumerate(d["stages"]):
            if stg["final"]:
                cases.append((f"stage {k} out", _nchw(outs[f"s{k}.out"])[:, :d["convs"][k]["cout"]],
                              lambda k=k: chain_iv()[k]))
    elif kind == "decode":
        for l in range(3):
            L = ins[f"L{l}"]
            h, w = H >> (3 + l), W >> (3 + l)
            a0 = _anchor_off(l, H, W)
            if l >= d["dlo"]:
                lg = L[:, 64:64 + nc]
                dev = y[:, 4:4 + nc, a0:a0 + h * w].reshape(y.shape[0], nc, h, w)
                cases.append((f"level {l} scores", dev, lambda lg=lg: oc.rnd_iv(*oc.sigmoid_iv(lg, lg), dtype)))
            if d["dbox"]:
                cases.append((f"level {l} boxes", y[:, 0:4, a0:a0 + h * w],
                              lambda L=L, l=l: oc.dfl_box(L[:, :64], L[:, :64], 8 << l, dtype)))
    else:
        raise AssertionError(f"no oracle for op kind {kind}")
    st = []
    f32 = fp32_reference(d, ins, x, params, dtype) if with_ref and kind in REF_KINDS else None
    for what, dev, fn in cases:
        lo, hi = fn()
        with oc.exact_values():
            ref, _ = fn()
        st.append(oc.compare(dev, lo, hi, ref, dtype, what))
        if f32 is not None:
            st[-1]["ref"] = oc.compare(refsel.get(what, lambda t: t)(f32), lo, hi, ref, dtype, what)
    return st


# Share of elements more than one ulp from the correctly rounded exact result, per op kind.
# Single-layer ops: 0.1 % (measured r05: at most 8e-5, the cancellation elements). Fused chains
# carry a layer's undecided roundings (1 ulp either way, both legitimate) into the next layer's
# K-sum, and attention rounds its softmax weights to the dtype for the P.V MFMA, so those kinds
# get a ceiling of about twice the largest share measured over C2 / n fp16 / C3 / C5 in r05
# (gpurun_out r5final2: c3k 4.8e-2, attention 1.04e-2, pw_chain 4.9e-3, c3k2 4.1e-3, head_cls
# 1.1e-3, stem_fused 8.6e-4): a regression that stays inside the (wider) propagated
# intervals still shows up here.
OVER1_MAX = {"c3k": 0.10, "attention": 0.025, "pw_chain": 0.012, "c3k2": 0.01, "head_cls": 0.003,
             "stem_fused": 0.002}
# Interval width (tests/_opcheck.py ulp_width: (hi - lo) in ulps of the dtype at the interval's
# magnitude; 0 = pinned, 1 = two adjacent values), (p50, p99) per op kind: the freedom the proven
# bound leaves a kernel. It is the oracle's looseness, not the device's error: the (2K + 4) u
# K-sum bound grows with K and with cancellation (|y| << sum |x w|), so the long 3x3 K-sums of C5
# (K up to 3456) reach p99 ~1800, and fused chains carry every layer's interval into the next
# (c3k: six layers, p50 ~1800). The device's own error is what over1 measures (share beyond one
# ulp of the correctly rounded exact value). Bounds: ~1.5x the r06 maxima over C2 / C2 unfused /
# n fp16 / C3 / C5 (round 6, run r6b), so a loosened oracle shows up as well.
# The fused kinds are pinned transitively rather than by their own intervals: each is bit-identical
# to its per-layer launches (tests/test_gpu_fusion.py), and those launches meet the single-layer
# bar (over1 <= 0.1 %, every element in its interval) at v11_n's shapes in test_op_parity_c2_unfused.
WIDTH_MAX = {"conv": (128, 2700), "stem": (1, 4), "dwconv": (1, 4), "decode": (1, 2), "box_dfl": (1, 2),
             "sppf": (0, 0), "stem_fused": (8, 360), "attention": (6, 240), "c3k2": (96, 2400),
             "c3k": (2700, 5300), "pw_chain": (600, 4200), "head_cls": (36, 128)}


def _handle(model, gpu, dtype, switches):
    """Engine made with the YH_* `switches` in the environment: every switch is read once, at
    handle creation, so the environment is put back before the first forward."""
    from yolo_hip.engine import Engine
    switches = {k: str(v) for k, v in (switches or {}).items()}
    assert all(k.startswith("YH_") for k in switches), switches
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        eng = Engine(*model._yh_arch, gpu, dtype)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_module(model)
    return eng


def run_op_parity(gpu, variant, dtype, batch, size, images, seed, height=None, width=None, kinds=None,
                  switches=None, ref_over1=False, width_max=None, report=None):
    """Step the forward of `variant` at (batch, height x width; size x size by default) op by op
    and check every active op's outputs of images `images` against the oracle.
    kinds: only ops of these kinds are evaluated (the others are still stepped, in order).
    switches: YH_* settings in force while the handle is made.
    ref_over1: the share beyond one ulp is not held to OVER1_MAX but, for the kinds of REF_KINDS,
    to the plain fp32 evaluation of the same op on the same operands (fp32_reference) put through
    the same comparison: that one must lie inside every interval itself, and the device's share
    may be at most twice its share + 3 / n (the project's factor of two over the reference's own
    noise: both are fp32 sums of the same terms in another order; 3 / n keeps an output of a few
    thousand elements from failing on one element). The other kinds' shares are printed only.
    width_max: per-kind (p50, p99) ceilings that replace WIDTH_MAX's for this run.
    report: a dict that receives "kernels" (label -> the kernel yh_op_kernel names, evaluated ops
    only) and "over1" (kind -> [(label, what, n, device share, reference share)]).
    Returns (the kinds evaluated, the number of elements compared)."""
    model = make_model(variant)
    params = oc.Params(model.state_dict(), dtype)
    H, W = height or size, width or size
    x = synth.synth_scenes(batch, H, W, seed=seed).to(gpu, dtype)
    eng = _handle(model, gpu, dtype, switches)
    y = eng.forward(x).clone()
    torch.cuda.synchronize()
    nc = eng.num_classes
    kernels = {i: o["kernel"] for i, o in enumerate(eng.ops(batch, H, W))}
    yd = torch.full_like(y, float("nan"))
    img = torch.tensor(images)
    x_sel = x[img].cpu()
    seen, failures = set(), []
    n_checked = 0
    if report is not None:
        report.update(kernels={}, over1={})
    for i in range(len(kernels)):
        d = eng.debug_op_desc(i, batch, H, W)
        if d["active"] != 1:
            continue
        if kinds is not None and d["kind"] not in kinds:
            eng.debug_run(x, yd, i, i + 1)
            continue
        ins = {}
        for s, o in enumerate(d["operands"]):
            if o["role"] in IN_ROLES or o["role"].split(".")[-1] in IN_ROLES:
                ins[o["role"]] = _nchw(eng.debug_operand(i, s, batch, d)[img].cpu()).double()
        eng.debug_run(x, yd, i, i + 1)
        outs = {}
        for s, o in enumerate(d["operands"]):
            if not (o["role"] in IN_ROLES or o["role"].split(".")[-1] in IN_ROLES):
                outs[o["role"]] = eng.debug_operand(i, s, batch, d)[img].cpu()
        torch.cuda.synchronize()
        st = _check_op(d, ins, outs, x_sel, yd[img].cpu(), H, W, nc, params, dtype, with_ref=ref_over1)
        seen.add(d["kind"])
        if report is not None:
            report["kernels"][d["label"]] = kernels[i]
        # the op kind's interval-width ceilings: a kind without an entry is a failure that names it
        wmax = (width_max or {}).get(d["kind"], WIDTH_MAX.get(d["kind"]))
        assert wmax is not None, f"op {d['label']}: no WIDTH_MAX entry for op kind {d['kind']!r}"
        w50, w99 = wmax
        for s in st:
            n_checked += s["n"]
            r = s.get("ref")
            print(f"{d['label']:<28} {kernels[i] or d['kind']:<36} {s['what']:<18} n={s['n']:<9} "
                  f"pinned {s['pinned']:.5f} exact {s['exact']:.5f} >1ulp {s['over1']:.2e} max_ulp {s['max_ulp']} "
                  f"width p50 {s['w50']:.2f} p99 {s['w99']:.2f} p99.9 {s['w999']:.1f} >4 {s['wide']:.2e} "
                  f"max {s['wmax']:.0f} bad {s['bad']}"
                  + (f" | fp32 ref >1ulp {r['over1']:.2e} max_ulp {r['max_ulp']} bad {r['bad']}" if r else ""))
            # every element within its proven interval; the share beyond one ulp and the
            # interval width under the op kind's ceilings (OVER1_MAX or the reference's, WIDTH_MAX)
            if not ref_over1:
                over = s["over1"] > OVER1_MAX.get(d["kind"], 1e-3)
            elif r:
                over = r["bad"] > 0 or s["over1"] > 2 * r["over1"] + 3 / s["n"]
            else:
                over = False
            if report is not None:
                report["over1"].setdefault(d["kind"], []).append(
                    (d["label"], s["what"], s["n"], s["over1"], r["over1"] if r else None))
            if s["bad"] or over or s["w50"] > w50 or s["w99"] > w99:
                failures.append((d["label"], kernels[i], s))
    assert not failures, failures[:4]
    # the stepped forward reproduces the graph forward bit for bit
    assert torch.equal(yd, y)
    return seen, n_checked
