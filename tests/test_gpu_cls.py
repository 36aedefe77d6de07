"""The classifier on the GPU (yh_create_cls / yh_classify; csrc/cls.hip). Marked gpu.

Cases (tests/_cls_cases.py CASES): the smallest shapes at which the head can still go wrong - 1, 4,
8, 15, 49 and 100 pixels per image at p5, width[5] of 256 and 512, 3 / 10 / 1000 classes, images that
share or straddle the fused head's 32-pixel row tiles, a batch beyond one workgroup's images.

Bars. `a` (head.conv's output) is held to the project's single-layer bar: at most 0.1 % of outputs
beyond one ulp of the dtype from the fp64 conv of the device's own input. The mean's bound
(HW + 2) * 2^-24 * mean_p |a| is the worst case of an fp32 sum of HW terms in any order plus the
scale and its rounding; the logits' 1282 * 2^-24 * (|W| |e| + |b|) is the same for a 1280-term dot
product and the bias. The probabilities get 4 x the deviation of torch's own fp32 CPU softmax on
the same logits (room for the device's exponential), not below 2^-23. End to end against the module
in fp64: the fp32 handle within 1e-3 (the project's fp32 bar), the 16-bit handles within mean 2 x /
max 3 x the deviation of the same module run on the CPU in that dtype (test_gpu_forward.py's factors).
"""
import functools
import os
from ctypes import c_void_p

import pytest
import torch

import _cls_cases as cc
from yolo_hip import _lib
from yolo_hip.engine import Engine

pytestmark = pytest.mark.gpu

HALF = [c for c in cc.CASES if c[1] != torch.float32]
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
EMIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}


def _engine(model, dtype, dev, **env):
    """A classifier engine built with the given YH_* settings in the environment at handle creation."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(*model._yh_arch, dev, dtype, task="classify")
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_module(model)
    return eng


@functools.lru_cache(maxsize=None)
def _setup(case):
    """Per case, once: the engine with the fused head (YH_CLSHEAD=1), the per-layer engine (YH_CLSHEAD=0;
    the same engine on the fp32 handle, which has no fused head), the uint8 input and both outputs."""
    variant, dtype, nc, batch, h, w = case
    dev = torch.device("cuda", 0)
    model = cc.make_model(variant, nc)
    x = cc.inputs(batch, h, w).to(dev)
    fused = _engine(model, dtype, dev, YH_CLSHEAD="1")
    plain = fused if dtype == torch.float32 else _engine(model, dtype, dev, YH_CLSHEAD="0")
    out_f = tuple(t.clone() for t in fused.classify(x, logits=True, embed=True))
    out_p = out_f if plain is fused else tuple(t.clone() for t in plain.classify(x, logits=True, embed=True))
    return dict(model=model, x=x, fused=fused, plain=plain, out_f=out_f, out_p=out_p)


def _ops(eng, case):
    _, _, _, batch, h, w = case
    n = _lib.lib().yh_op_count(eng._h)
    return [eng.debug_op_desc(i, batch, h, w) for i in range(n)]


def _ulp(ref, dtype):
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** EMIN[dtype])))
    return torch.exp2(e - MANT[dtype])


@pytest.mark.parametrize("case", HALF, ids=cc.case_id)
def test_fused_equals_per_layer(gpu, case):
    s = _setup(case)
    _, _, _, batch, h, w = case
    kf = {o["label"]: o for o in s["fused"].ops(batch, h, w)}
    kp = {o["label"]: o for o in s["plain"].ops(batch, h, w)}
    assert kf["head.conv+pool"]["kernel"] == "cls_head" and kf["head.conv+pool"]["cls"] == "cls"
    assert "head.conv+pool" not in kp and kp["head.pool"]["kernel"] == "cls_pool"
    act_f = {d["label"]: d["active"] for d in _ops(s["fused"], case)}
    act_p = {d["label"]: d["active"] for d in _ops(s["plain"], case)}
    assert act_f["head.conv+pool"] == 1 and act_f["head.conv"] == 0 and act_f["head.pool"] == 0
    assert act_p["head.conv"] == 1 and act_p["head.pool"] == 1
    for name, a, b in zip(("probs", "logits", "embed"), s["out_f"], s["out_p"]):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    # the default is the per-layer head (it measured faster), and YH_FUSE=0 has no fused head either
    for env in ({}, {"YH_FUSE": "0", "YH_CLSHEAD": "1"}):
        labels = [o["label"] for o in _engine(s["model"], case[1], gpu, **env).ops(batch, h, w)]
        assert "head.pool" in labels and "head.conv+pool" not in labels


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_batch_invariance_graph_and_input_kind(gpu, case):
    s = _setup(case)
    _, dtype, _, batch, h, w = case
    eng, x = s["fused"], s["x"]
    for i in sorted({0, batch // 2, batch - 1}):
        one = eng.classify(x[i:i + 1], logits=True, embed=True)
        for name, a, b in zip(("probs", "logits", "embed"), one, s["out_f"]):
            assert torch.equal(a[0], b[i]), (name, i, (a[0] - b[i]).abs().max().item())
    eng.set_graph(False)
    try:
        eager = eng.classify(x, logits=True, embed=True)
    finally:
        eng.set_graph(True)
    xf = x.to(dtype) / 255
    conv = eng.classify(xf, logits=True, embed=True)
    for name, a, b, c in zip(("probs", "logits", "embed"), s["out_f"], eager, conv):
        assert torch.equal(a, b), ("graph vs eager", name)
        assert torch.equal(a, c), ("uint8 vs dtype input", name)


def _taps(case):
    """The head's operands of the per-layer engine, read back through the parity taps: f (head.conv's
    input), a (its output), e and z, all on the CPU."""
    s = _setup(case)
    _, _, nc, batch, h, w = case
    eng = s["plain"]
    _, logits, embed = s["out_p"]
    descs = {d["label"]: d for d in _ops(eng, case)}
    dc, dp, dl = descs["head.conv"], descs["head.pool"], descs["head.linear"]
    roles = lambda d: [o["role"] for o in d["operands"]]
    assert roles(dc) == ["in0", "out"] and roles(dp) == ["a", "e"] and roles(dl) == ["e", "z"]
    f = eng.debug_operand(dc["index"], 0, batch, dc).cpu()
    a = eng.debug_operand(dp["index"], 0, batch, dp).cpu()
    e = eng.debug_operand(dp["index"], 1, batch, dp).cpu()
    z = eng.debug_operand(dl["index"], 1, batch, dl).cpu()
    assert tuple(a.shape) == (batch, h // 32, w // 32, 1280) and e.dtype == torch.float32 and z.dtype == torch.float32
    assert torch.equal(a, eng.debug_operand(dc["index"], 1, batch, dc).cpu())
    assert torch.equal(e.reshape(batch, 1280), embed.cpu()) and torch.equal(z.reshape(batch, -1)[:, :nc], logits.cpu())
    return f, a, e


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_head_conv_on_device_input(gpu, case):
    """a = head.conv(f) against the fp64 conv (folded weights rounded to the dtype, bias, SiLU) of
    the device's own f: at most 0.1 % of the outputs beyond one ulp of the dtype.

    Measured on an MI355X: bf16 0.0000 - 0.0008 %, fp16 0.003 - 0.009 %, fp32 0.0000 % of the outputs
    beyond one ulp. The fp32 handle meets the bar because head.conv's bias and SiLU run on the fp64
    accumulator (ACT_SILU_F64, conv.hip): with the fp32 epilogue every other fp32 conv has (the
    rounded K sum, then expf, an add and a division in fp32) it cannot. The reference folds the
    BatchNorm in IEEE fp32 as the library does (_cls_cases.folded_head_conv); DESIGN.md §15."""
    variant, dtype, nc, batch, h, w = case
    f, a, _ = _taps(case)
    hw = (h // 32) * (w // 32)
    wc, bc, _, _ = cc.folded_head_conv(variant, nc)
    pre = f.double().reshape(batch * hw, -1) @ wc.to(dtype).double().t() + bc.double()
    ref_a = pre * torch.sigmoid(pre)
    dev_a = a.double().reshape(batch * hw, 1280)
    beyond = ((dev_a - ref_a).abs() > _ulp(torch.maximum(ref_a.abs(), dev_a.abs()), dtype)).double().mean().item()
    print(f"a: {100 * beyond:.4f} % beyond one ulp")
    assert beyond <= 1e-3


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_pool_linear_softmax_on_device_inputs(gpu, case):
    """The mean, the linear layer and the softmax, each against fp64 on the stage's own device input.
    Measured on an MI355X (max over the cases): DESIGN.md §15."""
    s = _setup(case)
    variant, dtype, nc, batch, h, w = case
    probs, logits, _ = s["out_p"]
    _, a, e = _taps(case)
    hw = (h // 32) * (w // 32)
    _, _, wl, bl = cc.folded_head_conv(variant, nc)
    dev_a = a.double().reshape(batch * hw, 1280)

    # e: the mean of the device's own a
    a3 = dev_a.reshape(batch, hw, 1280)
    d_e = (e.double().reshape(batch, 1280) - a3.mean(1)).abs()
    bound_e = (hw + 2) * 2.0 ** -24 * a3.abs().mean(1)
    print(f"embed: max |d| / bound {(d_e / bound_e.clamp_min(1e-300)).max().item():.3f}")
    assert (d_e <= bound_e).all()

    # z: the linear layer on the device's own e
    w16, e64 = wl.to(dtype).double(), e.double().reshape(batch, 1280)
    ref_z = e64 @ w16.t() + bl.double()
    d_z = (logits.cpu().double() - ref_z).abs()
    bound_z = 1282 * 2.0 ** -24 * (e64.abs() @ w16.abs().t() + bl.double().abs())
    print(f"logits: max |d| / bound {(d_z / bound_z).max().item():.5f}")
    assert (d_z <= bound_z).all()

    # probs: the softmax of the device's own logits
    z32 = logits.cpu()
    ref_p = torch.softmax(z32.double(), 1)
    torch_dev = (torch.softmax(z32, 1).double() - ref_p).abs().max().item()
    d_p = (probs.cpu().double() - ref_p).abs().max().item()
    bar = max(4 * torch_dev, 2.0 ** -23)
    print(f"probs: max |d| {d_p:.3e} (torch fp32 CPU softmax {torch_dev:.3e}, bar {bar:.3e})")
    assert d_p <= bar
    assert torch.allclose(probs.sum(1), torch.ones(batch, device=probs.device), atol=1e-5)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_end_to_end_against_fp64_module(gpu, case):
    s = _setup(case)
    variant, dtype, nc, batch, h, w = case
    ref = cc.reference(variant, nc, batch, h, w)
    names = ("probs", "logits", "embed")
    which = names if nc == 1000 else ("embed",)
    dev = {n: (t.cpu().double() - r).abs() for n, t, r in zip(names, s["out_f"], ref)}
    if dtype == torch.float32:
        for n in which:
            print(f"{n}: fp32 max |d| {dev[n].max().item():.3e}")
        assert dev["embed"].max().item() <= 1e-3
        if nc == 1000:
            assert dev["logits"].max().item() <= 1e-3
        return
    cpu = {n: (t - r).abs() for n, t, r in zip(names, cc.cpu_in_dtype(variant, nc, batch, h, w, dtype), ref)}
    for n in which:
        print(f"{n}: device mean {dev[n].mean().item():.3e} max {dev[n].max().item():.3e} | "
              f"CPU {str(dtype).split('.')[-1]} mean {cpu[n].mean().item():.3e} max {cpu[n].max().item():.3e}")
    for n in which:
        assert dev[n].mean().item() <= 2.0 * cpu[n].mean().item(), n
        assert dev[n].max().item() <= 3.0 * cpu[n].max().item(), n


@pytest.mark.parametrize("case", [cc.CASES[3], cc.CASES[6]], ids=cc.case_id)
def test_count_masks_rows(gpu, case):
    s = _setup(case)
    _, _, nc, batch, _, _ = case
    eng, x = s["fused"], s["x"]
    full = s["out_f"]
    for cnt in (None, 0, 2, batch, batch + 5, -1):
        out = (torch.full((batch, nc), 7.5, device=gpu), torch.full((batch, nc), 7.5, device=gpu),
               torch.full((batch, 1280), 7.5, device=gpu))
        count = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=gpu)
        got = eng.classify(x, count=count, logits=True, embed=True, out=out)
        n = batch if cnt is None else min(max(cnt, 0), batch)
        for name, g, want in zip(("probs", "logits", "embed"), got, full):
            assert torch.equal(g[:n], want[:n]), (cnt, name)
            assert not g[n:].any(), (cnt, name)
    # outputs that were not asked for are not required
    only = eng.classify(x)
    assert only[1] is None and only[2] is None and torch.equal(only[0], full[0])


def test_wrong_handle_kind(gpu):
    from _util import make_model
    L = _lib.lib()
    det = make_model("n")
    deng = Engine(*det._yh_arch, gpu, torch.bfloat16)
    deng.load_module(det)
    s = _setup(cc.CASES[3])
    ceng, x = s["fused"], s["x"]
    probs = torch.full((5, 3), 7.5, device=gpu)
    stream = c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = L.yh_classify(deng._h, c_void_p(x.data_ptr()), 1, 5, 32, 32, None, c_void_p(probs.data_ptr()), None, None, stream)
    assert rc == -2 and b"yh_classify" in L.yh_last_error()
    y = torch.full((5, 7, 21), 7.5, device=gpu, dtype=torch.bfloat16)
    for fwd in (L.yh_forward, L.yh_forward_u8):
        rc = fwd(ceng._h, c_void_p(x.data_ptr()), 5, 32, 32, c_void_p(y.data_ptr()), stream)
        assert rc == -2 and b"classifier handle" in L.yh_last_error()
    with pytest.raises(RuntimeError, match="classifier handle"):
        ceng.num_anchors(32, 32)
    with pytest.raises(RuntimeError, match="task='classify'"):
        deng.classify(x)
    torch.cuda.synchronize()
    assert (probs == 7.5).all() and (y == 7.5).all()   # nothing was launched
    # a size that is no multiple of 32 is refused before anything runs
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ceng.classify(torch.zeros((1, 3, 48, 32), dtype=torch.uint8, device=gpu))


def test_dropin_module_runs_hip_path(gpu):
    """YOLOCls.forward / features on a cuda tensor in eval mode go through the engine."""
    s = _setup(cc.CASES[3])
    m = cc.make_model("n", 3).to(gpu)
    xf = s["x"].to(torch.bfloat16) / 255
    with torch.no_grad():
        p = m(xf)
        pf, z, e = m.features(xf)
    assert p.dtype == torch.bfloat16 and "_yh_engines" in m.__dict__
    assert torch.equal(pf, s["out_f"][0]) and torch.equal(z, s["out_f"][1]) and torch.equal(e, s["out_f"][2])
    assert torch.equal(p, pf.to(torch.bfloat16))
