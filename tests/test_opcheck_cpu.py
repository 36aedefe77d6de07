"""The per-op interval oracle (tests/_opcheck.py) itself, on the CPU: it accepts an fp32
evaluation of each op (torch's own fp32 kernels, a different summation order than the
device's) rounded like the device rounds, and it rejects a one-ulp change of a pinned
element. Runs the oracle on the v11_n synthetic weights at small shapes. The fp32 evaluations
are tests/_op_parity.py's (fp32_layer, fp32_attention), the ones the GPU edge tests take their
over1 bar from.

test_attention_oracle_rejects_an_off_by_one_key_mask documents what the small-map GPU cases
(tests/test_gpu_op_parity_edges.py) can see: an attention that drops the last key, or counts one
key row past the last token, leaves its intervals at T = 4, 15, 49 and 55."""
import pytest
import torch

import _opcheck as oc
from _op_parity import fp32_attention
from _op_parity import fp32_layer as _fp32_layer
from _util import make_model


def _desc(name, model, act=1, s=1):
    m = model.get_submodule(name)
    conv = getattr(m, "conv", m)
    return dict(name=name, k=conv.kernel_size[0], s=s, g=conv.groups, act=act, cin=conv.in_channels,
                cout=conv.out_channels, bias=int(conv.bias is not None))


# v11_n's positional DWConv (2 heads)
PE = dict(name="net.p5.3.res_m.0.conv1.conv1", k=3, s=1, g=128, act=0, cin=128, cout=128, bias=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_interval_oracle_accepts_fp32_and_rejects_an_ulp(dtype):
    model = make_model("n")
    params = oc.Params(model.state_dict(), dtype)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 20, 20, generator=g).to(dtype)
    d1 = _desc("head.box.0.0", model)
    d2 = _desc("head.box.0.1", model)
    # one layer, and a chain with a residual
    y1 = _fp32_layer(x, d1, params, dtype)
    lo, hi = oc.layer(x.double(), x.double(), d1, params, dtype)
    with oc.exact_values():
        ref, _ = oc.layer(x.double(), x.double(), d1, params, dtype)
    st = oc.compare(y1, lo, hi, ref, dtype, "layer")
    assert st["bad"] == 0 and st["exact"] > 0.99 and st["over1"] < 1e-3, st
    y2 = _fp32_layer(y1, d2, params, dtype, res=y1)
    lo2, hi2 = oc.layer(lo, hi, d2, params, dtype, res=(lo, hi))
    with oc.exact_values():
        ref2, _ = oc.layer(ref, ref, d2, params, dtype, res=(ref, ref))
    st = oc.compare(y2, lo2, hi2, ref2, dtype, "chain")
    assert st["bad"] == 0 and st["over1"] < 5e-3, st
    # a one-ulp change of a pinned element is caught
    idx = torch.nonzero(lo2 == hi2)[len(torch.nonzero(lo2 == hi2)) // 2].tolist()
    bad = y2.clone()
    bits = bad.view(torch.int16)
    bits[tuple(idx)] += 1
    assert oc.compare(bad, lo2, hi2, ref2, dtype, "perturbed")["bad"] == 1


def test_attention_and_dfl_intervals_hold_fp32_evaluations():
    dtype = torch.bfloat16
    model = make_model("n")
    params = oc.Params(model.state_dict(), dtype)
    g = torch.Generator().manual_seed(4)
    heads, H, W = 2, 8, 8
    qkv = torch.randn(1, heads * 128, H, W, generator=g).to(dtype)
    pe = dict(PE)
    lo, hi = oc.attention_op({"in0": qkv.double()}, {"convs": [pe]}, params, dtype, heads)
    # fp32 evaluation with the softmax weights rounded to the dtype before P.V (as the device)
    y = fp32_attention(qkv, pe, params, dtype, heads)
    with oc.exact_values():
        ref, _ = oc.attention_op({"in0": qkv.double()}, {"convs": [pe]}, params, dtype, heads)
    st = oc.compare(y, lo, hi, ref, dtype, "attention")
    assert st["bad"] == 0, st
    # DFL box rows from logits
    lg = torch.randn(1, 64, 4, 4, generator=g).to(dtype)
    blo, bhi = oc.dfl_box(lg.double(), lg.double(), 8, dtype)
    pr = torch.softmax(lg.float().view(1, 4, 16, 16), 2)
    dist = (pr * torch.arange(16.).view(1, 1, 16, 1)).sum(2)
    gy, gx = torch.meshgrid(torch.arange(4.) + 0.5, torch.arange(4.) + 0.5, indexing="ij")
    ax, ay = gx.reshape(1, -1), gy.reshape(1, -1)
    x1, y1, x2, y2 = ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]
    box = torch.stack([(x1 + x2) / 2 * 8, (y1 + y2) / 2 * 8, (x2 - x1) * 8, (y2 - y1) * 8], 1).to(dtype)
    with oc.exact_values():
        bref, _ = oc.dfl_box(lg.double(), lg.double(), 8, dtype)
    st = oc.compare(box, blo, bhi, bref, dtype, "dfl")
    assert st["bad"] == 0, st


def _drop_last_key(k, v):
    return k[..., :-1], v[..., :-1]


def _extra_zero_key(k, v):
    z = lambda t: torch.cat([t, torch.zeros_like(t[..., :1])], -1)
    return z(k), z(v)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (7, 7), (5, 11), (17, 17)])
def test_attention_oracle_rejects_an_off_by_one_key_mask(dtype, H, W):
    """randn qkv, 2 heads, batch 2, T = H * W tokens: the fp32 evaluation lies inside every
    interval; the same evaluation with the last key masked away (a key mask one short), or with
    one all-zero key row past the last token counted (a key mask one long: score 0, value 0, as
    the zero rows the kernels stage), does not.
    Known limit of the oracle: at T = 289 (17 x 17) the extra zero key moves the softmax sum by
    too little to leave the intervals (bf16: 0 of 73984 elements outside; fp16: 8, too few to
    lean on), so only the dropped key is required to be rejected there. The effect of one key
    shrinks like 1 / T while the proven bound does not, which is why the GPU cases lean on small T."""
    model = make_model("n")
    params = oc.Params(model.state_dict(), dtype)
    heads, T = 2, H * W
    qkv = torch.randn(2, heads * 128, H, W, generator=torch.Generator().manual_seed(100 + T)).to(dtype)
    op = {"convs": [dict(PE)]}
    lo, hi = oc.attention_op({"in0": qkv.double()}, op, params, dtype, heads)
    with oc.exact_values():
        ref, _ = oc.attention_op({"in0": qkv.double()}, op, params, dtype, heads)
    bad = lambda keys: oc.compare(fp32_attention(qkv, PE, params, dtype, heads, keys=keys), lo, hi, ref, dtype,
                                  f"T={T}")["bad"]
    n_ok, n_drop, n_extra = bad(None), bad(_drop_last_key), bad(_extra_zero_key)
    print(f"T={T} {dtype}: fp32 bad {n_ok}, last key dropped bad {n_drop}, extra zero key bad {n_extra} of {qkv.shape[0] * heads * 64 * T}")
    assert n_ok == 0
    assert n_drop > 0
    if T != 289:
        assert n_extra > 0
