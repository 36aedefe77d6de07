"""Op-by-op parity of the 16-bit kernels against the fp64 oracle where maps cut their tiles.
Marked gpu.

tests/test_gpu_op_parity.py runs the bench configurations: square, 640 or 1280, a p5 map of 400
or 1600 tokens, i.e. whole blocks of 16 keys and whole tiles almost everywhere. Here the same
driver (tests/_op_parity.py) runs v11_n (and v11_m's four heads) at the smallest maps at which
the kernels take their edge paths. All inputs are synth_scenes, all weights the synthetic ones.

Shapes (input -> p5 map, tokens T) and what they reach:
  *  64 x  64 b2 ->  2 x  2, T =   4: the smallest accepted input; a map of fewer than 16 tokens,
    one partial key block, clamped K-fragment reads, every conv map smaller than a tile;
  *  96 x 160 b3 ->  3 x  5, T =  15: one key short of a block; 315 anchors (no multiple of 8);
  * 160 x 352 b1 ->  5 x 11, T =  55: three whole key blocks + 7 keys; the stem output 40 x 88
    cuts the stem tiles, every level is rectangular;
  * 224 x 224 b2 ->  7 x  7, T =  49: a last query block of one query, a key tail of one key;
  * 544 x 544 b2 -> 17 x 17, T = 289: a second, partial 256-key chunk (33 keys) in
    psa_attention_lds, 19 query blocks over several workgroups (attention and SPPF only);
  * 832 x 832 b1 -> 26 x 26, T = 676: above AF_TMAX, so psa_attention_lds + pe_add by default,
    a 4-key tail in the third chunk (attention and SPPF only);
  * v11_m 224 x 224 b2: 4 heads at T = 49 (attention and SPPF only).
Kernels: whole forwards with the default switches (stem_fused, conv_mx / conv_mxr / conv_rw
plans, csp_fused, c3k_fused, pw_chain, sppf_fused, psa_attention_full<8>, head_cls, box_dfl) at
the first four shapes, bf16 and fp16 alternating; the per-layer launches (YH_FUSE=0 YH_PWCHAIN=0
YH_C3K=0 YH_HCLS_WIDE=0: conv_first, the conv plans, dwconv3x3_c4, the class-rows decode, box
decode) at 96 x 160 and 160 x 352, which closes the transitive pin of the fused kernels at those
maps (fused == per-layer: tests/test_gpu_fusion.py, tests/test_gpu_valu_edges.py); and every
16-bit attention kernel (psa_attention_full<8>, psa_attention_full<16> with YH_ATTN_NW=16
YH_ATTN_QS=1, psa_attention_lds + pe_add with YH_ATTN_FULL=0, psa_attention_mfma + pe_add with
YH_ATTN_FULL=0 YH_ATTN_LDS=0) at T = 4, 15, 49 and 289 in both dtypes. Each case asserts, by the
name yh_op_kernel reports, that the intended attention kernel ran.

tests/test_opcheck_cpu.py (test_attention_oracle_rejects_an_off_by_one_key_mask) shows on the CPU
that at T = 4, 15, 49 and 55 the oracle rejects an attention whose key mask is off by one in
either direction, so a wrong `key0 + r < kend`, a missing zero row past the last token or a
wrong clamp fails these cases. (At T = 289 an extra zero key stays inside the bf16 intervals.)

Bars, per compared output:
  1. every element inside its proven interval (bad == 0);
  2. interval widths (p50, p99) under tests/_op_parity.py's WIDTH_MAX for the kind (EDGE_WIDTH_MAX
     below holds the ceilings of the one case that needs its own: the per-layer stem in fp16);
  3. for attention, conv, dwconv and stem the share beyond one ulp (over1) is held not to
     OVER1_MAX, whose ceilings were measured at 640 / 1280 and do not transfer (on the CPU the
     fp32 evaluation of a T = 4 attention has over1 0.042 against the 0.025 ceiling), but to the
     plain fp32 CPU evaluation of the same op on the same device operands, rounded as the device
     rounds: that evaluation must itself be inside every interval, and the device's share at most
     twice its share + 3 / n;
  4. the fused kinds (stem_fused, c3k2, c3k, pw_chain, head_cls) and sppf / decode / box_dfl:
     bars 1 and 2, over1 printed;
  5. the stepped forward equals the graph forward bit for bit.

Measured on the MI355X (profiles/op_parity_edges_run.txt, the per-op lines of every case; each
case prints the running maxima as "over1 so far"): the largest device / reference over1 ratio
over all cases, per kind, where the reference's share is not zero:
  * attention 1.00 (device 4.5e-2 against 4.5e-2 at T = 4 fp16, 2.4e-2 at T = 4 bf16, down to
    6.6e-3 against 7.0e-3 at T = 289: never above the reference's; all four kernels give the same
    figures, as they are bit-identical);
  * conv 1.00, and at most 2 device elements beyond one ulp in an output where the reference has
    none (inside 3 / n);
  * stem 0.50 (1.1e-5 against 2.2e-5, the per-layer stem at 96 x 160 fp16);
  * dwconv: no element beyond one ulp on either side.
Every element of every output lay inside its interval (bad 0), for the device and the reference.
Interval widths stayed under WIDTH_MAX except the fp16 per-layer stem's (EDGE_WIDTH_MAX below,
from the same run; attention p50 2 - 3, p99 80 - 129 against (6, 240)).
"""
import pytest
import torch

from _op_parity import REF_KINDS, run_op_parity

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
UNFUSED = {"YH_FUSE": 0, "YH_PWCHAIN": 0, "YH_C3K": 0, "YH_HCLS_WIDE": 0}
FUSED_KINDS = {"stem_fused", "c3k2", "c3k", "head_cls", "pw_chain"}

# (p50, p99) interval-width ceilings of the cases that exceed WIDTH_MAX with every element inside
# its interval (the oracle's looseness at that case, not a device error): {case: {kind: (p50, p99)}},
# 1.5 x the measured value where that is above WIDTH_MAX's, else WIDTH_MAX's.
#   * unfused 96 x 160 fp16, stem: p50 0, p99 7 (profiles/op_parity_edges_run.txt, net.p1.0; bad 0,
#     the fp32 reference has the same widths by construction). The per-layer stem had only been
#     measured in bf16 (C2 unfused, C5): an fp16 ulp is an eighth of a bf16 one, so the same fp32
#     K-sum bound spans more of them.
EDGE_WIDTH_MAX = {"unfused-96x160-fp16": {"stem": (1, 10.5)}}

_worst = {}   # kind -> [largest device / reference ratio (reference > 0), most device elements where reference has 0]


def _run(gpu, variant, dtype, batch, h, w, seed, case=None, **kw):
    rep = {}
    kinds, n = run_op_parity(gpu, variant, dtype, batch, None, tuple(range(batch)), seed, height=h, width=w,
                             ref_over1=True, width_max=EDGE_WIDTH_MAX.get(case), report=rep, **kw)
    for kind, rows in rep["over1"].items():
        if kind not in REF_KINDS:
            continue
        wk = _worst.setdefault(kind, [0.0, 0])
        for label, what, cnt, dev, ref in rows:
            if ref > 0:
                wk[0] = max(wk[0], dev / ref)
            else:
                wk[1] = max(wk[1], round(dev * cnt))
    print("over1 so far (kind: largest device / reference ratio, most device elements where the reference has none): "
          + ", ".join(f"{k}: {v[0]:.2f}, {v[1]}" for k, v in sorted(_worst.items())))
    return kinds, rep["kernels"]


def _attn_kernels(kernels):
    return {k for k in kernels.values() if k and k.startswith("psa_attention")}


@pytest.mark.parametrize("dtype,batch,h,w", [(BF16, 2, 64, 64), (FP16, 3, 96, 160), (BF16, 1, 160, 352),
                                             (FP16, 2, 224, 224)], ids=["64x64", "96x160", "160x352", "224x224"])
def test_op_parity_n_small_maps(gpu, dtype, batch, h, w):
    """v11_n, default switches, every active op, all images."""
    kinds, kernels = _run(gpu, "n", dtype, batch, h, w, seed=61)
    assert FUSED_KINDS | {"conv", "sppf", "attention", "box_dfl"} <= kinds, kinds
    assert _attn_kernels(kernels) == {"psa_attention_full<8>"}, kernels


@pytest.mark.parametrize("dtype,batch,h,w", [(FP16, 3, 96, 160), (BF16, 1, 160, 352)], ids=["96x160", "160x352"])
def test_op_parity_n_small_maps_unfused(gpu, dtype, batch, h, w):
    """The per-layer launches each fused kernel is bit-identical to, at the same maps: they meet
    the single-layer bars themselves, which closes the transitive pin of the fused kernels here."""
    case = f"unfused-{h}x{w}-{'fp16' if dtype == FP16 else 'bf16'}"
    kinds, kernels = _run(gpu, "n", dtype, batch, h, w, seed=61, case=case, switches=UNFUSED)
    assert not kinds & FUSED_KINDS, kinds
    assert {"stem", "conv", "dwconv", "sppf", "attention", "decode"} <= kinds, kinds
    assert _attn_kernels(kernels) == {"psa_attention_full<8>"}, kernels


ATTN_SWITCHES = {
    "full": ({}, "psa_attention_full<8>"),
    "lds": ({"YH_ATTN_FULL": 0}, "psa_attention_lds+pe_add"),
    "mfma": ({"YH_ATTN_FULL": 0, "YH_ATTN_LDS": 0}, "psa_attention_mfma+pe_add"),
    "full16": ({"YH_ATTN_NW": 16, "YH_ATTN_QS": 1}, "psa_attention_full<16>"),
}


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("which", list(ATTN_SWITCHES))
@pytest.mark.parametrize("h,w", [(64, 64), (96, 160), (224, 224), (544, 544)], ids=["T4", "T15", "T49", "T289"])
def test_attention_kernels_small_maps(gpu, h, w, which, dtype):
    """Every 16-bit attention kernel (and sppf_fused before it) of v11_n, batch 2, at T = 4, 15,
    49 and 289 against the oracle; the other ops are stepped, not evaluated."""
    switches, kernel = ATTN_SWITCHES[which]
    kinds, kernels = _run(gpu, "n", dtype, 2, h, w, seed=62, kinds={"attention", "sppf"}, switches=switches)
    assert kinds == {"attention", "sppf"}, kinds
    assert _attn_kernels(kernels) == {kernel}, kernels


def test_attention_above_full_kernel_limit(gpu):
    """832 x 832: 676 tokens, above the whole-K/V kernel's limit (AF_TMAX = 640): the chunked
    kernel + pe_add by default, two whole 256-key chunks and one of 164 keys (a 4-key tail)."""
    kinds, kernels = _run(gpu, "n", BF16, 1, 832, 832, seed=63, kinds={"attention", "sppf"})
    assert kinds == {"attention", "sppf"}, kinds
    assert _attn_kernels(kernels) == {"psa_attention_lds+pe_add"}, kernels


@pytest.mark.parametrize("which", ["full", "lds"])
def test_attention_four_heads_small_map(gpu, which):
    """v11_m: 4 heads at 224 x 224 (T = 49), whole-K/V and chunked kernels."""
    switches, kernel = ATTN_SWITCHES[which]
    kinds, kernels = _run(gpu, "m", BF16, 2, 224, 224, seed=64, kinds={"attention", "sppf"}, switches=switches)
    assert kinds == {"attention", "sppf"}, kinds
    assert _attn_kernels(kernels) == {kernel}, kernels
