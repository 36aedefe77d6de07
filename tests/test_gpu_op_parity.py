"""Op-by-op parity of the benchmarked 16-bit kernels against the fp64 oracle. Marked gpu.

The forward of a bench configuration is stepped one op at a time through the parity taps
(include/yolo_hip.h: yh_debug_run_ops, yh_debug_operand). Each op's inputs are taken from the
workspace exactly as the device produced them; tests/_opcheck.py evaluates that one op in
float64 on them (nets/nn.py:28-270, utils/util.py:85-96) and returns, per output element, the
interval of dtype values a correct kernel may produce: the exact result rounded once per layer
output, widened only by the proven bound of the kernel's fp32 arithmetic (K-sum, exp /
reciprocal, the attention's 16-bit softmax weights). Every device output must lie in its
interval; where the exact value is not within that bound of a rounding boundary the interval
is one value and the device must be bit-exact. The printed line per op gives the share of
such pinned elements, the share equal to the correctly rounded exact value (oc.exact_values:
the exact result with every error bound dropped, rounded per layer), the share more than one
ulp from it and the largest distance in ulps (near-zero outputs of opposite sign count the
whole range between them), and the interval width (p50 / p99 / max, in ulps). Single-layer
ops must keep the share beyond one ulp under 0.1 % (measured r05: at most 8e-5); the fused kinds
have per-kind ceilings (OVER1_MAX), and every kind a ceiling on its interval widths (WIDTH_MAX).
The driver (run_op_parity) and both tables live in tests/_op_parity.py, shared with
tests/test_gpu_op_parity_edges.py (the same check on small and rectangular maps).

Covered kernels (by configuration):
  * C2 v11_n bf16 640 b32 (images 0, 17, 31): the tuned conv_mx / conv_mxr / conv_rw plans incl.
    the K-split ones (20x20 / 40x40 layers), stem_fused, csp_fused (whole-block and tail mode),
    c3k_fused in row bands and in SPLIT mode, sppf_fused, psa_attention_full, head_cls (all three
    levels, scores written straight into y), box_dfl;
  * C2 unfused (YH_FUSE=0 YH_PWCHAIN=0 YH_C3K=0 YH_HCLS_WIDE=0): the per-layer launches each
    fused kernel is bit-identical to, at v11_n's shapes, under the single-layer bar;
  * v11_n fp16 640 b2: the same kernels in fp16; v11_n bf16 640 b2: the plans the tuner picks
    at that batch;
  * C3 v11_s fp16 640 b64 (images 0, 63): wider conv plans, seven-launch C3k, per-layer cls
    branches (dwconv3x3_c4) and the class-rows decode (head_decode_lds);
  * C5 v11_x bf16 1280 b1: the 256-cout staged plans, conv_first_tile, the seven-launch C3k,
    psa_attention_lds + pe_add (1600 tokens), dwconv3x3_c4, head_decode_lds, box_dfl (96-channel
    K). Large conv layers are checked on three 4-row bands (top, middle, bottom) and 32 of
    their output channels; every other op on its whole output.
The stepped forward must leave y bit-identical to the graph forward.
"""
import pytest
import torch

from _op_parity import run_op_parity

pytestmark = pytest.mark.gpu


def test_op_parity_c2_n_bf16_b32(gpu):
    kinds, n = run_op_parity(gpu, "n", torch.bfloat16, 32, 640, (0, 17, 31), seed=21)
    assert {"stem_fused", "conv", "c3k2", "c3k", "sppf", "attention", "head_cls", "box_dfl", "pw_chain"} <= kinds, kinds


def test_op_parity_c2_unfused(gpu, monkeypatch):
    """C2 with every cross-layer fusion off (at handle creation): the per-layer launches that
    each fused kernel is bit-identical to (tests/test_gpu_fusion.py) run at v11_n's fused shapes
    and must meet the single-layer bar themselves (<= 0.1 % beyond one ulp, interval p99 width
    <= 4 ulps), which closes the transitive pin of the fused kernels."""
    for k in ("YH_FUSE", "YH_PWCHAIN", "YH_C3K", "YH_HCLS_WIDE"):
        monkeypatch.setenv(k, "0")
    kinds, n = run_op_parity(gpu, "n", torch.bfloat16, 32, 640, (0, 17, 31), seed=21)
    assert not kinds & {"stem_fused", "c3k2", "c3k", "head_cls", "pw_chain"}, kinds
    assert {"stem", "conv", "dwconv", "sppf", "attention", "decode"} <= kinds, kinds


def test_op_parity_n_fp16(gpu):
    kinds, n = run_op_parity(gpu, "n", torch.float16, 2, 640, (0, 1), seed=22)
    assert {"stem_fused", "conv", "c3k2", "c3k", "sppf", "attention", "head_cls", "box_dfl"} <= kinds, kinds


def test_op_parity_c3_s_fp16_b64(gpu):
    kinds, n = run_op_parity(gpu, "s", torch.float16, 64, 640, (0, 63), seed=23)
    assert {"stem_fused", "conv", "c3k2", "dwconv", "decode", "box_dfl", "attention", "sppf"} <= kinds, kinds


def test_op_parity_c5_x_bf16_1280(gpu):
    kinds, n = run_op_parity(gpu, "x", torch.bfloat16, 1, 1280, (0,), seed=24)
    assert {"stem", "conv", "dwconv", "decode", "box_dfl", "attention", "sppf"} <= kinds, kinds
    # (x: 96 box channels, the per-layer box convs + box_dfl)


def test_op_parity_n_bf16_b2(gpu):
    """v11_n bf16 at batch 2, a shape no other parity test runs: the tuner may pick other plans there."""
    kinds, n = run_op_parity(gpu, "n", torch.bfloat16, 2, 640, (0, 1), seed=25)
    assert {"stem_fused", "conv", "c3k2", "c3k", "sppf", "attention", "head_cls", "box_dfl"} <= kinds, kinds
