"""The 16-bit epilogues on packed fp32 pairs (dtypes.h silu2, mfma32.h bias_act_pack2 / add_pack2)
compute what the scalar forms computed, bit for bit. Marked gpu.

Two checks:
- yh_debug_silu_pairs runs silu<T> and silu2<T> over every fp32 bit pattern, each pattern once
  next to its neighbour (i ^ 1) and once next to its bit-reversed index, so both halves of a pair
  carry different values; the fp32 results must be equal as bits (NaN payloads included).
- the head output y of seeded inputs equals the output the library gave before its epilogues moved
  to the pair helpers (tests/golden/epilogue_parent_*.npz: this project's own earlier output, as
  uint16 bit patterns), with the default switches and with the fused launches off. The
  fused-vs-per-layer tests cannot pin this: both sides share the helpers.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import make_model
from conftest import load_golden
from yolo_hip import synth

pytestmark = pytest.mark.gpu

# (variant, dtype, batch, height, width): the smallest shapes that reach every epilogue variant.
# n bf16 96x160: partial tiles in both directions, 12x20 / 6x10 / 3x5 maps, 315 anchors (not a
# multiple of 8); s fp16: per-layer C3k, the 128-wide head and the decode path.
CASES = [("n", "bf16", 2, 96, 160), ("n", "fp16", 2, 224, 224), ("s", "fp16", 1, 96, 160)]
INPUT_SEED = 41
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# key in the fixture -> switches at handle creation
SETTINGS = {"y_default": {},
            "y_plain": {"YH_FUSE": "0", "YH_PWCHAIN": "0", "YH_C3K": "0", "YH_HCLS_WIDE": "0"}}


def fixture_name(variant, dt, batch, h, w):
    return f"epilogue_parent_{variant}_{dt}_b{batch}_{h}x{w}.npz"


def head_bits(variant, dt, batch, h, w, env, dev):
    """Head output of the seeded input as uint16 bit patterns, (batch, 84, anchors), on the CPU."""
    from yolo_hip.engine import Engine
    dtype = DTYPES[dt]
    model = make_model(variant)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(*model._yh_arch, dev, dtype)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_module(model)
    x = synth.synth_scenes(batch, h, w, seed=INPUT_SEED).to(dev, dtype)
    y = eng.forward(x).clone()
    assert y.dtype == dtype
    return y.view(torch.int16).cpu()


@pytest.mark.parametrize("key", list(SETTINGS))
@pytest.mark.parametrize("variant,dt,batch,h,w", CASES)
def test_head_output_equals_parent_recording(gpu, variant, dt, batch, h, w, key):
    want = torch.from_numpy(load_golden(fixture_name(variant, dt, batch, h, w))[key].view(np.int16))
    got = head_bits(variant, dt, batch, h, w, SETTINGS[key], gpu)
    assert got.shape == want.shape
    nbad = int((got != want).sum())
    assert torch.equal(got, want), f"{nbad} of {got.numel()} output values differ from the recording"


def _bitrev32(i):
    """Bit reversal of the low 32 bits of an int64 tensor."""
    i = ((i & 0x55555555) << 1) | ((i >> 1) & 0x55555555)
    i = ((i & 0x33333333) << 2) | ((i >> 2) & 0x33333333)
    i = ((i & 0x0F0F0F0F) << 4) | ((i >> 4) & 0x0F0F0F0F)
    i = ((i & 0x00FF00FF) << 8) | ((i >> 8) & 0x00FF00FF)
    return ((i & 0x0000FFFF) << 16) | ((i >> 16) & 0x0000FFFF)


def test_bitrev32():
    i = torch.tensor([0, 1, 2, 0x80000000, 0xFFFFFFFF, 0x12345678], dtype=torch.int64)
    assert _bitrev32(i).tolist() == [0, 0x80000000, 0x40000000, 1, 0xFFFFFFFF, 0x1E6A2C48]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_silu2_equals_silu_on_every_fp32_pattern(gpu, dt):
    from yolo_hip import _lib
    lib = _lib.lib()
    code = {"bf16": _lib.YH_BF16, "fp16": _lib.YH_F16}[dt]
    n = 1 << 25                      # elements per launch: 3 x 128 MB of operands
    x = torch.empty(n, dtype=torch.int32, device=gpu)
    ys = torch.empty_like(x)
    yp = torch.empty_like(x)
    bad = torch.zeros((), dtype=torch.int64, device=gpu)
    first = torch.full((), 1 << 40, dtype=torch.int64, device=gpu)   # smallest differing pattern
    ar = torch.arange(n, dtype=torch.int64, device=gpu)
    half = ar[: n // 2]

    def run(pat):
        """pat: n int64 patterns in 0 .. 2^32-1; positions 2k and 2k+1 form a pair."""
        x.copy_((pat << 32) >> 32)   # the low 32 bits, sign-extended: exact as int32
        rc = lib.yh_debug_silu_pairs(code, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(ys.data_ptr()),
                                     ctypes.c_void_p(yp.data_ptr()), ctypes.c_size_t(n))
        _lib.check(rc, "yh_debug_silu_pairs")
        ne = ys != yp
        bad.add_(ne.sum())
        first.copy_(torch.minimum(first, torch.where(ne, pat, 1 << 40).min()))

    # the entry computes SiLU at all: a few known values through the scalar output
    known = torch.tensor([0.0, 1.0, -1.0, 20.0], dtype=torch.float32)
    run(torch.cat([known.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, torch.zeros(n - 4, dtype=torch.int64)]).to(gpu))
    got = ys[:4].view(torch.float32).cpu()
    assert torch.allclose(got, known * torch.sigmoid(known), rtol=1e-5, atol=0), got.tolist()

    # pass 1: natural order, pattern i next to i ^ 1
    for base in range(0, 1 << 32, n):
        run(ar + base)
    # pass 2: pattern i next to its bit-reversed index (the same value only for palindromes)
    pair = torch.empty(n, dtype=torch.int64, device=gpu)
    for base in range(0, 1 << 32, n // 2):
        i = half + base
        pair[0::2] = i
        pair[1::2] = _bitrev32(i)
        run(pair)
    nbad = int(bad)
    assert nbad == 0, f"silu2<{dt}> differs from silu<{dt}> on {nbad} values, the smallest pattern 0x{int(first):08x}"
