"""Tile and map edges of the fused stem (conv.hip stem_fused) and head_cls (head.hip). Marked gpu.

Their index walks (staging chunks, stem pixel groups, depthwise items, pointwise store
addresses) can only go wrong where a tile is cut by the map's edge, so the shapes here are small
maps that cut the 4 x 32 stem tiles and the head_cls tiles in both directions, maps smaller than
one tile, the uint8 staging path and the smallest input the fused engine accepts: 64 x 64 (at
32 x 32 or 32 x 64 the p5 map is below head_cls's smallest 2 x 2 tile and the forward is
refused with "head.cls: no LDS tile"). Every case asserts that the v11_n forward with fusion on equals the per-layer forward
(YH_FUSE=0) bit for bit, replayed from the captured graph and launched eagerly.

The stem's K padding (taps k >= 27 of the 32-deep MFMA step) must contribute exactly zero
whatever the input holds: one case feeds a few inf / nan pixels and compares, with equal_nan,
the fused op's output with the per-layer one where the effect is still local. The last case pins
the fused stem's refusal of an image beyond its 32-bit offsets.
"""
import os

import pytest
import torch

from _util import make_model
from yolo_hip import synth

pytestmark = pytest.mark.gpu


def _engine(model, dtype, dev, fuse):
    """Engine built with YH_FUSE set at handle creation."""
    from yolo_hip.engine import Engine
    old = os.environ.get("YH_FUSE")
    os.environ["YH_FUSE"] = "1" if fuse else "0"
    try:
        eng = Engine(*model._yh_arch, dev, dtype)
    finally:
        if old is None:
            del os.environ["YH_FUSE"]
        else:
            os.environ["YH_FUSE"] = old
    eng.load_module(model)
    return eng


# (engine dtype, uint8 input, batch, height, width)
SHAPES = [
    pytest.param(torch.bfloat16, False, 1, 160, 352, id="bf16-1x160x352"),   # stem output 40 x 88
    pytest.param(torch.float16, False, 2, 64, 96, id="fp16-2x64x96"),        # maps below one tile
    pytest.param(torch.bfloat16, True, 1, 96, 160, id="u8-bf16-1x96x160"),   # uint8 staging
    pytest.param(torch.bfloat16, False, 1, 64, 64, id="bf16-1x64x64"),       # smallest accepted
]


@pytest.fixture(scope="module")
def model():
    return make_model("n")


def _input(dtype, u8, batch, h, w, gpu):
    if u8:
        g = torch.Generator().manual_seed(11)
        return torch.randint(0, 256, (batch, 3, h, w), dtype=torch.uint8, generator=g).to(gpu)
    return synth.synth_scenes(batch, h, w, seed=43).to(gpu, dtype)


def _forwards(model, dtype, gpu, x):
    """(fused graph replay, fused eager, per-layer) forwards of x."""
    b, _, h, w = x.shape
    fused = _engine(model, dtype, gpu, True)
    plain = _engine(model, dtype, gpu, False)
    labels = [o["label"] for o in fused.ops(b, h, w)]
    assert "net.p1.0+p2.0" in labels and "head_cls" in {o["cls"] for o in fused.ops(b, h, w)}
    assert "net.p1.0+p2.0" not in [o["label"] for o in plain.ops(b, h, w)]
    yp = plain.forward(x).clone()
    fused.forward(x)                    # captures
    yg = fused.forward(x).clone()       # replays
    fused.set_graph(False)
    ye = fused.forward(x).clone()
    return yg, ye, yp


@pytest.mark.parametrize("dtype,u8,batch,h,w", SHAPES)
def test_fused_equals_per_layer_at_tile_edges(gpu, model, dtype, u8, batch, h, w):
    x = _input(dtype, u8, batch, h, w, gpu)
    yg, ye, yp = _forwards(model, dtype, gpu, x)
    assert torch.isfinite(yp.float()).all()
    assert torch.equal(yg, yp), (yg.float() - yp.float()).abs().max().item()
    assert torch.equal(ye, yp), (ye.float() - yp.float()).abs().max().item()


def _p2_out(eng, x, pick):
    """Output of the first active op that `pick` accepts, after running the ops up to it only."""
    b, _, h, w = x.shape
    y = eng.forward(x)          # sizes the workspace
    for i in range(len(eng.ops(b, h, w))):
        d = eng.debug_op_desc(i, b, h, w)
        if d["active"] == 1 and pick(d):
            eng.debug_run(x, torch.empty_like(y), 0, i + 1)
            slot = [o["role"] for o in d["operands"]].index("out")
            return eng.debug_operand(i, slot, b, d).float().cpu()
    raise AssertionError("op not found")


def test_stem_k_padding_ignores_non_finite_pixels(gpu, model):
    """The stem's padded K slots read the window corner (channel 0, kh = kw = 0) of each stem
    pixel. If that value reached the MFMA, inf * 0 would turn a stem pixel whose corner is +inf
    from +inf into nan. Further down nothing tells the two apart (p5's attention spreads any
    non-finite value over the whole output), so the comparison is made at net.p2.0's output: the
    fused op's against the per-layer stem + conv. The stem and p2.0 weights are made positive,
    so that a +inf input gives +inf (not nan from inf - inf or silu(-inf)) in all channels of
    both layers: around the +inf pixels the per-layer output must be +inf, and a leak is a nan."""
    import copy
    dtype = torch.bfloat16
    pos = copy.deepcopy(model)
    with torch.no_grad():
        for name in ("net.p1.0", "net.p2.0"):
            pos.get_submodule(name).conv.weight.abs_().clamp_(min=2.0 ** -6)
    x = _input(dtype, False, 1, 160, 352, gpu)
    # +inf in channel 0 at odd (row, col): the corner of stem pixel ((row + 1) / 2, (col + 1) / 2).
    # The first stem pixel, a tile seam (stem column 63: the 65th region column of one tile and
    # the first of the next), the interior, the last stem pixel.
    corners = [(1, 1), (17, 125), (77, 201), (157, 349)]
    for r, c in corners:
        x[0, 0, r, c] = float("inf")
    # and the kinds that end as nan either way, away from the corners' footprints
    x[0, 1, 40, 300] = float("nan")
    x[0, 2, 120, 60] = float("-inf")
    x[0, 0, 100, 20] = float("nan")
    yf = _p2_out(_engine(pos, dtype, gpu, True), x, lambda d: d["kind"] == "stem_fused")
    yp = _p2_out(_engine(pos, dtype, gpu, False), x, lambda d: d["label"] == "net.p2.0")
    assert yf.shape == yp.shape == (1, 40, 88, 32)
    for r, c in corners:
        sh, sw = (r + 1) // 2, (c + 1) // 2
        assert torch.isposinf(yp[0, sh // 2, sw // 2]).all(), (r, c)
    assert torch.isnan(yp).any()
    assert torch.isfinite(yp).float().mean() > 0.99    # 7 pixels reach at most 7 x 4 of 3520 outputs
    assert torch.allclose(yf, yp, rtol=0.0, atol=0.0, equal_nan=True)


def test_fused_stem_refuses_oversized_image(gpu, model):
    """The fused stem addresses an image with 32-bit element offsets: a handle that fuses it
    refuses a larger input by name when the shape is reserved, before allocating anything."""
    eng = _engine(model, torch.bfloat16, gpu, True)
    with pytest.raises(RuntimeError, match="too large for the fused stem"):
        eng.reserve(1, 37856, 37856)      # 3 * 37856^2 = 2^32 + 4.3e6
    x = _input(torch.bfloat16, False, 1, 64, 64, gpu)
    assert torch.isfinite(eng.forward(x).float()).all()
