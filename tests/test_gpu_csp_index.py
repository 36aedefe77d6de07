"""Index and address math of the fused C3k2 kernel (csrc/c3k2.hip). Marked gpu.

The kernel keeps its input DMA descriptors in registers for the whole launch (a lane's chunks
of the halo tile, at most 4 rounds of 1024 whole-block and 6 in tail mode), finds a pixel's row
by an exact multiply-shift instead of a division, walks its tiles as (image, tile row, tile
column) with carries, and addresses the map through a wave-uniform base per tile plus a 32-bit
lane offset. Every case compares the fused forward bit for bit with the per-layer engine and
checks that the requested tile was the one that ran; the shapes aim at what that math can get
wrong and stay small (maps of 8 .. 24 rows).

The per-layer reference of a (variant, dtype, shape, seed) is computed once and shared.
"""
import functools
import os

import pytest
import torch

from _util import make_model
from yolo_hip import synth

pytestmark = pytest.mark.gpu


class _env:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _model(variant):
    return make_model(variant)


_PLAIN = {}
_REF = {}


def _plain(variant, dtype, dev):
    """The per-layer engine (YH_FUSE=0) of a variant and dtype, built once."""
    from yolo_hip.engine import Engine
    key = (variant, dtype)
    if key not in _PLAIN:
        with _env(YH_FUSE="0"):
            eng = Engine(*_model(variant)._yh_arch, dev, dtype)
        eng.load_module(_model(variant))
        _PLAIN[key] = eng
    return _PLAIN[key]


def _input(dtype, dev, batch, h, w, seed):
    return synth.synth_scenes(batch, h, w, seed=seed).to(dev, dtype)


def _reference(variant, dtype, dev, batch, h, w, seed):
    key = (variant, dtype, batch, h, w, seed)
    if key not in _REF:
        eng = _plain(variant, dtype, dev)
        y = eng.forward(_input(dtype, dev, batch, h, w, seed)).clone()
        assert not [o for o in eng.ops(batch, h, w) if o["cls"] == "c3k2"]
        _REF[key] = y
    return _REF[key]


def _fused(variant, dtype, dev, tile=None, tail=False):
    from yolo_hip.engine import Engine
    with _env(YH_FUSE="1", YH_CSP_TILE=tile, YH_CSP_TAIL="1" if tail else None):
        eng = Engine(*_model(variant)._yh_arch, dev, dtype)
    eng.load_module(_model(variant))
    return eng


def _check(dev, dtype, batch, h, w, seed, tile=None, tail=False, variant="n"):
    """Fused forward (YH_CSP_TILE read at handle creation) == per-layer forward; returns the fused
    engine and {label: plan string} of its c3k2 ops."""
    ref = _reference(variant, dtype, dev, batch, h, w, seed)
    eng = _fused(variant, dtype, dev, tile, tail)
    y = eng.forward(_input(dtype, dev, batch, h, w, seed)).clone()
    plans = {o["label"]: o["kernel"] for o in eng.ops(batch, h, w) if o["cls"] == "c3k2"}
    assert plans, "no fused c3k2 op"
    if tail:
        assert "net.p3.1.tail" in plans and "fpn.h2.tail" in plans, plans
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, ref), (y.float() - ref.float()).abs().max().item()
    return eng, plans


# ---------------------------------------------------------------- chunk descriptors
# 64 x 512 input: net.p2.1 runs on a 16 x 128 map, the level-3 blocks on 8 x 64.
#   16x20: halo tile 20 x 24 = 480 pixels; whole-block v11_n p2.1 has 5 chunks per pixel (2400,
#          3 rounds, 352 chunks in the last), the tail instances 9 (4320, 5 rounds)
#   4x60:  halo tile 8 x 64 = 512 pixels: 2560 / 4608 chunks (3 / 5 rounds, half-full last round)
# Neither count is a multiple of 1024, and 2400 and 4320 are no multiple of 64: the last round
# ends inside a wave. Both tiles are taller (16x20) or nearly as wide (4x60) as the level-3 map.
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tile", ["16x20", "4x60"])
def test_chunk_descriptor_rounds(gpu, tile, dtype, tail):
    _, plans = _check(gpu, dtype, 2, 64, 512, seed=61, tile=tile, tail=tail)
    assert plans["net.p2.1"] == "c3k2_t" + tile, plans
    if tail:   # both tiles fit the (0, 2, 2) instance of fpn.h2
        assert plans["fpn.h2.tail"] == "c3k2_t" + tile, plans


def test_tile_taller_and_wider_than_the_map_tail(gpu):
    """96 x 160 input: the tail launches run 14 x 22 tiles on 12 x 20 maps (one clipped tile per
    image, every halo row and column past the map comes from the zero page)."""
    _, plans = _check(gpu, torch.bfloat16, 2, 96, 160, seed=62, tile="14x22", tail=True)
    assert plans["net.p3.1.tail"] == "c3k2_t14x22" and plans["fpn.h2.tail"] == "c3k2_t14x22", plans


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_tile_taller_and_wider_than_the_map_whole_block(gpu, dtype):
    """64 x 64 input: net.p2.1 runs one 18 x 20 tile per 16 x 16 map."""
    _, plans = _check(gpu, dtype, 2, 64, 64, seed=63, tile="18x20")
    assert plans["net.p2.1"] == "c3k2_t18x20", plans


# ---------------------------------------------------------------- tile walk across images
# 96 x 128 input: net.p2.1 on 24 x 32 maps in 10 x 32 tiles has three tiles per image, the last
# clipped to 4 rows. With batch 3 every workgroup has one tile (the issue's case); with batch 90
# there are 270 tiles, more than any MI355X has CUs (256), so the workgroups that run a second
# tile step by grid tiles = 85 images + 1 tile row: image, tile row and clipping change at once.
@pytest.mark.parametrize("batch", [3, 90])
def test_tile_walk_crosses_images(gpu, batch):
    dtype, h, w = torch.bfloat16, 96, 128
    eng, plans = _check(gpu, dtype, batch, h, w, seed=64, tile="10x32")
    assert plans["net.p2.1"] == "c3k2_t10x32", plans
    # another input, graph replay off: the same walk launched eagerly
    eng.set_graph(False)
    y2 = eng.forward(_input(dtype, gpu, batch, h, w, 65)).clone()
    assert torch.equal(y2, _reference("n", dtype, gpu, batch, h, w, 65)), "second forward differs"


def test_tile_walk_crosses_images_tail(gpu):
    """The same at level 3 in tail mode: 12 x 16 maps in 5 x 16 tiles, three per image (the last 2
    rows), batch 90."""
    _, plans = _check(gpu, torch.bfloat16, 90, 96, 128, seed=64, tile="5x16", tail=True)
    assert plans["net.p3.1.tail"] == "c3k2_t5x16" and plans["fpn.h2.tail"] == "c3k2_t5x16", plans


# ---------------------------------------------------------------- quotient exactness
# Widths 12, 20, 28, 36, 60 (region widths TW, TW + 2, TW + 4 mostly no powers of two) at the
# tallest tile the LDS admits: the largest pixel indices each instance divides.
@pytest.mark.parametrize("tile", ["32x12", "20x20", "14x28", "10x36", "5x60"])
def test_quotients_largest_tiles_whole_block(gpu, tile):
    _, plans = _check(gpu, torch.bfloat16, 2, 64, 512, seed=66, tile=tile)
    assert plans["net.p2.1"] == "c3k2_t" + tile, plans


@pytest.mark.parametrize("tile", ["25x12", "15x20", "10x28", "8x36", "3x60"])
def test_quotients_largest_tiles_tail(gpu, tile):
    """The tallest tiles of the (0, 2, 4) tail instance; they fit (0, 2, 2) and (2, 1, 2) too."""
    _, plans = _check(gpu, torch.bfloat16, 2, 64, 512, seed=66, tile=tile, tail=True)
    assert set(plans.values()) == {"c3k2_t" + tile}, plans


def test_rejected_tile_falls_back_to_default(gpu):
    """The host check (csp_lds: LDS size, descriptor rounds, exact quotients) refuses 16 x 64 for
    every instance: the default choice runs instead."""
    _, plans = _check(gpu, torch.bfloat16, 2, 64, 512, seed=66, tile="16x64")
    _, default = _check(gpu, torch.bfloat16, 2, 64, 512, seed=66)
    assert "c3k2_t16x64" not in plans.values() and plans == default, (plans, default)


# ---------------------------------------------------------------- the (4, 2, 4) instance
@pytest.mark.parametrize("tile", [None, "7x20"])
def test_v11s_p2_whole_block(gpu, tile):
    """v11_s net.p2.1 is the whole-block (4, 2, 4) instance (16-byte fragment reads at a 144-byte
    pixel stride): batch 2 at 128 x 128, the default tile and the tallest 20-wide one."""
    _, plans = _check(gpu, torch.bfloat16, 2, 128, 128, seed=67, tile=tile, variant="s")
    assert "net.p2.1" in plans, plans
    if tile:
        assert plans["net.p2.1"] == "c3k2_t" + tile, plans
