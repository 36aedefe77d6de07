"""Fused C3k2 launches (csrc/c3k2.hip) are bit-identical to the per-layer launches at every
tile shape. Marked gpu.

The kernel takes any run-time TH x TW (pixels are linearised into 32-pixel B tiles), the engine
picks the tile per launch from the map size, the batch and the CU count (Engine::csp_tile) and
YH_CSP_TILE=<TH>x<TW>, read at handle creation like every switch, overrides it. The cases cover what the choice can produce: more tiles
than workgroups (the persistent loop, the counted top-of-tile wait across tiles, a part-empty
last round), tile widths that are no multiple of 16 or 32, tiles that do not divide the map in
either direction, tail mode, the default choice, and a second forward on another input without
graph replay (nothing stale in LDS).
"""
import os
import re

import pytest
import torch

from _util import make_model
from yolo_hip import synth

pytestmark = pytest.mark.gpu


def _engine(model, dtype, dev, fuse, **env):
    """Engine built with YH_FUSE (and any extra YH_* settings) set at handle creation."""
    from yolo_hip.engine import Engine
    env = {"YH_FUSE": "1" if fuse else "0", **env}
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
    return eng


def _csp_ops(eng, batch, h, w):
    return [o for o in eng.ops(batch, h, w) if o["cls"] == "c3k2"]


def _check(gpu, dtype, batch, h, w, seed, tile=None, tail=False):
    model = make_model("n")
    x = synth.synth_scenes(batch, h, w, seed=seed).to(gpu, dtype)
    env = {"YH_CSP_TILE": tile} if tile else {}
    fused = _engine(model, dtype, gpu, True, **({"YH_CSP_TAIL": "1"} if tail else {}), **env)
    plain = _engine(model, dtype, gpu, False)
    yf = fused.forward(x).clone()
    yp = plain.forward(x).clone()
    csp = _csp_ops(fused, batch, h, w)
    assert csp and not _csp_ops(plain, batch, h, w)
    labels = [o["label"] for o in csp]
    if tail:
        assert "net.p3.1.tail" in labels and "fpn.h2.tail" in labels, labels
    assert torch.isfinite(yf.float()).all()
    assert torch.equal(yf, yp), (yf.float() - yp.float()).abs().max().item()
    return fused, plain, csp


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_more_tiles_than_workgroups(gpu, dtype, tail):
    """2 x 8 tiles at batch 2, 320 x 256: net.p2.1 (80 x 64 map) has 640 tiles, 2.5 rounds over
    256 persistent workgroups."""
    _, _, csp = _check(gpu, dtype, 2, 320, 256, seed=41, tile="2x8", tail=tail)
    assert all(o["kernel"] == "c3k2_t2x8" for o in csp), [o["kernel"] for o in csp]


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("tile", ["8x20", "8x12", "4x36"])
def test_odd_tiles_partial_in_both_directions(gpu, tile, tail):
    """96 x 160 at batch 3: the fused maps are 24 x 40 and 12 x 20, so these tiles are clipped
    at the right and the bottom edge; widths 20, 12 and 36 are no multiple of 16 or 32."""
    _, _, csp = _check(gpu, torch.bfloat16, 3, 96, 160, seed=43, tile=tile, tail=tail)
    assert any(o["kernel"] == "c3k2_t" + tile for o in csp), [o["kernel"] for o in csp]


@pytest.mark.parametrize("batch,h,w", [(2, 640, 640), (3, 96, 160)])
def test_default_tile_choice(gpu, batch, h, w):
    _, _, csp = _check(gpu, torch.bfloat16, batch, h, w, seed=47)
    for o in csp:
        m = re.fullmatch(r"c3k2_t(\d+)x(\d+)", o["kernel"])
        assert m, o
        th, tw = int(m.group(1)), int(m.group(2))
        lv = {"net.p2.1": 2, "net.p3.1": 3, "net.p3.1.tail": 3, "fpn.h2.tail": 3}[o["label"]]
        assert 0 < th <= (h >> lv) and 0 < tw <= (w >> lv), o   # a tile the kernel has LDS for, inside the map


def test_second_forward_without_graph_replay(gpu):
    """Another input through the same engines with graph replay off: whatever the first forward
    left in LDS (C2, R1, T1 of the last tile) must not reach the second result."""
    dtype, batch, h, w = torch.bfloat16, 3, 96, 160
    fused, plain, _ = _check(gpu, dtype, batch, h, w, seed=53)
    fused.set_graph(False)
    x2 = synth.synth_scenes(batch, h, w, seed=59).to(gpu, dtype)
    y2 = fused.forward(x2).clone()
    assert torch.equal(y2, plain.forward(x2)), "second forward differs"


def test_switch_binds_at_handle_creation(gpu):
    """A handle keeps the switches its creation saw. Engine A is created with YH_CSP_TILE=8x12 and
    runs after the variable is gone; engine B is created without it and runs its first forward
    with the variable set; C never sees it; P is the per-layer reference (YH_FUSE=0). A must run
    the 8x12 tile, B must run exactly C's kernels, and all three must equal P bit for bit."""
    dtype, batch, h, w = torch.bfloat16, 3, 96, 160
    model = make_model("n")
    x = synth.synth_scenes(batch, h, w, seed=43).to(gpu, dtype)
    assert "YH_CSP_TILE" not in os.environ
    # YH_CONV=0: every dense conv on its first candidate plan, so that the kernel lists do not
    # depend on the autotuner's timings (the plans are bit-identical either way)
    a = _engine(model, dtype, gpu, True, YH_CONV="0", YH_CSP_TILE="8x12")
    b = _engine(model, dtype, gpu, True, YH_CONV="0")
    c = _engine(model, dtype, gpu, True, YH_CONV="0")
    p = _engine(model, dtype, gpu, False, YH_CONV="0")
    ya = a.forward(x).clone()
    os.environ["YH_CSP_TILE"] = "8x12"
    try:
        yb = b.forward(x).clone()
        torch.cuda.synchronize()
    finally:
        del os.environ["YH_CSP_TILE"]
    yc = c.forward(x).clone()
    yp = p.forward(x).clone()
    kernels = lambda e: [o["kernel"] for o in e.ops(batch, h, w)]
    assert any(o["kernel"] == "c3k2_t8x12" for o in _csp_ops(a, batch, h, w)), kernels(a)
    assert kernels(b) == kernels(c)
    assert torch.isfinite(yp.float()).all()
    for y in (ya, yb, yc):
        assert torch.equal(y, yp), (y.float() - yp.float()).abs().max().item()
