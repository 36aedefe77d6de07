"""The host-only parts of yolo_hip.detect: tiles(), tile_transform() and the public names."""
import numpy as np
import pytest

import yolo_hip
from yolo_hip import _lib
from yolo_hip.detect import tile_transform, tiles
from yolo_hip.preprocess import geometry

TILE, OVERLAP = 64, 0.25
STEP = TILE - int(TILE * OVERLAP)
SIZES = sorted({1, 17, TILE - 1, TILE, TILE + 1, 2 * TILE - STEP - 1, 2 * TILE - STEP, 2 * TILE - STEP + 1,
                2 * TILE, 3 * TILE + 5})


def _check_tiling(h, w, tile, overlap, crops):
    step = tile - int(tile * overlap)
    if h <= tile and w <= tile:
        assert crops == [(0, 0, w, h)]
        return
    cover = np.zeros((h, w), bool)
    for x0, y0, cw, ch in crops:
        assert (cw, ch) == (min(tile, w), min(tile, h))
        assert 0 <= x0 and 0 <= y0 and x0 + cw <= w and y0 + ch <= h
        cover[y0:y0 + ch, x0:x0 + cw] = True
    assert cover.all()
    xs = sorted({c[0] for c in crops})
    ys = sorted({c[1] for c in crops})
    assert xs[0] == 0 and ys[0] == 0
    assert all(0 < b - a <= step for a, b in zip(xs, xs[1:])) and all(0 < b - a <= step for a, b in zip(ys, ys[1:]))
    assert all(b - a == step for a, b in zip(xs[:-1], xs[1:-1])) and all(b - a == step for a, b in zip(ys[:-1], ys[1:-1]))
    assert crops == [(x, y, min(tile, w), min(tile, h)) for y in ys for x in xs]          # row-major, a full grid


@pytest.mark.parametrize("h", SIZES)
def test_tiles_cover_the_image(h):
    for w in SIZES:
        crops = tiles(h, w, TILE, OVERLAP)
        _check_tiling(h, w, TILE, OVERLAP, crops)
        assert crops == tiles(h, w, TILE, OVERLAP)                                        # deterministic
        full = tiles(h, w, TILE, OVERLAP, full_image=True)
        if len(crops) > 1:
            assert full == crops + [(0, 0, w, h)]
        else:
            assert full == crops


def test_tiles_of_a_4k_frame():
    crops = tiles(2160, 3840, 640, 0.2)
    _check_tiling(2160, 3840, 640, 0.2, crops)
    assert len(crops) == 8 * 4 and crops[0] == (0, 0, 640, 640) and crops[-1] == (3200, 1520, 640, 640)
    assert tiles(2160, 3840, 640, 0.2, full_image=True)[-1] == (0, 0, 3840, 2160)
    assert tiles(640, 640, 640) == [(0, 0, 640, 640)]
    _check_tiling(416, 544, 320, 0.25, tiles(416, 544, 320, 0.25))
    assert tiles(416, 544, 320, 0.25) == [(0, 0, 320, 320), (224, 0, 320, 320), (0, 96, 320, 320), (224, 96, 320, 320)]


def test_tiles_rejects_bad_arguments():
    for args in ((0, 5, 4), (5, 5, 0), (5, 5, 4, 1.0), (5, 5, 4, -0.1)):
        with pytest.raises(ValueError):
            tiles(*args)


@pytest.mark.parametrize("crop,size", [((0, 0, 640, 480), 320), ((224, 96, 320, 320), 320), ((0, 0, 300, 200), 320),
                                       ((3200, 1520, 640, 640), 640), ((0, 0, 3840, 2160), 640), ((7, 9, 333, 500), 640)])
def test_tile_transform_is_the_inverse_of_the_letterbox_geometry(crop, size):
    x0, y0, w, h = crop
    nh, nw, top, left = geometry(h, w, size)
    f = tile_transform(crop, size)
    assert all(isinstance(v, np.float32) for v in f) and len(f) == 6
    assert f[0] == np.float32(w) / np.float32(nw) and f[1] == np.float32(h) / np.float32(nh)
    assert f[2:] == (left, top, x0, y0)
    if (w, h) == (size, size):
        assert f[0] == 1.0 and f[1] == 1.0 and f[2] == 0 and f[3] == 0
    # the corners of the resized crop on the canvas are the corners of the crop in the source
    assert (left - f[2]) * f[0] + f[4] == x0 and (top - f[3]) * f[1] + f[5] == y0
    assert abs((np.float32(left + nw) - f[2]) * f[0] + f[4] - (x0 + w)) <= 2.0 ** -23 * (x0 + w)


def test_public_names():
    assert yolo_hip.tiles is tiles and yolo_hip.tile_transform is tile_transform
    from yolo_hip import detect
    assert yolo_hip.Detector is detect.Detector and yolo_hip.merge is detect.merge
    assert _lib.ABI_VERSION == 7 and _lib.lib().yh_abi_version() == 7
    assert _lib.MERGE_MAX_CAND >= 4096 and _lib.MERGE_MAX_CAND % 1024 == 0
