"""numpy restatement of the video front end's semantics (include/yolo_hip.h: yh_letterbox_geometry2,
yh_nv12_to_bgr_host, yh_letterbox_frames) and the cases test_video_host.py / test_gpu_video.py
share. The resize is the unchanged oracle.preprocess.resize_linear; only the geometry on a
rectangular canvas, the NV12 conversion and the composition are stated here. TEST INFRASTRUCTURE
ONLY.
"""
import numpy as np

from oracle import preprocess as opre

# (CY, CUB, CUG, CVG, CVR) = round(c * 2^20) of the published 3-decimal coefficients
COEF = {601: (1.164, 2.018, -0.391, -0.813, 1.596), 709: (1.164, 2.112, -0.213, -0.533, 1.793)}
FIXED = {601: (1220542, 2116026, -409993, -852492, 1673527), 709: (1220542, 2214593, -223347, -558891, 1880097)}

CANVASES = ((64, 96), (96, 64), (64, 64))
# (height, width): downscale, exact 2x into (64, 96), no resize on (64, 96), upscale, tall, smallest,
# and 50x70, whose 89 resized columns start at left = 3 on (64, 96): a 4-pixel store group straddles
# border and image on both sides
SHAPES = ((36, 64), (128, 192), (64, 96), (18, 32), (90, 40), (2, 2), (50, 70))


def geometry(h, w, ch, cw):
    r = min(ch / h, cw / w)
    nh, nw = (int(h * r), int(w * r)) if r != 1 else (h, w)
    dw, dh = (cw - nw) / 2, (ch - nh) / 2
    return nh, nw, int(round(dh - 0.1)), int(round(dw - 0.1))


def nv12_to_bgr(y, uv, matrix):
    """(h, w) Y and (h / 2, w) interleaved UV uint8 -> (h, w, 3) BGR uint8: integer, shift 20,
    limited range, nearest chroma."""
    cy, cub, cug, cvg, cvr = FIXED[matrix]
    h, w = y.shape
    yy = np.maximum(y.astype(np.int64) - 16, 0) * cy + (1 << 19)
    u = np.repeat(np.repeat(uv[:, 0::2].astype(np.int64), 2, 0), 2, 1)[:h, :w] - 128
    v = np.repeat(np.repeat(uv[:, 1::2].astype(np.int64), 2, 0), 2, 1)[:h, :w] - 128
    b = (yy + cub * u) >> 20
    g = (yy + cvg * v + cug * u) >> 20
    r = (yy + cvr * v) >> 20
    return np.clip(np.stack((b, g, r), -1), 0, 255).astype(np.uint8)


def nv12_to_bgr_float(y, uv, matrix):
    """The same conversion in float64 with the 3-decimal coefficients, rounded half up."""
    cy, cub, cug, cvg, cvr = COEF[matrix]
    h, w = y.shape
    yy = np.maximum(y.astype(np.float64) - 16, 0) * cy
    u = np.repeat(np.repeat(uv[:, 0::2].astype(np.float64), 2, 0), 2, 1)[:h, :w] - 128
    v = np.repeat(np.repeat(uv[:, 1::2].astype(np.float64), 2, 0), 2, 1)[:h, :w] - 128
    out = np.stack((yy + cub * u, yy + cvg * v + cug * u, yy + cvr * v), -1)
    return np.clip(np.floor(out + 0.5), 0, 255)


def letterbox(bgr, ch, cw):
    """(h, w, 3) uint8 BGR -> (3, ch, cw) uint8 RGB on a rectangular canvas."""
    nh, nw, top, left = geometry(bgr.shape[0], bgr.shape[1], ch, cw)
    out = np.zeros((ch, cw, 3), dtype=np.uint8)
    out[top:top + nh, left:left + nw] = opre.resize_linear(bgr, nh, nw)
    return np.ascontiguousarray(out.transpose(2, 0, 1)[::-1])


def bgr_image(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if h > 4 and w > 4:   # a smooth gradient in one channel: rounding at every level
        img[..., 1] = ((np.arange(w)[None, :] * 255) // max(1, w - 1)).astype(np.uint8)
    return img


def nv12_planes(h, w, seed, pad=0):
    """Random Y (h, w) and UV (h / 2, w) planes whose first pixels walk the corner values
    Y in {0, 16, 235, 255} x U, V in {0, 128, 255}; pad > 0: views of wider buffers (strided rows)."""
    rng = np.random.default_rng(seed)
    yb = rng.integers(0, 256, (h, w + pad), dtype=np.uint8)
    ub = rng.integers(0, 256, (h // 2, w + 2 * pad), dtype=np.uint8)
    y, uv = yb[:, :w], ub[:, :w]
    if h > 4 and w > 4:
        y[h // 2:] = ((np.arange(w)[None, :] * 255) // max(1, w - 1)).astype(np.uint8)
    return y, uv


def corner_planes():
    """Every combination of Y in {0, 16, 235, 255} and U, V in {0, 128, 255}: 36 2x2 blocks in a row."""
    ys, cs = (0, 16, 235, 255), (0, 128, 255)
    combos = [(a, b, c) for a in ys for b in cs for c in cs]
    y = np.zeros((2, 2 * len(combos)), np.uint8)
    uv = np.zeros((1, 2 * len(combos)), np.uint8)
    for k, (a, b, c) in enumerate(combos):
        y[:, 2 * k:2 * k + 2] = a
        uv[0, 2 * k], uv[0, 2 * k + 1] = b, c
    return y, uv
