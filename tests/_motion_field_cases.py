"""The rules of yh_motion_field (include/yolo_hip.h) restated in numpy - int64 up to the refit, np.float32
operations with one rounding each after it - and the cases the motion-field tests share. TEST
INFRASTRUCTURE ONLY. Luma, thumbnail, the global table's result and the state bytes are those of
tests/_motion_cases.py.
"""
import functools

import numpy as np

import _motion_cases as mc

F = np.float32
I = np.int64
DEFAULTS = dict(max_mad=24, min_contrast=4, tol=1, min_blocks=2)


def f32(v):
    return np.asarray(v, I).astype(F)[()]          # int64 -> fp32 in one rounding


def edges(g, w, R):
    return [R + (p * w) // g for p in range(g + 1)]


def block_tables(C, P, R, gh, gw):
    """-> (gh * gw, 2R+1, 2R+1) int64 SAD tables, [(r0, r1, c0, c1)] per block."""
    th, tw = C.shape
    rows, cols = edges(gh, th - 2 * R, R), edges(gw, tw - 2 * R, R)
    boxes = [(rows[p], rows[p + 1], cols[q], cols[q + 1]) for p in range(gh) for q in range(gw)]
    t = np.zeros((len(boxes), 2 * R + 1, 2 * R + 1), I)
    Ci, Pi = C.astype(I), P.astype(I)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = np.abs(Ci[R:th - R, R:tw - R] - Pi[R - dy:th - R - dy, R - dx:tw - R - dx])
            for k, (r0, r1, c0, c1) in enumerate(boxes):
                t[k, dy + R, dx + R] = d[r0 - R:r1 - R, c0 - R:c1 - R].sum()
    return t, boxes


def pair_fit(a, b):
    dX, dY, dU, dV = (int(a[i]) - int(b[i]) for i in range(4))
    num, den = dX * dU + dY * dV, dX * dX + dY * dY
    return num, den, (a[2] + b[2]) * den - num * (a[0] + b[0]), (a[3] + b[3]) * den - num * (a[1] + b[1])


def inlier(m, k, tol):
    num, den, txn, tyn = m
    return (abs(2 * den * k[2] - txn - 2 * num * k[0]) <= 4 * tol * den
            and abs(2 * den * k[3] - tyn - 2 * num * k[1]) <= 4 * tol * den)


def field_row(C, P, H, W, R, gh, gw, max_mad, min_contrast, tol, min_blocks):
    """One row with a previous frame -> motion (3,) f32, sad (2,) i32, field (gh * gw, 4) i32."""
    th, tw = C.shape
    t, boxes = block_tables(C, P, R, gh, gw)
    motion, sad = mc.result(t.sum(0), R, H, W, th, tw, max_mad)
    field = np.zeros((len(boxes), 4), np.int32)
    pts = []
    for k, (r0, r1, c0, c1) in enumerate(boxes):
        s0, _, dy, dx = mc.best_shift(t[k], R)
        n = (r1 - r0) * (c1 - c0)
        vote = (abs(dy) < R and abs(dx) < R and (max_mad < 0 or s0 <= max_mad * n)
                and int(t[k].max()) - s0 >= min_contrast * n)
        field[k] = (dy, dx, s0, int(vote))
        pts.append((c0 + c1 - tw, r0 + r1 - th, 2 * dx, 2 * dy))
    voters = [k for k in range(len(boxes)) if field[k, 3]]
    cut = max_mad >= 0 and int(sad[0]) > max_mad * (th - 2 * R) * (tw - 2 * R)
    if len(voters) < min_blocks or cut:
        return motion, sad, field
    best = None                                         # most inliers, then the smaller a, then the smaller b
    for i, a in enumerate(voters):
        for b in voters[i + 1:]:
            m = pair_fit(pts[a], pts[b])
            key = (-sum(inlier(m, pts[k], tol) for k in voters), a, b)
            best = key if best is None or key < best else best
    n = -best[0]
    if n < 2 or 2 * n < len(voters):
        return motion, sad, field
    m = pair_fit(pts[best[1]], pts[best[2]])
    inl = [k for k in voters if inlier(m, pts[k], tol)]
    X, Y, U, V = (np.array([pts[k][i] for k in inl], I) for i in range(4))
    Sx, Sy, Su, Sv = (int(v.sum()) for v in (X, Y, U, V))
    Sxx, Sxu = int((X * X + Y * Y).sum()), int((X * U + Y * V).sum())
    z = f32(n * Sxu - Sx * Su - Sy * Sv) / f32(n * Sxx - Sx * Sx - Sy * Sy)
    s = F(1) + z
    if not (s >= F(0.8) and s <= F(1.25)):
        return motion, sad, field
    tu = (f32(Su) - z * f32(Sx)) / f32(2 * n)
    tv = (f32(Sv) - z * f32(Sy)) / f32(2 * n)
    tx = tu * (F(W) / F(tw)) - z * (F(0.5) * F(W))
    ty = tv * (F(H) / F(th)) - z * (F(0.5) * F(H))
    assert all(v.dtype == F for v in (s, tx, ty))
    field[inl, 3] |= 2
    return np.array([s, tx, ty], F), sad, field


class RefField(mc.RefMotion):
    """mc.RefMotion with a second way to advance the same state: field_step is one yh_motion_field call."""

    def field_step(self, frames, radius, grid, stream_ids=None, **kw):
        kw = {**DEFAULTS, **kw}
        B, th, tw, n, NB = len(frames), self.th, self.tw, self.n, grid[0] * grid[1]
        motion = np.tile(np.array([1, 0, 0], F), (B, 1))
        sad = np.zeros((B, 2), np.int32)
        field = np.zeros((B, NB, 4), np.int32)
        for b, f in enumerate(frames):
            s = b if stream_ids is None else int(stream_ids[b])
            if not 0 <= s < self.S:
                continue
            y = mc.luma(f)
            C = mc.thumbnail(y, th, tw)
            blk = self.state[s * (mc.HDR + n):(s + 1) * (mc.HDR + n)]
            if blk[:4].view(np.uint32)[0]:
                P = blk[mc.HDR:].reshape(th, tw)
                motion[b], sad[b], field[b] = field_row(C, P, y.shape[0], y.shape[1], radius, grid[0], grid[1], **kw)
            blk[:mc.HDR] = 0
            blk[0] = 1
            blk[mc.HDR:] = C.reshape(-1)
            st = self.S * (mc.HDR + n) + (b % mc.LAUNCH) * n
            self.state[st:st + n] = C.reshape(-1)
        return motion, sad, field


# ---------------------------------------------------------------- frames
def zoomed(wd, h, w, s, centre, shift):
    """The world seen by a camera whose content moved by x -> s (x - c) + c + shift against the window at
    (wd.shape - (h, w)) / 2: bilinear resampling in fp64 -> (h, w, 3) uint8."""
    oy, ox = (wd.shape[0] - h) / 2, (wd.shape[1] - w) / 2
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    sx = (xx - centre[0] - shift[0]) / s + centre[0] + ox - 0.5       # where this pixel's centre was before
    sy = (yy - centre[1] - shift[1]) / s + centre[1] + oy - 0.5
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    a = wd.astype(np.float64)
    out = ((1 - fy) * ((1 - fx) * a[y0, x0] + fx * a[y0, x0 + 1]) + fy * ((1 - fx) * a[y0 + 1, x0] + fx * a[y0 + 1, x0 + 1]))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def as_kind(img, kind):
    """A BGR array as the frame kind of a case: 'bgr', or 'nv12' (Y = channel 1)."""
    if kind == "bgr":
        return img
    return mc.pre.NV12(np.ascontiguousarray(img[..., 1]), np.ascontiguousarray(img[::2, :, 0]), 601)


# name: (frame h, w, thumb, R, grid, kind). Frames are 3 x 4 source pixels per thumbnail pixel and less
# regular sizes; every case runs first frame, translation, zoom in, zoom out (SEQ).
CASES = {
    "24x32-r2-g2x2": (72, 128, (24, 32), 2, (2, 2), "bgr"),
    "40x52-r3-g3x4": (122, 210, (40, 52), 3, (3, 4), "bgr"),        # block edges off dwords, ragged, R % 4 != 0
    "32x48-r4-g2x3": (96, 192, (32, 48), 4, (2, 3), "nv12"),        # R % 4 == 0
    "40x52-r3-g1x1": (122, 210, (40, 52), 3, (1, 1), "bgr"),        # equals yh_motion
    "12x16-r2-g2x3": (48, 64, (12, 16), 2, (2, 3), "nv12"),         # blocks of exactly 4 x 4
}
SEQ = ((1.0, (0, 0)), (1.0, (5, -3)), (1.06, (2, 1)), (0.95, (-3, 2)))


@functools.lru_cache(maxsize=None)
def case_frames(name):
    """The frames of a case: each the previous one's content zoomed and shifted by SEQ's step."""
    h, w, _, _, _, kind = CASES[name]
    wd = mc.world(40 + len(name) + h, h + 96, w + 96)
    s_tot, t_tot, out = 1.0, np.zeros(2), []
    for s, shift in SEQ:                              # compose about the frame centre
        s_tot, t_tot = s_tot * s, s * t_tot + np.array(shift, float)
        out.append(as_kind(zoomed(wd, h, w, s_tot, (w / 2, h / 2), t_tot), kind))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_steps(n=33):
    """The first case's shapes, n rows over n + 2 streams with shuffled ids and one invalid id per step
    (two launches): rows 0 mod 5 see flat frames (no votes), rows 3 mod 7 unrelated content at step 1 (a
    scene cut), and step 2 advances the state with yh_motion -> [(model, frames, ids)]."""
    h, w, _, _, _, _ = CASES["24x32-r2-g2x2"]
    seq = case_frames("24x32-r2-g2x2")
    other = mc.bgr_frame(mc.world(77, h + 24, w + 24), 12, 12, h, w)
    steps = []
    for t, model in enumerate(("similarity", "similarity", "translation", "similarity")):
        ids = [(2 * b + 3 + t) % (n + 2) for b in range(n)]     # distinct: n + 2 is odd
        ids[(7 * t + 2) % n] = n + 5 if t % 2 else -1
        frames = [mc.flat_frame(h, w, 90 + t) if b % 5 == 0 else other if (t == 1 and b % 7 == 3) else seq[t]
                  for b in range(n)]
        steps.append((model, frames, ids))
    return steps


def run(steps, streams, thumb, R, grid, device="cpu", **kw):
    """yolo_hip.motion.estimate over steps of (model, frames, ids) on a fresh state, outputs poisoned
    -> per step (motion, sad, field, state) as numpy arrays (field is None after a translation step)."""
    import torch
    from yolo_hip import motion as ym
    kw = {**DEFAULTS, **kw}
    state = ym.motion_state(streams, thumb, device)
    res = []
    for model, frames, ids in steps:
        B = len(frames)
        out = (torch.full((B, 3), -7.0, device=device), torch.full((B, 2), -7, dtype=torch.int32, device=device))
        tid = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=device)
        field = None
        if model == "similarity":
            field = torch.full((B, grid[0] * grid[1], 4), -7, dtype=torch.int32, device=device)
            ym.estimate(frames, state, thumb, R, kw["max_mad"], stream_ids=tid, out=out, model=model, grid=grid,
                        min_contrast=kw["min_contrast"], tol=kw["tol"], min_blocks=kw["min_blocks"], field=field, threads=3)
        else:
            ym.estimate(frames, state, thumb, R, kw["max_mad"], stream_ids=tid, out=out, threads=3)
        res.append(tuple(None if t is None else t.cpu().numpy().copy() for t in (out[0], out[1], field, state)))
    return res


def ref(steps, streams, thumb, R, grid, **kw):
    """The same over the restatement."""
    r = RefField(streams, thumb)
    res = []
    for model, frames, ids in steps:
        if model == "similarity":
            m, s, f = r.field_step(frames, R, grid, ids, **kw)
        else:
            m, s = r.step(frames, R, {**DEFAULTS, **kw}["max_mad"], ids)
            f = None
        res.append((m, s, f, r.state.copy()))
    return res


def assert_same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].tobytes() == w[0].tobytes(), f"{what} step {i}: motion {g[0].tolist()} vs {w[0].tolist()}"
        assert np.array_equal(g[1], w[1]), f"{what} step {i}: sad"
        assert (g[2] is None and w[2] is None) or np.array_equal(g[2], w[2]), f"{what} step {i}: field"
        assert np.array_equal(g[3], w[3]), f"{what} step {i}: state"


def corner_error(m, s, centre, shift, h, w):
    """The largest displacement error at the four frame corners of an estimate m = (s, tx, ty)."""
    err = 0.0
    for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
        tx, ty = s * (x - centre[0]) + centre[0] + shift[0], s * (y - centre[1]) + centre[1] + shift[1]
        err = max(err, float(np.hypot(float(m[0]) * x + float(m[1]) - tx, float(m[0]) * y + float(m[2]) - ty)))
    return err
