// Internal interface of csrc/motion_host.cpp (HIP-free): the argument check both entry points of
// yh_motion share, the host twin, and - because the kernels (csrc/motion.hip) and the twin must
// agree bit for bit - the state layout and the arithmetic of the estimate, written once for both.
// The C ABI wrappers live in post_abi.cpp. The semantics are stated at yh_motion in
// include/yolo_hip.h; tests/_motion_cases.py restates them in numpy.
#ifndef YH_MOTION_HOST_H
#define YH_MOTION_HOST_H

#include <cstddef>
#include <cstdint>

#include "box_math.h"
#include "yolo_hip.h"

// State, in bytes (no pointers; host and device use the same bytes):
//   per stream a YH_MOTION_HDR byte header (word 0: 1 once a thumbnail is stored, words 1 .. 3 zero),
//   then the stream's last thumbnail, thumb_h * thumb_w bytes, row major;
//   behind the `streams` blocks the staging area: YH_MOTION_LAUNCH thumbnails. Batch row b of a call
//   leaves its current thumbnail in staging slot b % YH_MOTION_LAUNCH (a row with an invalid id leaves
//   its slot alone). The device needs the area - the thumbnail kernel has to put the current
//   thumbnail somewhere while the search still reads the previous one from the stream's block - and
//   the host writes the same bytes there, so the whole state compares equal.
enum { YH_MOTION_HDR = 16, YH_MOTION_LAUNCH = 32 };

YH_HD size_t yh_motion_stream_bytes(int thumb_h, int thumb_w) {
    return (size_t)YH_MOTION_HDR + (size_t)thumb_h * (size_t)thumb_w;
}
YH_HD size_t yh_motion_staging_offset(int streams, int thumb_h, int thumb_w) {
    return (size_t)streams * yh_motion_stream_bytes(thumb_h, thumb_w);
}

// One validated frame: what the luma needs of a yh_frame.
struct yh_motion_src {
    const unsigned char* p0;   // BGR: HWC uint8; NV12: the Y plane
    int h, w, stride0, format;
};

// luma of a BGR pixel: OpenCV's fixed-point BGR2GRAY
YH_HD unsigned yh_motion_luma(unsigned b, unsigned g, unsigned r) {
    return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// first source row (column) of thumbnail row (column) i: (i * H) / thumb_h
YH_HD int yh_motion_edge(int i, int src, int thumb) { return (int)(((long long)i * src) / thumb); }

// the mean of a box of n luma bytes, rounded half up
YH_HD unsigned yh_motion_mean(unsigned sum, unsigned n) { return (sum + n / 2u) / n; }

// The candidates' total order as one number, smaller is better: (SAD, |dy| + |dx|, dy, dx).
YH_HD uint64_t yh_motion_key(uint32_t sad, int dy, int dx) {
    const unsigned l1 = (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx));
    return ((uint64_t)sad << 32) | ((uint64_t)l1 << 16) | ((uint64_t)(unsigned)(dy + YH_MOTION_MAX_RADIUS) << 8) |
           (uint64_t)(unsigned)(dx + YH_MOTION_MAX_RADIUS);
}
YH_HD int yh_motion_key_dy(uint64_t k) { return (int)((k >> 8) & 0xff) - YH_MOTION_MAX_RADIUS; }
YH_HD int yh_motion_key_dx(uint64_t k) { return (int)(k & 0xff) - YH_MOTION_MAX_RADIUS; }

// the parabola's vertex through the SADs at -1, 0, +1 around the best shift s0 (sm, sp >= s0)
YH_HD float yh_motion_refine(int32_t s0, int32_t sm, int32_t sp) {
    const int32_t den = (sm - s0) + (sp - s0);
    if (den <= 0) return 0.0f;
    return (0.5f * (float)(sm - sp)) / (float)den;
}

// The outputs of one row from its SAD table ((2 R + 1)^2 entries, entry (dy + R) * (2 R + 1) + dx + R)
// and the best shift: the refinement, the scale to source pixels and the gate.
YH_HD void yh_motion_result(const int32_t* table, int R, int dy, int dx, int H, int W, int thumb_h, int thumb_w,
                            int max_mad, float m[3], int32_t s[2]) {
    const int n = 2 * R + 1;
    const int32_t* c = table + (dy + R) * n + (dx + R);
    const int32_t s0 = c[0];
    s[0] = s0;
    s[1] = table[R * n + R];
    m[0] = 1.0f;
    m[1] = 0.0f;
    m[2] = 0.0f;
    const long long window = (long long)(thumb_h - 2 * R) * (long long)(thumb_w - 2 * R);
    if (max_mad >= 0 && (long long)s0 > (long long)max_mad * window) return;
    const float fx = (dx > -R && dx < R) ? yh_motion_refine(s0, c[-1], c[1]) : 0.0f;
    const float fy = (dy > -R && dy < R) ? yh_motion_refine(s0, c[-n], c[n]) : 0.0f;
    m[1] = ((float)dx + fx) * ((float)W / (float)thumb_w);
    m[2] = ((float)dy + fy) * ((float)H / (float)thumb_h);
}

// ---- yh_motion_field: the block grid, the votes, the pair consensus and the refit, written once
// for the kernels (motion_field_search, motion_field_fit) and the twin. Rule numbers are those at
// yh_motion_field in include/yolo_hip.h.

// Workspace of the device entry, per batch row of a launch (YH_MOTION_LAUNCH rows at most are in
// flight: the launches of a call follow each other on one stream): a record of 4 int32 per block
// (dy, dx, best SAD, max SAD - min SAD), then grid_h partial tables of (2 R + 1)^2 int32, block row
// p's the sum of its blocks' tables.
YH_HD size_t yh_mf_ws_row_bytes(int grid_h, int grid_w, int R) {
    return (size_t)grid_h * grid_w * 16 + (size_t)grid_h * (2 * R + 1) * (2 * R + 1) * 4;
}
// dynamic LDS of a motion_field_search workgroup: the header's formula (the two strips at pitch
// thumb_w + 4 with their slack, the block row's tables, 16 bytes per block of the row)
YH_HD size_t yh_mf_lds_bytes(int thumb_h, int thumb_w, int grid_h, int grid_w, int R) {
    const int bh = (thumb_h - 2 * R + grid_h - 1) / grid_h;
    return (size_t)(2 * bh + 2 * R) * (thumb_w + 4) + (size_t)4 * grid_w * (2 * R + 1) * (2 * R + 1) + 4160;
}

// rule 3: does a block of n pixels with this best shift, best SAD and table spread vote?
YH_HD bool yh_mf_votes(int dy, int dx, int32_t best, int32_t spread, int n, int R, int max_mad, int min_contrast) {
    if (dy <= -R || dy >= R || dx <= -R || dx >= R) return false;
    if (max_mad >= 0 && (long long)best > (long long)max_mad * n) return false;
    return (long long)spread >= (long long)min_contrast * n;
}

// rule 4, doubled units: a block as the fit sees it, and a pair's model
struct yh_mf_pt {
    int32_t X, Y, U, V;
};
struct yh_mf_pair {
    int64_t num, den, txn, tyn;
};
YH_HD yh_mf_pair yh_mf_pair_fit(const yh_mf_pt& a, const yh_mf_pt& b) {
    const int64_t dX = a.X - b.X, dY = a.Y - b.Y, dU = a.U - b.U, dV = a.V - b.V;
    yh_mf_pair m;
    m.num = dX * dU + dY * dV;
    m.den = dX * dX + dY * dY;
    m.txn = (int64_t)(a.U + b.U) * m.den - m.num * (int64_t)(a.X + b.X);
    m.tyn = (int64_t)(a.V + b.V) * m.den - m.num * (int64_t)(a.Y + b.Y);
    return m;
}
// 2 den and 2 num fit 32 bits - |X| < thumb_w, |Y| < thumb_h with thumb_h * thumb_w <= YH_MOTION_MAX_THUMB
// give den < 4 (thumb_w^2 + thumb_h^2) < 2^28, and |U|, |V| <= 2 R give |num| < 2^22 -, so the four
// products below are 32 x 32 -> 64 bit multiplies (one v_mad_i64_i32 each on the device)
YH_HD bool yh_mf_inlier(const yh_mf_pair& m, const yh_mf_pt& k, int tol) {
    const int32_t den2 = (int32_t)(2 * m.den), num2 = (int32_t)(2 * m.num);
    const int64_t lim = 2 * (int64_t)tol * den2;
    const int64_t ru = (int64_t)den2 * k.U - m.txn - (int64_t)num2 * k.X;
    const int64_t rv = (int64_t)den2 * k.V - m.tyn - (int64_t)num2 * k.Y;
    return (ru < 0 ? -ru : ru) <= lim && (rv < 0 ? -rv : rv) <= lim;
}
// the winner's total order as one number, larger is better: (inliers, smaller a, smaller b) with
// a < b block indices below YH_MOTION_FIELD_MAX_BLOCKS
YH_HD uint64_t yh_mf_pair_key(int inliers, int a, int b) {
    return ((uint64_t)(unsigned)inliers << 32) | ((uint64_t)(unsigned)(0xffff - a) << 16) | (uint64_t)(unsigned)(0xffff - b);
}
YH_HD int yh_mf_key_inliers(uint64_t k) { return (int)(k >> 32); }
YH_HD int yh_mf_key_a(uint64_t k) { return 0xffff - (int)((k >> 16) & 0xffff); }
YH_HD int yh_mf_key_b(uint64_t k) { return 0xffff - (int)(k & 0xffff); }

// block (p, q) as the fit sees it, from its record rec (dy, dx, ...), and its pixel count
YH_HD void yh_mf_block_pt(int p, int q, int thumb_h, int thumb_w, int grid_h, int grid_w, int R, const int32_t* rec,
                          yh_mf_pt* pt, int* n) {
    const int wh = thumb_h - 2 * R, ww = thumb_w - 2 * R;
    const int r0 = R + yh_motion_edge(p, wh, grid_h), r1 = R + yh_motion_edge(p + 1, wh, grid_h);
    const int c0 = R + yh_motion_edge(q, ww, grid_w), c1 = R + yh_motion_edge(q + 1, ww, grid_w);
    pt->X = c0 + c1 - thumb_w;
    pt->Y = r0 + r1 - thumb_h;
    pt->U = 2 * rec[1];
    pt->V = 2 * rec[0];
    *n = (r1 - r0) * (c1 - c0);
}
// The refit over the winner's inliers and the last fp32 operations (rules 4 and 5), serial. win: the
// largest yh_mf_pair_key over the voters' pairs (0: there was no pair); flags: bit 0 = the block
// voted; bit 1 is set here for the winner's inliers when the fit stands.
// -> true: m holds the fit's (s, tx, ty); false: the row is yh_motion's.
YH_HD bool yh_mf_refit(const yh_mf_pt* pts, int32_t* flags, int blocks, int voters, uint64_t win, int tol, int H, int W,
                       int thumb_h, int thumb_w, float m[3]) {
    const int n = yh_mf_key_inliers(win);
    if (n < 2 || 2 * n < voters) return false;
    const yh_mf_pair pm = yh_mf_pair_fit(pts[yh_mf_key_a(win)], pts[yh_mf_key_b(win)]);
    int64_t Sx = 0, Sy = 0, Su = 0, Sv = 0, Sxx = 0, Sxu = 0;
    for (int k = 0; k < blocks; ++k) {
        if (!(flags[k] & 1) || !yh_mf_inlier(pm, pts[k], tol)) continue;
        const yh_mf_pt& t = pts[k];
        Sx += t.X; Sy += t.Y; Su += t.U; Sv += t.V;
        Sxx += (int64_t)t.X * t.X + (int64_t)t.Y * t.Y;
        Sxu += (int64_t)t.X * t.U + (int64_t)t.Y * t.V;
    }
    const int64_t zn = n * Sxu - Sx * Su - Sy * Sv, zd = n * Sxx - Sx * Sx - Sy * Sy;   // zd > 0: n >= 2 distinct centres
    const float z = (float)zn / (float)zd;
    const float s = 1.0f + z;
    if (!(s >= 0.8f && s <= 1.25f)) return false;
    const float n2 = (float)(2 * n);
    const float tu = ((float)Su - z * (float)Sx) / n2;
    const float tv = ((float)Sv - z * (float)Sy) / n2;
    m[0] = s;
    m[1] = tu * ((float)W / (float)thumb_w) - z * (0.5f * (float)W);
    m[2] = tv * ((float)H / (float)thumb_h) - z * (0.5f * (float)H);
    for (int k = 0; k < blocks; ++k)
        if ((flags[k] & 1) && yh_mf_inlier(pm, pts[k], tol)) flags[k] |= 2;
    return true;
}

// the complaint about the parameters of yh_motion_field beyond yh_motion_check's, or NULL
const char* yh_motion_field_check(const yh_motion_field_params* p, int thumb_h, int thumb_w);

// The host twin of yh_motion_field; arguments already checked. field may be NULL.
int yh_motion_field_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                             int thumb_h, int thumb_w, const yh_motion_field_params* p, float* motion, int32_t* sad,
                             int32_t* field, int threads);

// The frame rules of yh_letterbox_frames alone: NULL and s filled, or the complaint (yh_propagate's
// check shares them).
const char* yh_motion_describe(const yh_frame& f, yh_motion_src& s);

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL). On
// success src[k] describes frames[k] (src: batch entries, may be NULL for batch == 0).
const char* yh_motion_check(const yh_frame* frames, int batch, const void* state, int streams, int thumb_h,
                            int thumb_w, int radius, const void* motion, const void* sad, yh_motion_src* src);

// The host twin proper; arguments already checked, src from yh_motion_check. Batch rows run in
// parallel over `threads` (<= 0: every hardware thread).
int yh_motion_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                       int thumb_h, int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, int threads);

#endif
