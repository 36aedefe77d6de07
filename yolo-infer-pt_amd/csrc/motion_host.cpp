// Host (CPU) twin of the camera-motion estimate (csrc/motion.hip), and the argument check both
// entry points share. HIP-free on purpose: this file compiles alone with any C++17 compiler (build
// it with -ffp-contract=off, as the device file is). The state layout and the arithmetic are in
// csrc/motion_host.h, shared with the kernels.
//
// Semantics: the rules stated at yh_motion in include/yolo_hip.h. Where the kernels spread the
// source bytes and the candidates over lanes and waves, this file does what the text says: a box
// sum per thumbnail pixel, a SAD per candidate, the smallest key. Every sum is an integer sum, so
// the orders need not agree.
#include "motion_host.h"

#include <cstring>
#include <vector>

#include "host_parallel.h"

namespace {

// The frame rules of yh_letterbox_frames (csrc/preprocess.hip, lb_describe), restated here because
// this file must stay HIP-free: format, matrix, even NV12 sides, planes, strides.
const char* describe(const yh_frame& f, yh_motion_src& s) {
    if (f.format != YH_PIX_BGR && f.format != YH_PIX_NV12) return "motion: unknown pixel format";
    const bool nv12 = f.format == YH_PIX_NV12;
    if (nv12) {
        if (f.matrix != YH_YUV_BT601 && f.matrix != YH_YUV_BT709) return "motion: unknown YUV matrix";
        if (f.height <= 0 || f.width <= 0 || f.height % 2 || f.width % 2)
            return "motion: an NV12 frame needs even, positive height and width";
    }
    if (!f.plane0) return "motion: plane0 is NULL";
    if (nv12 && !f.plane1) return "motion: plane1 of an NV12 frame is NULL";
    if (f.height <= 0 || f.width <= 0) return "motion: frame sides must be positive";
    const long long row0 = nv12 ? (long long)f.width : 3ll * f.width;
    const long long stride0 = f.stride0 ? f.stride0 : row0;
    const long long stride1 = nv12 ? (f.stride1 ? f.stride1 : f.width) : 0;
    if (row0 >= (1ll << 31) || stride0 < row0 || (nv12 && stride1 < f.width)) return "motion: a stride is smaller than the row";
    s.p0 = static_cast<const unsigned char*>(f.plane0);
    s.h = f.height;
    s.w = f.width;
    s.stride0 = (int)stride0;
    s.format = f.format;
    return nullptr;
}

unsigned luma(const yh_motion_src& f, int y, int x) {
    const unsigned char* row = f.p0 + (size_t)y * f.stride0;
    if (f.format == YH_PIX_NV12) return row[x];
    const unsigned char* p = row + (size_t)x * 3;
    return yh_motion_luma(p[0], p[1], p[2]);
}

void thumbnail(const yh_motion_src& f, int th, int tw, unsigned char* out) {
    for (int i = 0; i < th; ++i) {
        const int r0 = yh_motion_edge(i, f.h, th), r1 = yh_motion_edge(i + 1, f.h, th);
        for (int j = 0; j < tw; ++j) {
            const int c0 = yh_motion_edge(j, f.w, tw), c1 = yh_motion_edge(j + 1, f.w, tw);
            unsigned sum = 0;
            for (int y = r0; y < r1; ++y)
                for (int x = c0; x < c1; ++x) sum += luma(f, y, x);
            out[(size_t)i * tw + j] = (unsigned char)yh_motion_mean(sum, (unsigned)(r1 - r0) * (unsigned)(c1 - c0));
        }
    }
}

}  // namespace

const char* yh_motion_check(const yh_frame* frames, int batch, const void* state, int streams, int thumb_h,
                            int thumb_w, int radius, const void* motion, const void* sad, yh_motion_src* src) {
    if (batch < 0) return "motion: batch must be >= 0";
    if (streams < 0) return "motion: streams must be >= 0";
    if (radius < 1 || radius > YH_MOTION_MAX_RADIUS) return "motion: radius must be in [1, " YH_STR(YH_MOTION_MAX_RADIUS) "]";
    if (thumb_h < 1 || thumb_w < 1 || thumb_w % 4) return "motion: thumb_w must be a positive multiple of 4";
    if (thumb_h - 2 * radius < 4 || thumb_w - 2 * radius < 4) return "motion: the search window (thumb - 2 * radius) must be at least 4 x 4";
    if ((long long)thumb_h * thumb_w > YH_MOTION_MAX_THUMB) return "motion: thumb_h * thumb_w exceeds YH_MOTION_MAX_THUMB (" YH_STR(YH_MOTION_MAX_THUMB) ")";
    if (batch > 0 && (!frames || !motion || !sad)) return "motion: null frames / motion / sad";
    if (batch > 0 && !state) return "motion: null state";
    for (int k = 0; k < batch; ++k) {
        yh_motion_src s{};
        if (const char* bad = describe(frames[k], s)) return bad;
        if (s.h < thumb_h || s.w < thumb_w) return "motion: a frame is smaller than the thumbnail";
        // a box sum stays below 2^32
        if ((long long)(s.h / thumb_h + 1) * (long long)(s.w / thumb_w + 1) * 255ll >= (1ll << 32))
            return "motion: a frame is too large for this thumbnail";
        if (src) src[k] = s;
    }
    return nullptr;
}

int yh_motion_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                       int thumb_h, int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, int threads) {
    const int R = radius, n = 2 * R + 1;
    const size_t pixels = (size_t)thumb_h * thumb_w;
    const size_t stride = yh_motion_stream_bytes(thumb_h, thumb_w);
    unsigned char* base = static_cast<unsigned char*>(state);
    unsigned char* staging = base + yh_motion_staging_offset(streams, thumb_h, thumb_w);
    auto row = [&](int b) {
        float* m = motion + (size_t)b * 3;
        int32_t* so = sad + (size_t)b * 2;
        m[0] = 1.0f; m[1] = 0.0f; m[2] = 0.0f;
        so[0] = 0; so[1] = 0;
        const int s = stream_ids ? stream_ids[b] : b;
        if (s < 0 || s >= streams) return;
        std::vector<unsigned char> cur(pixels);
        thumbnail(src[b], thumb_h, thumb_w, cur.data());
        unsigned char* blk = base + (size_t)s * stride;
        uint32_t have;
        std::memcpy(&have, blk, 4);
        unsigned char* prev = blk + YH_MOTION_HDR;
        if (have) {
            std::vector<int32_t> table((size_t)n * n);
            uint64_t best = ~(uint64_t)0;
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    uint32_t acc = 0;
                    for (int i = R; i < thumb_h - R; ++i) {
                        const unsigned char* c = cur.data() + (size_t)i * thumb_w;
                        const unsigned char* p = prev + (size_t)(i - dy) * thumb_w + (R - dx);   // column R - dx >= 0
                        for (int j = R; j < thumb_w - R; ++j) {
                            const int a = c[j], q = p[j - R];
                            acc += (uint32_t)(a > q ? a - q : q - a);
                        }
                    }
                    table[(size_t)(dy + R) * n + (dx + R)] = (int32_t)acc;
                    const uint64_t key = yh_motion_key(acc, dy, dx);
                    if (key < best) best = key;
                }
            yh_motion_result(table.data(), R, yh_motion_key_dy(best), yh_motion_key_dx(best), src[b].h, src[b].w,
                             thumb_h, thumb_w, max_mad, m, so);
        }
        const uint32_t hdr[4] = {1u, 0u, 0u, 0u};
        std::memcpy(blk, hdr, YH_MOTION_HDR);
        std::memcpy(prev, cur.data(), pixels);
        std::memcpy(staging + (size_t)(b % YH_MOTION_LAUNCH) * pixels, cur.data(), pixels);
    };
    // rows that share a staging slot (b and b + YH_MOTION_LAUNCH) must not run at the same time: the
    // last writer wins on the device, launch after launch
    for (int b0 = 0; b0 < batch; b0 += YH_MOTION_LAUNCH) {
        const int nb = batch - b0 < YH_MOTION_LAUNCH ? batch - b0 : YH_MOTION_LAUNCH;
        yh::parallel_strided(nb, threads, [&](int k) { row(b0 + k); });
    }
    return 0;
}
