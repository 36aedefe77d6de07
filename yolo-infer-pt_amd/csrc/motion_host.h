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

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL). On
// success src[k] describes frames[k] (src: batch entries, may be NULL for batch == 0).
const char* yh_motion_check(const yh_frame* frames, int batch, const void* state, int streams, int thumb_h,
                            int thumb_w, int radius, const void* motion, const void* sad, yh_motion_src* src);

// The host twin proper; arguments already checked, src from yh_motion_check. Batch rows run in
// parallel over `threads` (<= 0: every hardware thread).
int yh_motion_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                       int thumb_h, int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, int threads);

#endif
