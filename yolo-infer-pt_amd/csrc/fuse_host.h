// Internal interface of csrc/fuse_host.cpp (HIP-free): the argument check shared by yh_fuse and
// yh_fuse_host, the host fusion loop, and the arithmetic of one candidate and one cluster that the
// kernel (csrc/fuse.hip) and the host twin share. The C ABI wrappers live in post_abi.cpp.
// Every function below is one rounding per operation; both sides are built with -ffp-contract=off.
#ifndef YH_FUSE_HOST_H
#define YH_FUSE_HOST_H

#include <cstdint>

#include "box_math.h"
#include "yolo_hip.h"

static_assert(YH_FUSE_MAX_CAND == 4096, "the keys below hold a position or a cluster slot in 12 bits");
constexpr int YH_FUSE_POS_BITS = 12;
constexpr uint32_t YH_FUSE_MAX_CLASS = (1u << 20) - 1;   // class indices are below this: 20 bits of a key
constexpr uint64_t YH_FUSE_NONE = ~(uint64_t)0;          // sorts last

struct yh_fuse_box {
    float x1, y1, x2, y2;
};

// the running sums of a cluster: S = sum s, x1 .. y2 = sum s * coordinate, n members
struct yh_fuse_sums {
    float s, x1, y1, x2, y2, n;
};

// Candidate order: class ascending, then s descending, then position ascending. One ascending sort
// of these keys makes every class a contiguous segment in the order the clustering walks it.
YH_HD uint64_t yh_fuse_cand_key(uint32_t cls, float s, uint32_t pos) {
    return ((uint64_t)cls << 44) | ((uint64_t)yh::float_order<true>(s) << YH_FUSE_POS_BITS) | pos;
}
YH_HD uint32_t yh_fuse_key_class(uint64_t key) { return (uint32_t)(key >> 44); }
YH_HD uint32_t yh_fuse_key_low(uint64_t key) { return (uint32_t)key & ((1u << YH_FUSE_POS_BITS) - 1); }

// Output order: score descending, then class ascending, then slot ascending. The clusters of a
// class take consecutive slots in creation order, so the slot orders them by creation index.
YH_HD uint64_t yh_fuse_out_key(float score, uint32_t cls, uint32_t slot) {
    return ((uint64_t)yh::float_order<true>(score) << 32) | ((uint64_t)cls << YH_FUSE_POS_BITS) | slot;
}
YH_HD uint32_t yh_fuse_out_key_class(uint64_t key) { return ((uint32_t)key >> YH_FUSE_POS_BITS) & YH_FUSE_MAX_CLASS; }

// One row d of group g -> candidate: the map of yh_merge through xf (sx, sy, px, py, ox, oy), the
// swap a mirrored group needs, the clip to the W x H image, the weight. false: dropped (empty after
// the clip, a class that is no index below YH_FUSE_MAX_CLASS, or s < skip).
YH_HD bool yh_fuse_map_row(const float* __restrict__ d, const float* __restrict__ xf, float W, float H, float weight,
                           float skip, yh_fuse_box& b, float& s, uint32_t& cls) {
    using yh::greater;
    using yh::lesser;
    const float sx = xf[0], sy = xf[1], px = xf[2], py = xf[3], ox = xf[4], oy = xf[5];
    float x1 = d[0] - px, y1 = d[1] - py, x2 = d[2] - px, y2 = d[3] - py;
    x1 = x1 * sx; y1 = y1 * sy; x2 = x2 * sx; y2 = y2 * sy;
    x1 = x1 + ox; y1 = y1 + oy; x2 = x2 + ox; y2 = y2 + oy;
    if (x2 < x1) { const float t = x1; x1 = x2; x2 = t; }
    if (y2 < y1) { const float t = y1; y1 = y2; y2 = t; }
    x1 = lesser(greater(x1, 0.0f), W); y1 = lesser(greater(y1, 0.0f), H);
    x2 = lesser(greater(x2, 0.0f), W); y2 = lesser(greater(y2, 0.0f), H);
    b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2;
    if (x2 <= x1 || y2 <= y1) return false;
    const float c = d[5];
    if (!(c >= 0.0f && c < (float)YH_FUSE_MAX_CLASS)) return false;
    cls = (uint32_t)c;
    if ((float)cls != c) return false;
    s = d[4] * weight;
    return !(s < skip);
}

YH_HD float yh_fuse_area(const yh_fuse_box& b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }

// yh_merge's IoU of a fused box f (area fa) and a candidate b (area ba); disjoint boxes are 0
YH_HD float yh_fuse_iou(const yh_fuse_box& f, float fa, const yh_fuse_box& b, float ba) {
    const float inter = yh::intersection(f.x1, f.y1, f.x2, f.y2, b.x1, b.y1, b.x2, b.y2);
    if (inter == 0.0f) return 0.0f;
    return inter / ((fa + ba) - inter);
}

// a cluster's first member
YH_HD yh_fuse_sums yh_fuse_open(float s, const yh_fuse_box& b) {
    return yh_fuse_sums{s, s * b.x1, s * b.y1, s * b.x2, s * b.y2, 1.0f};
}

// one more member: each product is rounded, then added
YH_HD void yh_fuse_add(yh_fuse_sums& c, float s, const yh_fuse_box& b) {
    const float px1 = s * b.x1, py1 = s * b.y1, px2 = s * b.x2, py2 = s * b.y2;
    c.s = c.s + s;
    c.x1 = c.x1 + px1; c.y1 = c.y1 + py1; c.x2 = c.x2 + px2; c.y2 = c.y2 + py2;
    c.n = c.n + 1.0f;
}

// the fused box of a cluster (correctly rounded divisions)
YH_HD yh_fuse_box yh_fuse_box_of(const yh_fuse_sums& c) {
    return yh_fuse_box{c.x1 / c.s, c.y1 / c.s, c.x2 / c.s, c.y2 / c.s};
}

// the confidence of a cluster of an image whose group weights sum to wtot
YH_HD float yh_fuse_score(const yh_fuse_sums& c, float wtot) {
    float t = c.s / c.n;
    t = t * yh::lesser(c.n, wtot);
    return t / wtot;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_fuse_check(const void* dets, const void* counts, int groups, int max_det, const void* group_xf,
                          const void* group_weight, const void* group_offsets, const void* image_wh, int images,
                          int max_groups, int max_out, const void* out, const void* out_counts);
// yh_fuse_host only (the device never reads a weight back): the weight of every group an image owns is > 0
const char* yh_fuse_check_weights(const float* group_weight, const int* group_offsets, int images, int groups,
                                  int max_groups);

// The host twin proper; arguments already checked. Images run in parallel over `threads`
// (<= 0: every hardware thread).
int yh_fuse_host_run(const float* dets, const int* counts, int groups, int max_det, const float* group_xf,
                     const float* group_weight, const int* group_offsets, const float* image_wh, int images,
                     int max_groups, double iou_threshold, float skip_score, int max_out, float* out,
                     int* out_counts, int threads);

#endif
