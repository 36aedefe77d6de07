// Internal interface of csrc/merge_host.cpp (HIP-free): the argument check shared by yh_merge
// and yh_merge_host, the host merge loop, and the arithmetic of one row that the kernel
// (csrc/merge.hip) and the host twin share. The C ABI wrappers live in post_abi.cpp; host_util.h
// holds yh_last_error()'s message.
#ifndef YH_MERGE_HOST_H
#define YH_MERGE_HOST_H

#include <cstdint>

#include "box_math.h"
#include "yolo_hip.h"

struct yh_merge_box {
    float x1, y1, x2, y2;
};

// Ascending key = descending score, then ascending position.
YH_HD uint64_t yh_merge_sort_key(float score, uint32_t pos) {
    return ((uint64_t)yh::float_order<true>(score) << 32) | pos;
}

// the map of one row d through its tile's xf (sx, sy, px, py, ox, oy), clipped to the W x H image;
// false: dropped
YH_HD bool yh_merge_map_row(const float* __restrict__ d, const float* __restrict__ xf, float W, float H,
                            yh_merge_box& b) {
    using yh::greater;
    using yh::lesser;
    const float sx = xf[0], sy = xf[1], px = xf[2], py = xf[3], ox = xf[4], oy = xf[5];
    float x1 = d[0] - px, y1 = d[1] - py, x2 = d[2] - px, y2 = d[3] - py;
    x1 = x1 * sx; y1 = y1 * sy; x2 = x2 * sx; y2 = y2 * sy;
    x1 = x1 + ox; y1 = y1 + oy; x2 = x2 + ox; y2 = y2 + oy;
    x1 = lesser(greater(x1, 0.0f), W); y1 = lesser(greater(y1, 0.0f), H);
    x2 = lesser(greater(x2, 0.0f), W); y2 = lesser(greater(y2, 0.0f), H);
    b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2;
    return !(x2 <= x1 || y2 <= y1);
}

// does the kept box (k*, area ka) kill the later box b (area ba)? Disjoint boxes (most pairs) skip
// the division: their quotient is 0 (or NaN), never above a threshold >= 0.
YH_HD bool yh_merge_kills(float kx1, float ky1, float kx2, float ky2, float ka, const yh_merge_box& b, float ba,
                          double iou) {
    const float inter = yh::intersection(kx1, ky1, kx2, ky2, b.x1, b.y1, b.x2, b.y2);
    if (inter == 0.0f && iou >= 0.0) return false;
    const float ovr = inter / ((ka + ba) - inter);
    return (double)ovr > iou;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_merge_check(const void* dets, const void* counts, int tiles, int max_det, const void* tile_xf,
                           const void* tile_offsets, const void* image_wh, int images, int max_tiles, int max_out,
                           const void* out, const void* out_counts);

// The host twin proper; arguments already checked. Images run in parallel over `threads`
// (<= 0: every hardware thread).
int yh_merge_host_run(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
                      const int* tile_offsets, const float* image_wh, int images, int max_tiles,
                      double iou_threshold, int max_out, float* out, int* out_counts, int threads);

#endif
