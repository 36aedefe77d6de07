// Internal interface of csrc/match_host.cpp (HIP-free): the argument check shared by yh_match
// and yh_match_host, the host matching loop, and the IoU that the kernel (csrc/match.hip) and the
// host twin share. The C ABI wrappers live in post_abi.cpp; host_util.h holds yh_last_error()'s
// message.
#ifndef YH_MATCH_HOST_H
#define YH_MATCH_HOST_H

#include <stdint.h>

#include "box_math.h"
#include "yolo_hip.h"

// IoU of a label (a) and a detection (b), corners and areas given, in fp32 and in the operation
// order of yolo_hip.metrics._iou (torch's elementwise ops). Inputs must be finite.
YH_HD float yh_match_iou(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1, float bx2,
                         float by2, float area_b) {
    const float inter = yh::intersection(ax1, ay1, ax2, ay2, bx1, by1, bx2, by2);
    const float den = ((area_a + area_b) - inter) + 1e-7f;
    return inter / den;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_match_check(const void* dets, const void* counts, int batch, int max_det, const void* labels,
                           const void* label_offsets, const void* iou_v, int num_iou, const void* tp);

// The host twin proper; arguments already checked. Images run in parallel over `threads`
// (<= 0: every hardware thread).
int yh_match_host_run(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                      const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                      int* counts_out, int threads);

#endif
