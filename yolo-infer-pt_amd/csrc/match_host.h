// Internal interface of csrc/match_host.cpp (HIP-free): the argument check shared by yh_match
// and yh_match_host, and the host matching loop. The C ABI wrappers live in post_abi.cpp; host_util.h
// holds yh_last_error()'s message.
#ifndef YH_MATCH_HOST_H
#define YH_MATCH_HOST_H

#include <stdint.h>

#include "yolo_hip.h"

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_match_check(const void* dets, const void* counts, int batch, int max_det, const void* labels,
                           const void* label_offsets, const void* iou_v, int num_iou, const void* tp);

// The host twin proper; arguments already checked. Images run in parallel over `threads`
// (<= 0: every hardware thread).
int yh_match_host_run(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                      const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                      int* counts_out, int threads);

#endif
