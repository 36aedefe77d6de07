// Internal interface of csrc/merge_host.cpp (HIP-free): the argument check shared by yh_merge
// and yh_merge_host, and the host merge loop. The C ABI wrappers live in post_abi.cpp; host_util.h
// holds yh_last_error()'s message.
#ifndef YH_MERGE_HOST_H
#define YH_MERGE_HOST_H

#include "yolo_hip.h"

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
