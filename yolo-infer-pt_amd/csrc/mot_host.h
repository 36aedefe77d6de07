// Internal interface of csrc/mot_host.cpp (HIP-free): the argument check shared by yh_mot_eval and
// yh_mot_eval_host, and the arithmetic the kernel (csrc/mot.hip) and the host twin share - the id
// gate, the allowed-pair test with its weight, the layout of the overlap counts. The rules are
// stated at yh_mot_eval in include/yolo_hip.h.
#ifndef YH_MOT_HOST_H
#define YH_MOT_HOST_H

#include <cstddef>
#include <cstdint>

#include "assign_host.h"
#include "box_math.h"
#include "yolo_hip.h"

static_assert(YH_MOT_MAX_IDS == YH_ASSIGN_MAX_SIZE, "the closing assignment is yh_assign's");
static_assert(YH_MOT_MAX_ROWS <= 256, "a frame's row index is a byte");
static_assert(YH_MOT_MAX_FRAMES <= 65535, "an overlap count is a uint16");

constexpr int YH_MOT_OUT = 8;   // int64 per (sequence, threshold): TP FP FN IDSW SIOU IDTP GT HYP
enum { YH_MOT_TP, YH_MOT_FP, YH_MOT_FN, YH_MOT_IDSW, YH_MOT_SIOU, YH_MOT_IDTP, YH_MOT_GT, YH_MOT_HYP };

// a row takes part iff its id names one of the n identities
YH_HD bool yh_mot_id_ok(int id, int n) { return id >= 0 && id < n; }

YH_HD int yh_mot_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The weight of the pair (ground-truth row g: x1 y1 x2 y2 class, hypothesis row t: x1 y1 x2 y2 score
// class) at threshold a: 0 when the pair is not allowed, else yh_trk_weight(iou) in
// [1, YH_ASSIGN_MAX_WEIGHT]. iou is 0 for boxes that do not intersect.
YH_HD int yh_mot_weight(const float* g, const float* t, int class_aware, float a) {
    if (class_aware && !(g[4] == t[5])) return 0;
    const float inter = yh::intersection(g[0], g[1], g[2], g[3], t[0], t[1], t[2], t[3]);
    float iou = 0.0f;
    if (inter != 0.0f) {
        const float ag = (g[2] - g[0]) * (g[3] - g[1]);
        const float at = (t[2] - t[0]) * (t[3] - t[1]);
        iou = inter / ((ag + at) - inter);
    }
    return iou >= a ? yh_trk_weight(iou) : 0;
}

// The overlap counts C of one (sequence, threshold): n_gt_ids x n_tr_ids uint16, row-major, each
// block padded to 16 bytes; block (s, a) of a launch lies at (s * num_thr + a) * yh_mot_c_bytes.
YH_HD size_t yh_mot_c_bytes(int n_gt_ids, int n_tr_ids) {
    return ((size_t)n_gt_ids * n_tr_ids * 2 + 15) / 16 * 16;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_mot_check(const void* tr, const void* tr_ids, const void* tr_counts, int max_out, const void* gt,
                         const void* gt_ids, const void* gt_counts, int max_gt, int sequences, int frame_cap,
                         const void* thr, int num_thr, int n_gt_ids, int n_tr_ids, int class_aware, const void* out,
                         const void* ignored);

// The host twin proper; arguments already checked. Sequences run in parallel over `threads`.
void yh_mot_eval_host_run(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out,
                          const float* gt, const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int sequences,
                          int frame_cap, const int32_t* frames, const float* thr, int num_thr, int n_gt_ids,
                          int n_tr_ids, int class_aware, int64_t* out, int32_t* ignored, int threads);

#endif
