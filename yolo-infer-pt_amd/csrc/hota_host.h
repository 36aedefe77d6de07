// Internal interface of csrc/hota_host.cpp (HIP-free): the argument check shared by yh_hota_eval
// and yh_hota_eval_host, and everything the kernels (csrc/hota.hip) and the host twin share - the
// similarity, the integer quotients of the rules, the threshold levels and the workspace layout.
// The rules are stated at yh_hota_eval in include/yolo_hip.h.
#ifndef YH_HOTA_HOST_H
#define YH_HOTA_HOST_H

#include <cstddef>
#include <cstdint>

#include "assign_host.h"
#include "box_math.h"
#include "yolo_hip.h"

static_assert(YH_MOT_MAX_IDS == YH_ASSIGN_MAX_SIZE && YH_MOT_MAX_ROWS <= YH_ASSIGN_MAX_SIZE, "a frame is one yh_assign problem");
static_assert((uint64_t)YH_HOTA_MAX_FRAMES * 65536 < (1ull << 32), "P is a uint32");
static_assert(YH_HOTA_MAX_THR <= 32, "a lane's levels are a register array of 32");

constexpr int YH_HOTA_OUT = 8;   // int64 per (sequence, threshold): TP FP FN LOC ASSA ASSRE ASSPR PAIRS
enum { YH_HOTA_TP, YH_HOTA_FP, YH_HOTA_FN, YH_HOTA_LOC, YH_HOTA_ASSA, YH_HOTA_ASSRE, YH_HOTA_ASSPR, YH_HOTA_PAIRS };
constexpr int YH_HOTA_ONE = 65536;        // the similarity of two equal boxes
constexpr int YH_HOTA_ASS_SHIFT = 20;     // the association terms are in units of 2^-20

YH_HD bool yh_hota_id_ok(int id, int n) { return id >= 0 && id < n; }
YH_HD int yh_hota_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// fp32 IoU of a ground-truth row (x1 y1 x2 y2 class) and a hypothesis row (x1 y1 x2 y2 score class):
// yh_mot_eval's rule 1, 0 for boxes that do not intersect
YH_HD float yh_hota_iou(const float* g, const float* t) {
    const float inter = yh::intersection(g[0], g[1], g[2], g[3], t[0], t[1], t[2], t[3]);
    if (inter == 0.0f) return 0.0f;
    const float ag = (g[2] - g[0]) * (g[3] - g[1]);
    const float at = (t[2] - t[0]) * (t[3] - t[1]);
    return inter / ((ag + at) - inter);
}

// rule 1: the similarity of the pair in [0, 65536]; anything but a positive number counts as 0
YH_HD int yh_hota_sim(float iou) {
    const float s = iou * 65536.0f;
    if (!(s > 0.0f)) return 0;
    return s >= 65536.0f ? YH_HOTA_ONE : (int)s;
}
YH_HD int yh_hota_pair_sim(const float* g, const float* t, int class_aware) {
    if (class_aware && !(g[4] == t[5])) return 0;
    return yh_hota_sim(yh_hota_iou(g, t));
}

// (num * 2^16) div den for num <= 2^16 and 0 < den < 2^32. num * 2^16 is 2^32 at most; the one value
// that does not fit 32 bits is taken apart, so that the kernels divide 32-bit numbers.
YH_HD uint32_t yh_hota_div16(uint32_t num, uint32_t den) {
    if (num < 65536u) return (num << 16) / den;
    const uint32_t q = 0xFFFFFFFFu / den;
    return q + (0xFFFFFFFFu - q * den == den - 1u ? 1u : 0u);
}

// rule 2: the frame's Jaccard term of a pair of similarity s > 0 in a row of sum R and a column of sum C
YH_HD uint32_t yh_hota_jaccard(int s, int R, int C) { return yh_hota_div16((uint32_t)s, (uint32_t)(R + C - s)); }

// rule 3: the alignment of the identities g and t from P[g][t] and their frame counts, in [0, 65536]
YH_HD uint32_t yh_hota_align(uint32_t P, uint32_t ng, uint32_t nt) {
    if (P == 0) return 0;
    return (uint32_t)(((uint64_t)P << 16) / (((uint64_t)(ng + nt) << 16) - P));
}

// rule 4: the weight of a pair of similarity s under the alignment A
YH_HD int yh_hota_weight(uint32_t A, int s) {
    if (s <= 0) return 0;
    const uint64_t w = ((uint64_t)A * (uint32_t)s) >> 16;
    return w < 1 ? 1 : (w > 65535 ? 65535 : (int)w);
}

// rule 5: the three association terms of an identity pair matched m > 0 times
YH_HD void yh_hota_terms(uint32_t m, uint32_t ng, uint32_t nt, uint64_t* a, uint64_t* re, uint64_t* pr) {
    const uint64_t q = ((uint64_t)m * m) << YH_HOTA_ASS_SHIFT;
    *a = q / (uint64_t)(ng + nt - m);
    *re = q / ng;
    *pr = q / nt;
}

// Levels. A matched pair reaches `yh_hota_reached` of the thresholds; it is filed under level
// reached - 1. Threshold a is met by the pairs of the levels >= yh_hota_rank(a): its place in
// ascending order (equal values in index order; a NaN is met by nothing). No sorted copy is needed.
YH_HD int yh_hota_reached(float iou, const float* thr, int num_thr) {
    int k = 0;
    for (int a = 0; a < num_thr; ++a) k += iou >= thr[a];
    return k;
}
YH_HD int yh_hota_rank(const float* thr, int num_thr, int a) {
    if (!(thr[a] == thr[a])) return num_thr;
    int k = 0;
    for (int b = 0; b < num_thr; ++b) k += thr[b] < thr[a] || (thr[b] == thr[a] && b < a);
    return k;
}

// The workspace of one sequence, every part padded to 16 bytes: P (G x T uint32), n_g (G uint32),
// n_t (T uint32), H (num_thr x G x T uint32: matched pairs by level), the counters (int64: per level
// TP, LOC, ASSA, ASSRE, ASSPR, PAIRS; then GT rows, HYP rows, ignored GT, ignored HYP) and the ticket
// of the closing launch. Sequence s lies at s * bytes.
constexpr int YH_HOTA_CTR = 6;   // int64 per level
enum { YH_HOTA_C_TP, YH_HOTA_C_LOC, YH_HOTA_C_ASSA, YH_HOTA_C_ASSRE, YH_HOTA_C_ASSPR, YH_HOTA_C_PAIRS };
struct yh_hota_ws {
    size_t P, ng, nt, H, ctr, ticket, bytes;
};
YH_HD size_t yh_hota_up16(size_t v) { return (v + 15) / 16 * 16; }
YH_HD yh_hota_ws yh_hota_layout(int num_thr, int n_gt_ids, int n_tr_ids) {
    const size_t GT = (size_t)n_gt_ids * n_tr_ids;
    yh_hota_ws w{};
    w.P = 0;
    w.ng = w.P + yh_hota_up16(GT * 4);
    w.nt = w.ng + yh_hota_up16((size_t)n_gt_ids * 4);
    w.H = w.nt + yh_hota_up16((size_t)n_tr_ids * 4);
    w.ctr = w.H + yh_hota_up16(GT * num_thr * 4);
    w.ticket = w.ctr + ((size_t)num_thr * YH_HOTA_CTR + 4) * 8;
    w.bytes = yh_hota_up16(w.ticket + 4);
    return w;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_hota_check(const void* tr, const void* tr_ids, const void* tr_counts, int max_out, const void* gt,
                          const void* gt_ids, const void* gt_counts, int max_gt, int sequences, int frame_cap,
                          const void* thr, int num_thr, int n_gt_ids, int n_tr_ids, int class_aware, const void* out,
                          const void* rows, const void* ignored);

// The host twin proper; arguments already checked. Sequences run in parallel over `threads`.
void yh_hota_eval_host_run(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out,
                           const float* gt, const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int sequences,
                           int frame_cap, const int32_t* frames, const float* thr, int num_thr, int n_gt_ids,
                           int n_tr_ids, int class_aware, int64_t* out, int64_t* rows, int32_t* ignored, int threads);

#endif
