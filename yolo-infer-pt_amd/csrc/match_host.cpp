// Host (CPU) twin of the batched detection-to-label matching (csrc/match.hip), and the
// argument check both entry points share. HIP-free on purpose: this file compiles alone
// with any C++17 compiler (build it with -ffp-contract=off, as the device file is).
//
// Semantics (yolo_hip/metrics.py compute_metric, utils/util.py:99-120), per image, in one pass
// over all thresholds:
//   1. best[d] = the label of equal class (f32 ==) with the highest IoU, the lower label index
//      on ties; biou[d] = that IoU. No equal-class label: no best label.
//   2. tp[d, t] = 1 iff d has a best label, biou[d] >= iou_v[t], and no e < d has
//      best[e] == best[d] and biou[e] >= iou_v[t].
// IoU in fp32, the operation order of metrics._iou: iw = min(x2) - max(x1) clamped at 0, ih
// likewise, inter = iw * ih, den = ((areaA + areaB) - inter) + 1e-7f, iou = inter / den
// (yh_match_iou in csrc/match_host.h, shared with the kernel).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host_parallel.h"
#include "match_host.h"

namespace {

void match_image(const float* dets, int cnt, int max_det, const float* labels, int lo, int hi, const float* iou_v,
                 int T, uint8_t* tp, float* score_cls) {
    std::vector<int> best(cnt, -1);
    std::vector<float> biou(cnt, -1.0f);
    for (int d = 0; d < cnt; ++d) {
        const float* o = dets + 6 * (size_t)d;
        const float bx1 = o[0], by1 = o[1], bx2 = o[2], by2 = o[3], cls = o[5];
        const float area_b = (bx2 - bx1) * (by2 - by1);
        for (int l = lo; l < hi; ++l) {
            const float* g = labels + 5 * (size_t)l;
            if (!(g[0] == cls)) continue;
            const float area_a = (g[3] - g[1]) * (g[4] - g[2]);
            const float iou = yh_match_iou(g[1], g[2], g[3], g[4], area_a, bx1, by1, bx2, by2, area_b);
            if (iou > biou[d]) { biou[d] = iou; best[d] = l; }
        }
    }
    std::vector<uint32_t> mask(cnt, 0u);
    for (int d = 0; d < cnt; ++d) {
        if (best[d] < 0) continue;
        uint32_t m = 0;
        for (int t = 0; t < T; ++t)
            if (biou[d] >= iou_v[t]) m |= 1u << t;
        mask[d] = m;
    }
    for (int d = 0; d < max_det; ++d) {
        uint32_t bits = 0;
        if (d < cnt && best[d] >= 0) {
            uint32_t taken = 0;
            for (int e = 0; e < d; ++e)
                if (best[e] == best[d]) taken |= mask[e];
            bits = mask[d] & ~taken;
        }
        for (int t = 0; t < T; ++t) tp[(size_t)d * T + t] = (uint8_t)((bits >> t) & 1u);
        if (score_cls) {
            score_cls[2 * (size_t)d] = d < cnt ? dets[6 * (size_t)d + 4] : 0.0f;
            score_cls[2 * (size_t)d + 1] = d < cnt ? dets[6 * (size_t)d + 5] : 0.0f;
        }
    }
}

}  // namespace

const char* yh_match_check(const void* dets, const void* counts, int batch, int max_det, const void* labels,
                           const void* label_offsets, const void* iou_v, int num_iou, const void* tp) {
    if (batch < 0) return "batch must be >= 0";
    if (max_det < 0) return "max_det must be >= 0";
    if (max_det > YH_MATCH_MAX_DET) return "max_det exceeds YH_MATCH_MAX_DET (" YH_STR(YH_MATCH_MAX_DET) ")";
    if (num_iou < 1 || num_iou > 32) return "num_iou must be in [1, 32]";
    if (!iou_v) return "null iou_v";
    if (batch > 0 && (!counts || !label_offsets)) return "null counts / label_offsets";
    if (batch > 0 && max_det > 0 && (!dets || !tp)) return "null dets / tp";
    (void)labels;   // may be NULL when there is no label at all
    return nullptr;
}

int yh_match_host_run(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                      const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                      int* counts_out, int threads) {
    auto run = [&](int b) {
        const int cnt = std::min(std::max(counts[b], 0), max_det);
        match_image(dets + (size_t)b * max_det * 6, cnt, max_det, labels, label_offsets[b], label_offsets[b + 1], iou_v,
                    num_iou, tp + (size_t)b * max_det * num_iou,
                    score_cls ? score_cls + (size_t)b * max_det * 2 : nullptr);
        if (counts_out) counts_out[b] = cnt;
    };
    yh::parallel_strided(batch, threads, run);
    return 0;
}
