// Batched matching of NMS detections to ground-truth labels (yh_match): the reference's
// compute_metric (utils/util.py:99-120) for a whole batch in one launch, straight from the
// fixed-size NMS output dets (B, max_det, 6) / counts (B). The host twin is
// csrc/match_host.cpp; the semantics are stated there and in include/yolo_hip.h. The IoU is
// shared with it through csrc/match_host.h.
//
// One workgroup of MATCH_T threads per image, no communication between workgroups.
//   phase 1  every thread owns the detections d = tid, tid + MATCH_T, ...; the image's labels
//            stream through LDS in chunks of MATCH_CHUNK (struct of arrays, so the inner loop's
//            reads are one broadcast address per wave) and each detection keeps its best
//            equal-class label (strict > : the lower label index wins an exact IoU tie);
//   phase 2  mask[d] = the thresholds biou[d] reaches, one bit each (num_iou <= 32);
//   phase 3  bits[d] = mask[d] & ~OR(mask[e] : e < d, best[e] == best[d]);
//   phase 4  coalesced byte stores of all max_det * num_iou tp bytes (0 beyond counts[b]), and of
//            the optional score / class copy.
// Rows at or beyond counts[b] are never read: they are uninitialised memory.
// Built with -ffp-contract=off: the IoU must round exactly as torch's elementwise fp32 ops.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "match_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int MATCH_T = 256;       // threads per workgroup (4 waves)
constexpr int MATCH_CHUNK = 256;   // labels per LDS chunk
// LDS plan: 12 B per detection slot + 6 KiB of labels; the ABI's cap must fit the 64 KiB a
// workgroup may request without an attribute
static_assert((size_t)YH_MATCH_MAX_DET * 12 + 6 * MATCH_CHUNK * sizeof(float) <= 64 * 1024, "LDS plan");

// dynamic LDS only, every carve a multiple of 16 bytes (max_det is rounded up to 4 entries)
__global__ __launch_bounds__(MATCH_T) void match_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        int max_det, const float* __restrict__ labels,
                                                        const int* __restrict__ label_offsets,
                                                        const float* __restrict__ iou_v, int num_iou,
                                                        uint8_t* __restrict__ tp, float* __restrict__ score_cls,
                                                        int* __restrict__ counts_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int md4 = (max_det + 3) & ~3;
    int* best = reinterpret_cast<int*>(smem);                  // [md4] label index, -1 = none
    float* biou = reinterpret_cast<float*>(best + md4);        // [md4] IoU with best
    unsigned* mask = reinterpret_cast<unsigned*>(biou + md4);  // [md4] thresholds reached
    float* lab = reinterpret_cast<float*>(mask + md4);         // [6][MATCH_CHUNK] cls x1 y1 x2 y2 area
    // bits[d] of phase 3 reuses biou's storage (biou is dead after phase 2)
    unsigned* bits = reinterpret_cast<unsigned*>(biou);

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > max_det ? max_det : cnt);
    const int lo = label_offsets[b];
    const int hi = label_offsets[b + 1];
    const float* img = dets + (size_t)b * max_det * 6;

    for (int d = tid; d < cnt; d += MATCH_T) {
        best[d] = -1;
        biou[d] = -1.0f;
    }
    // phase 1 (best / biou entries are private to the thread that owns d: no barrier needed for them)
    for (int base = lo; base < hi; base += MATCH_CHUNK) {
        const int n = min(MATCH_CHUNK, hi - base);
        __syncthreads();   // the previous chunk is no longer read
        for (int i = tid; i < n; i += MATCH_T) {
            const float* g = labels + (size_t)(base + i) * 5;
            const float c = g[0], x1 = g[1], y1 = g[2], x2 = g[3], y2 = g[4];
            lab[i] = c;
            lab[MATCH_CHUNK + i] = x1;
            lab[2 * MATCH_CHUNK + i] = y1;
            lab[3 * MATCH_CHUNK + i] = x2;
            lab[4 * MATCH_CHUNK + i] = y2;
            lab[5 * MATCH_CHUNK + i] = (x2 - x1) * (y2 - y1);
        }
        __syncthreads();
        for (int d = tid; d < cnt; d += MATCH_T) {
            const float* o = img + (size_t)d * 6;
            const float bx1 = o[0], by1 = o[1], bx2 = o[2], by2 = o[3], cls = o[5];
            const float area_b = (bx2 - bx1) * (by2 - by1);
            int bl = best[d];
            float bi = biou[d];
            for (int i = 0; i < n; ++i) {
                if (!(lab[i] == cls)) continue;
                const float iou = yh_match_iou(lab[MATCH_CHUNK + i], lab[2 * MATCH_CHUNK + i], lab[3 * MATCH_CHUNK + i],
                                               lab[4 * MATCH_CHUNK + i], lab[5 * MATCH_CHUNK + i], bx1, by1, bx2, by2,
                                               area_b);
                if (iou > bi) {
                    bi = iou;
                    bl = base + i;
                }
            }
            best[d] = bl;
            biou[d] = bi;
        }
    }
    // phase 2
    for (int d = tid; d < cnt; d += MATCH_T) {
        unsigned m = 0;
        if (best[d] >= 0) {
            const float bi = biou[d];
            for (int t = 0; t < num_iou; ++t)
                if (bi >= iou_v[t]) m |= 1u << t;
        }
        mask[d] = m;
    }
    __syncthreads();
    // phase 3: reads best / mask of lower detections, writes bits (= biou's storage, which no
    // thread reads any more)
    for (int d = tid; d < cnt; d += MATCH_T) {
        const int bl = best[d];
        unsigned taken = 0;
        if (bl >= 0) {
            // four lower detections per step: two 16-byte LDS reads (one address per wave, a
            // broadcast) and no branch, so the reads of successive steps overlap
            const int4* best4 = reinterpret_cast<const int4*>(best);
            const uint4* mask4 = reinterpret_cast<const uint4*>(mask);
            const int quads = d >> 2;
            for (int q = 0; q < quads; ++q) {
                const int4 l = best4[q];
                const uint4 m = mask4[q];
                taken |= (l.x == bl ? m.x : 0u) | (l.y == bl ? m.y : 0u) | (l.z == bl ? m.z : 0u) |
                         (l.w == bl ? m.w : 0u);
            }
            for (int e = quads * 4; e < d; ++e) taken |= best[e] == bl ? mask[e] : 0u;
        }
        bits[d] = mask[d] & ~taken;
    }
    __syncthreads();
    // phase 4
    uint8_t* tpo = tp + (size_t)b * max_det * num_iou;
    const int total = max_det * num_iou;   // <= 4096 * 32
    for (int i = tid; i < total; i += MATCH_T) {
        const int d = i / num_iou, t = i - d * num_iou;
        tpo[i] = d < cnt ? (uint8_t)((bits[d] >> t) & 1u) : (uint8_t)0;
    }
    if (score_cls) {
        float* sc = score_cls + (size_t)b * max_det * 2;
        for (int i = tid; i < 2 * max_det; i += MATCH_T) {
            const int d = i >> 1;
            sc[i] = d < cnt ? img[(size_t)d * 6 + 4 + (i & 1)] : 0.0f;
        }
    }
    if (counts_out && tid == 0) counts_out[b] = cnt;
}

}  // namespace

int launch_match(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                 const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                 int* counts_out, hipStream_t s) {
    // arguments were checked by yh_match (yh_match_check): max_det <= YH_MATCH_MAX_DET, 1 <= num_iou <= 32
    if (batch <= 0) return 0;
    const int md4 = (max_det + 3) & ~3;
    const size_t lds = (size_t)md4 * 12 + (size_t)6 * MATCH_CHUNK * sizeof(float);
    hipLaunchKernelGGL(match_kernel, dim3(batch), dim3(MATCH_T), lds, s, dets, counts, max_det, labels, label_offsets,
                       iou_v, num_iou, tp, score_cls, counts_out);
    return (int)hipGetLastError();
}

}  // namespace yh
