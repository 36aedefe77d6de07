// Weighted boxes fusion of augmented passes (yh_fuse): the NMS outputs of several passes or models
// over the same image ("groups") are mapped to source pixels, clustered per class by IoU against
// each cluster's running confidence-weighted mean box, and every cluster comes out once with that
// mean box and a confidence that falls when few groups found it - one launch for all images.
// The host twin is csrc/fuse_host.cpp; the semantics are stated in include/yolo_hip.h. The map, the
// keys and the arithmetic of a cluster are shared with the twin through csrc/fuse_host.h.
//
// One workgroup of FUSE_T threads (16 waves) per image, no communication between workgroups, no
// atomics.
//   phase 1  slot s = (group, row) of the image's group range is mapped and weighted in registers
//            and gets a 64-bit key in LDS: class | inverted s | position; invalid and dropped rows
//            get the all-ones sentinel, which sorts last. The member count of every slot is zeroed;
//   phase 2  bitonic sort of the keys over the next power of two (>= 64): every class is now a
//            contiguous segment, already in the order the clustering takes its candidates;
//   phase 3  segment starts: a ballot per wave, the waves' counts through LDS, one list of starts;
//   phase 4  clustering. Segment j belongs to wave j % 16 alone. The wave loads 64 sorted candidates
//            at a time (lane i maps candidate i again: same operations, same bits) and walks them
//            with lane reads. Cluster k of the segment is owned by lane k % 64; its sums live in
//            LDS at slot (segment start + k) - a segment of c candidates has at most c clusters, so
//            the segments' slots never meet - and the owner of a cluster k < 64 also keeps its fused
//            box and area in registers. Per candidate every lane evaluates the IoU against its own
//            clusters (the first from registers, k >= 64 from the LDS sums), a six-step butterfly
//            finds (max IoU, min k) for the wave, and the owning lane alone updates the cluster. A
//            lane only ever reads the sums it wrote itself: no barrier inside a segment;
//   phase 5  after one barrier every slot with members turns its sums into fused box and score in
//            place and writes the output key score | class | slot over its candidate key;
//   phase 6  the same sort, now over the clusters;
//   phase 7  the first max_out clusters are written, every other row is zeroed, the count stored.
// Rows at or beyond a group's count are never read: they are uninitialised memory.
//
// LDS plan (YH_FUSE_MAX_CAND = 4096 candidates):
//   keys   4096 x 8 B                      32768   candidate keys, later the clusters' output keys
//   sums   6 x 4096 x 4 B                  98304   S, Sx1, Sy1, Sx2, Sy2, n of each slot (one array
//                                                  per field: a wave's 64 owners read 64 banks)
//   wsum   4 x 16 x 4 B                      256   per round and wave: segment starts | valid << 16
//   ctl    4 x 4 B                            16   segments, clusters, Wtot
//   seg    (4096 + 8) x 2 B                 8208   segment starts and the end of the last one
//                                          139552 B of the 160 KiB of a CU
// The sort's 8-byte accesses at distance j < 32 are 2-way bank conflicts, as in csrc/merge.hip.
// Built with -ffp-contract=off and without packed fp32 instructions: one rounding per operation.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"
#include "fuse_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int FUSE_T = 1024;                               // threads per workgroup
constexpr int FUSE_WAVES = FUSE_T / 64;
constexpr int FUSE_ROUNDS = YH_FUSE_MAX_CAND / FUSE_T;     // slots per thread
constexpr int FUSE_SEG = YH_FUSE_MAX_CAND + 8;
static_assert(YH_FUSE_MAX_CAND % FUSE_T == 0 && FUSE_ROUNDS >= 1, "slots are dealt out FUSE_T at a time");
static_assert(YH_FUSE_MAX_CAND < 65536, "wsum packs two counts of at most YH_FUSE_MAX_CAND into 16 bits each; seg is 16-bit");
constexpr size_t FUSE_LDS = (size_t)YH_FUSE_MAX_CAND * 8 + 6 * (size_t)YH_FUSE_MAX_CAND * sizeof(float) +
                            FUSE_ROUNDS * FUSE_WAVES * sizeof(int) + 4 * sizeof(int) + FUSE_SEG * sizeof(uint16_t);
// above the 64 KiB a workgroup gets by default: launch_fuse requests the size (up to 160 KiB on gfx950)
static_assert(FUSE_LDS <= 160 * 1024, "LDS plan");

// lane i's value of v, i wave-uniform (v_readlane_b32: no LDS round trip)
__device__ inline float lane_value(float v, int i) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}
__device__ inline int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the sums of slot p; field f of slot p is at sums[f * YH_FUSE_MAX_CAND + p]
__device__ inline yh_fuse_sums load_sums(const float* sums, int p) {
    return yh_fuse_sums{sums[p], sums[YH_FUSE_MAX_CAND + p], sums[2 * YH_FUSE_MAX_CAND + p],
                        sums[3 * YH_FUSE_MAX_CAND + p], sums[4 * YH_FUSE_MAX_CAND + p], sums[5 * YH_FUSE_MAX_CAND + p]};
}
__device__ inline void store_sums(float* sums, int p, const yh_fuse_sums& c) {
    sums[p] = c.s;
    sums[YH_FUSE_MAX_CAND + p] = c.x1;
    sums[2 * YH_FUSE_MAX_CAND + p] = c.y1;
    sums[3 * YH_FUSE_MAX_CAND + p] = c.x2;
    sums[4 * YH_FUSE_MAX_CAND + p] = c.y2;
    sums[5 * YH_FUSE_MAX_CAND + p] = c.n;
}

// ascending bitonic sort of keys[0 .. n2), n2 a power of two; ends on a barrier
__device__ inline void sort_keys(uint64_t* keys, int n2, int tid) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += FUSE_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t a = keys[i], b = keys[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

struct FuseGroups {
    const float* dets;
    const int* counts;
    const float* xf;
    const float* weight;
    int lo, max_det;
    float W, H, skip;
};

// candidate at position pos of the image: false when the row is invalid or dropped
__device__ inline bool map_position(const FuseGroups& g, int pos, yh_fuse_box& b, float& s, uint32_t& cls) {
    const int gl = pos / g.max_det, r = pos - gl * g.max_det, t = g.lo + gl;
    int cnt = g.counts[t];
    cnt = cnt < 0 ? 0 : (cnt > g.max_det ? g.max_det : cnt);
    if (r >= cnt) return false;
    return yh_fuse_map_row(g.dets + ((size_t)t * g.max_det + r) * 6, g.xf + 6 * (size_t)t, g.W, g.H, g.weight[t], g.skip,
                           b, s, cls);
}

__global__ __launch_bounds__(FUSE_T) void fuse_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                      int groups, int max_det, const float* __restrict__ group_xf,
                                                      const float* __restrict__ group_weight,
                                                      const int* __restrict__ group_offsets,
                                                      const float* __restrict__ image_wh, int max_groups, double iou,
                                                      float skip, int max_out, float* __restrict__ out,
                                                      int* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                    // [YH_FUSE_MAX_CAND]
    float* sums = reinterpret_cast<float*>(keys + YH_FUSE_MAX_CAND);       // [6][YH_FUSE_MAX_CAND]
    int* wsum = reinterpret_cast<int*>(sums + 6 * YH_FUSE_MAX_CAND);       // [FUSE_ROUNDS][FUSE_WAVES]
    int* ctl = wsum + FUSE_ROUNDS * FUSE_WAVES;                            // [0] segments [1] clusters [2] Wtot
    uint16_t* seg = reinterpret_cast<uint16_t*>(ctl + 4);                  // [FUSE_SEG]

    const int img = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // the group range, clamped to the group axis and to max_groups (<= YH_FUSE_MAX_CAND / max_det:
    // the slots below never exceed the keys)
    int lo = group_offsets[img], hi = group_offsets[img + 1];
    lo = lo < 0 ? 0 : (lo > groups ? groups : lo);
    hi = hi < lo ? lo : (hi > groups ? groups : hi);
    if (hi - lo > max_groups) hi = lo + max_groups;
    const FuseGroups G{dets, counts, group_xf, group_weight, lo, max_det, image_wh[2 * img], image_wh[2 * img + 1], skip};
    const int used = (hi - lo) * max_det;              // <= max_groups * max_det <= YH_FUSE_MAX_CAND
    int n2 = 64;
    while (n2 < used) n2 <<= 1;

    // phase 1
    for (int s = tid; s < n2; s += FUSE_T) {
        uint64_t key = YH_FUSE_NONE;
        if (s < used) {
            yh_fuse_box b;
            float sc;
            uint32_t cls;
            if (map_position(G, s, b, sc, cls)) key = yh_fuse_cand_key(cls, sc, (uint32_t)s);
        }
        keys[s] = key;
        sums[5 * YH_FUSE_MAX_CAND + s] = 0.0f;
    }
    if (tid == 0) {
        float wtot = 0.0f;
        for (int g = lo; g < hi; ++g) wtot = wtot + group_weight[g];
        ctl[1] = 0;
        ctl[2] = __float_as_int(wtot);
    }
    __syncthreads();
    // phase 2
    sort_keys(keys, n2, tid);
    // phase 3
    unsigned long long starts[FUSE_ROUNDS];
#pragma unroll
    for (int r = 0; r < FUSE_ROUNDS; ++r) {
        const int s = r * FUSE_T + tid;
        const uint64_t k = s < n2 ? keys[s] : YH_FUSE_NONE;
        const bool valid = k != YH_FUSE_NONE;
        const bool start = valid && (s == 0 || yh_fuse_key_class(keys[s - 1]) != yh_fuse_key_class(k));
        starts[r] = __ballot(start);
        const unsigned long long v = __ballot(valid);
        if (lane == 0) wsum[r * FUSE_WAVES + wave] = __popcll(starts[r]) | (__popcll(v) << 16);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < FUSE_ROUNDS; ++r) {
        int before = 0;
        for (int e = 0; e < r * FUSE_WAVES + wave; ++e) before += wsum[e] & 0xffff;   // one address per wave
        if ((starts[r] >> lane) & 1ull)
            seg[before + __popcll(starts[r] & ((1ull << lane) - 1ull))] = (uint16_t)(r * FUSE_T + tid);
    }
    if (tid == 0) {
        int total = 0;
        for (int e = 0; e < FUSE_ROUNDS * FUSE_WAVES; ++e) total += wsum[e];
        seg[total & 0xffff] = (uint16_t)(total >> 16);      // the end of the last segment: the valid candidates
        ctl[0] = total & 0xffff;
    }
    __syncthreads();
    // phase 4
    const int nseg = uniform(ctl[0]);
    for (int j = wave; j < nseg; j += FUSE_WAVES) {
        const int a = uniform(seg[j]), b = uniform(seg[j + 1]);
        int K = 0;                                       // clusters of the segment so far, wave-uniform
        yh_fuse_box cf{0.0f, 0.0f, 0.0f, 0.0f};          // cluster `lane`: fused box and area
        float ca = 0.0f;
        for (int base = a; base < b; base += 64) {
            yh_fuse_box cb{0.0f, 0.0f, 0.0f, 0.0f};
            float cs = 0.0f;
            if (base + lane < b) {
                uint32_t cls;
                map_position(G, (int)yh_fuse_key_low(keys[base + lane]), cb, cs, cls);
            }
            const int m = b - base < 64 ? b - base : 64;
            for (int i = 0; i < m; ++i) {
                const yh_fuse_box x{lane_value(cb.x1, i), lane_value(cb.y1, i), lane_value(cb.x2, i), lane_value(cb.y2, i)};
                const float s = lane_value(cs, i);
                const float xa = yh_fuse_area(x);
                float best = -1.0f;                      // every IoU is >= 0 (or NaN, which never wins)
                int at = INT_MAX;
                if (lane < K) {
                    const float v = yh_fuse_iou(cf, ca, x, xa);
                    if (v > best) {
                        best = v;
                        at = lane;
                    }
                }
                for (int q = lane + 64; q < K; q += 64) {
                    const yh_fuse_box f = yh_fuse_box_of(load_sums(sums, a + q));
                    const float v = yh_fuse_iou(f, yh_fuse_area(f), x, xa);
                    if (v > best) {
                        best = v;
                        at = q;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(best, o);
                    const int oa = __shfl_xor(at, o);
                    if (ov > best || (ov == best && oa < at)) {
                        best = ov;
                        at = oa;
                    }
                }
                at = uniform(at);
                best = __int_as_float(uniform(__float_as_int(best)));
                const bool join = at != INT_MAX && (double)best > iou;
                const int k = join ? at : K;
                if (lane == (k & 63)) {
                    yh_fuse_sums c;
                    if (join) {
                        c = load_sums(sums, a + k);
                        yh_fuse_add(c, s, x);
                    } else {
                        c = yh_fuse_open(s, x);
                    }
                    store_sums(sums, a + k, c);
                    if (k < 64) {
                        cf = yh_fuse_box_of(c);
                        ca = yh_fuse_area(cf);
                    }
                }
                if (!join) ++K;
            }
        }
    }
    __syncthreads();
    // phase 5
    const float wtot = __int_as_float(ctl[2]);
    for (int p = tid; p < n2; p += FUSE_T) {
        const uint64_t k = keys[p];
        uint64_t key = YH_FUSE_NONE;
        if (k != YH_FUSE_NONE && sums[5 * YH_FUSE_MAX_CAND + p] > 0.0f) {
            const yh_fuse_sums c = load_sums(sums, p);
            const yh_fuse_box f = yh_fuse_box_of(c);
            const float score = yh_fuse_score(c, wtot);
            store_sums(sums, p, yh_fuse_sums{score, f.x1, f.y1, f.x2, f.y2, c.n});
            key = yh_fuse_out_key(score, yh_fuse_key_class(k), (uint32_t)p);
        }
        keys[p] = key;
    }
    __syncthreads();
    // phase 6
    sort_keys(keys, n2, tid);
    // phase 7
    float* rows = out + (size_t)img * max_out * 6;
    for (int i = tid; i < max_out; i += FUSE_T) {
        const uint64_t k = i < n2 ? keys[i] : YH_FUSE_NONE;
        float* o = rows + (size_t)i * 6;
        if (k != YH_FUSE_NONE) {
            const yh_fuse_sums c = load_sums(sums, (int)yh_fuse_key_low(k));     // score and fused box since phase 5
            o[0] = c.x1; o[1] = c.y1; o[2] = c.x2; o[3] = c.y2;
            o[4] = c.s;
            o[5] = (float)yh_fuse_out_key_class(k);
        } else {
            o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0f;
        }
    }
    for (int p = tid; p < n2; p += FUSE_T)               // the last cluster in sorted order: one thread at most
        if (keys[p] != YH_FUSE_NONE && (p + 1 == n2 || keys[p + 1] == YH_FUSE_NONE)) ctl[1] = p + 1;
    __syncthreads();
    if (tid == 0) out_counts[img] = ctl[1] < max_out ? ctl[1] : max_out;
}

}  // namespace

int launch_fuse(const float* dets, const int* counts, int groups, int max_det, const float* group_xf,
                const float* group_weight, const int* group_offsets, const float* image_wh, int images, int max_groups,
                double iou_threshold, float skip_score, int max_out, float* out, int* out_counts, hipStream_t s) {
    // arguments were checked by yh_fuse (yh_fuse_check): 1 <= max_groups, max_groups * max_det <= YH_FUSE_MAX_CAND
    if (images <= 0) return 0;
    if (int rc = lds_optin(reinterpret_cast<const void*>(fuse_kernel), (int)FUSE_LDS)) return rc;
    hipLaunchKernelGGL(fuse_kernel, dim3(images), dim3(FUSE_T), FUSE_LDS, s, dets, counts, groups, max_det, group_xf,
                       group_weight, group_offsets, image_wh, max_groups, iou_threshold, skip_score, max_out, out,
                       out_counts);
    return (int)hipGetLastError();
}

}  // namespace yh
