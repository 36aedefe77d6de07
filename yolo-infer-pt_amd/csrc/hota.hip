// HOTA evaluation (yh_hota_eval): the detection, association and localisation counts of a batch of
// sequences at a list of IoU thresholds. The rules are stated in include/yolo_hip.h, the arithmetic
// is csrc/hota_host.h's (shared with the host twin csrc/hota_host.cpp), the per-frame matching is
// csrc/assign.h's solver (shared with yh_assign, the tracker and yh_mot_eval).
//
// Work split. HOTA has no carry from frame to frame: a frame's matching depends on the alignment of
// the identities, which is a sum over all frames, and on nothing else. So both walks over the frames
// are parallel over (sequence, frame), one wave per frame, and meet in integer atomics on the
// caller's workspace - frame order, wave order and atomic order cannot change a byte.
//
//   hota_zero   clears the workspace (a kernel, not a memset: the entry may be captured in a graph).
//   hota_count  pass A. A wave stages its frame's boxes and ids in LDS (16-byte loads where the
//               address allows, nothing beyond the counts). Lane l owns the ground-truth rows l,
//               l + 64, ...: one sweep over the hypothesis rows gives the row sums R in registers and
//               the column sums C by LDS atomics, a second sweep adds every pair's Jaccard term to
//               P[gt id][track id] with 32-bit atomics in global memory.
//   hota_match  pass B. A wave stages its frame again and turns P, n_g, n_t and the boxes into the
//               frame's weights, once per pair, as a uint16 tile in LDS: a row of the tile per
//               step, a lane's four columns fetched from P together. assign_solve<false> then reads
//               the tile only. Each matched pair is filed under the highest threshold level it
//               reaches with one atomic on H[level][gt id][track id]; TP and the similarity sum go
//               to per-level counters, one atomic per wave and level. The host packs as many waves
//               into a workgroup as their LDS allows: one at 256 x 256 rows, thirteen at 64 x 64.
//   hota_close  over (sequence, 256 identity pairs): a lane sums one pair's levels from the top
//               down in registers, which turns H into the match counts of every threshold, takes the
//               three 64-bit quotients where the count changes, and the waves add their sums to the
//               level counters. The last workgroup of a sequence (a ticket) writes the outputs.
//
// No wave waits for another one; every loop is bounded by a count the whole wave shares.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign.h"
#include "common.h"
#include "hota_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int HOTA_K = YH_MOT_MAX_ROWS / 64;   // rows per lane at the cap
constexpr int HOTA_COUNT_WAVES = 4;            // frames per workgroup of pass A
constexpr int HOTA_MATCH_WAVES = 16;           // at most, in pass B
constexpr int HOTA_LDS = 160 * 1024;
constexpr int HOTA_CLOSE_THREADS = 256;
static_assert(YH_MOT_MAX_ROWS % 64 == 0, "rows per lane");

__host__ __device__ constexpr int up(int v, int m) { return (v + m - 1) / m * m; }

// a wave's words in LDS: the staged frame, then pass A's column sums or pass B's solver words and tile
struct HotaLds {
    int rg, rt;                  // rows per side, rounded up to quads
    int staged, count, match;    // bytes: the staged frame, a wave of pass A, a wave of pass B
    int match_waves;
};
__host__ __device__ constexpr HotaLds hota_lds(int max_gt, int max_out) {
    HotaLds m{};
    m.rg = up(max_gt, 4);
    m.rt = up(max_out, 4);
    m.staged = (m.rg * 5 + m.rt * 6 + m.rg + m.rt) * 4;
    m.count = m.staged + m.rt * 4;
    m.match = m.staged + (int)assign_lds_words(m.rg, m.rt) * 4 + up(max_gt * m.rt * 2, 16);
    const int fit = m.match ? HOTA_LDS / m.match : HOTA_MATCH_WAVES;   // no rows on either side: no bytes
    m.match_waves = fit < 1 ? 1 : (fit > HOTA_MATCH_WAVES ? HOTA_MATCH_WAVES : fit);
    return m;
}
static_assert(hota_lds(YH_MOT_MAX_ROWS, YH_MOT_MAX_ROWS).match == YH_HOTA_LDS_AT_CAPS && YH_HOTA_LDS_AT_CAPS <= HOTA_LDS,
              "the budget stated in the header");
static_assert(hota_lds(YH_MOT_MAX_ROWS, YH_MOT_MAX_ROWS).count * HOTA_COUNT_WAVES <= 64 * 1024, "pass A needs no opt-in");
static_assert(hota_lds(64, 64).match_waves == 13, "as documented");

struct Staged {
    float* gb;   // [rg][5]
    float* tb;   // [rt][6]
    int* gi;     // [rg]
    int* ti;     // [rt]
};
__device__ inline Staged staged_at(char* base, const HotaLds& m) {
    Staged h;
    h.gb = reinterpret_cast<float*>(base);
    h.tb = h.gb + m.rg * 5;
    h.gi = reinterpret_cast<int*>(h.tb + m.rt * 6);
    h.ti = h.gi + m.rg;
    return h;
}

// n words from global memory to LDS by one wave; dst is 16-byte aligned
__device__ inline void wave_copy(int* dst, const int* src, int n, int lane) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {   // one address for the wave: uniform
        const int n4 = n >> 2;
        for (int i = lane; i < n4; i += 64) reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(src)[i];
        done = n4 * 4;
    }
    for (int i = done + lane; i < n; i += 64) dst[i] = src[i];
}

__device__ inline void stage(const HotaEval& p, const Staged& h, size_t sf, int ng, int nh, int lane) {
    wave_copy(reinterpret_cast<int*>(h.gb), reinterpret_cast<const int*>(p.gt + sf * p.max_gt * 5), ng * 5, lane);
    wave_copy(reinterpret_cast<int*>(h.tb), reinterpret_cast<const int*>(p.tr + sf * p.max_out * 6), nh * 6, lane);
    wave_copy(h.gi, p.gt_ids + sf * p.max_gt, ng, lane);
    wave_copy(h.ti, p.tr_ids + sf * p.max_out, nh, lane);
    assign_wave_sync();
}

// the frame of this wave: false when there is none. W waves of a workgroup take W consecutive frames.
__device__ inline bool my_frame(const HotaEval& p, int wave, int waves, int& s, int& f) {
    const int groups = (p.F + waves - 1) / waves;
    s = (int)(blockIdx.x / (unsigned)groups);
    f = (int)(blockIdx.x % (unsigned)groups) * waves + wave;
    int nf = p.frames ? p.frames[s] : p.F;
    nf = __builtin_amdgcn_readfirstlane(yh_hota_clampi(nf, p.F));
    return f < nf;
}

__device__ inline int uniform_count(const int* counts, size_t at, int cap) {
    return __builtin_amdgcn_readfirstlane(yh_hota_clampi(counts[at], cap));
}

using u64 = unsigned long long;
struct WsPtr {
    unsigned *P, *ng, *nt, *H, *ticket;
    u64* ctr;     // [num_thr][YH_HOTA_CTR], then GT rows, HYP rows, ignored GT, ignored HYP
};
__device__ inline WsPtr ws_at(const HotaEval& p, int s) {
    const yh_hota_ws w = yh_hota_layout(p.num_thr, p.n_gt_ids, p.n_tr_ids);
    char* b = p.ws + (size_t)s * w.bytes;
    WsPtr q;
    q.P = reinterpret_cast<unsigned*>(b + w.P);
    q.ng = reinterpret_cast<unsigned*>(b + w.ng);
    q.nt = reinterpret_cast<unsigned*>(b + w.nt);
    q.H = reinterpret_cast<unsigned*>(b + w.H);
    q.ctr = reinterpret_cast<u64*>(b + w.ctr);
    q.ticket = reinterpret_cast<unsigned*>(b + w.ticket);
    return q;
}

__global__ __launch_bounds__(256) void hota_zero(uint4* ws, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
        ws[i] = uint4{0, 0, 0, 0};
}

__global__ __launch_bounds__(64 * HOTA_COUNT_WAVES) void hota_count(const HotaEval p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int s, f;
    if (!my_frame(p, wave, HOTA_COUNT_WAVES, s, f)) return;
    const HotaLds m = hota_lds(p.max_gt, p.max_out);
    char* wb = smem + wave * m.count;
    const Staged h = staged_at(wb, m);
    int* Cl = reinterpret_cast<int*>(wb + m.staged);
    const size_t sf = (size_t)s * p.F + f;
    const int ng = uniform_count(p.gt_counts, sf, p.max_gt), nh = uniform_count(p.tr_counts, sf, p.max_out);
    const int ngi = p.n_gt_ids, nti = p.n_tr_ids, ca = p.class_aware;
    const WsPtr w = ws_at(p, s);

    for (int c = lane; c < nh; c += 64) Cl[c] = 0;
    stage(p, h, sf, ng, nh, lane);

    // the rows of this lane; who takes part
    int gid[HOTA_K], R[HOTA_K];
    int ngt = 0, nhyp = 0, ign_g = 0, ign_h = 0;
#pragma unroll
    for (int k = 0; k < HOTA_K; ++k) {
        gid[k] = -1;
        R[k] = 0;
        const int i = k * 64 + lane;
        if (k * 64 < ng && i < ng) {
            const int g = h.gi[i];
            if (yh_hota_id_ok(g, ngi)) {
                gid[k] = g;
                ++ngt;
                atomicAdd(&w.ng[g], 1u);
            } else {
                ++ign_g;
            }
        }
        if (k * 64 < nh && i < nh) {
            const int t = h.ti[i];
            if (yh_hota_id_ok(t, nti)) {
                ++nhyp;
                atomicAdd(&w.nt[t], 1u);
            } else {
                ++ign_h;
            }
        }
    }
    // first sweep: row sums in registers, column sums in LDS
    for (int c = 0; c < nh; ++c) {
        if (!yh_hota_id_ok(h.ti[c], nti)) continue;   // one address for the wave
        int part = 0;
#pragma unroll
        for (int k = 0; k < HOTA_K; ++k) {
            if (gid[k] < 0) continue;
            const int sim = yh_hota_pair_sim(h.gb + 5 * (k * 64 + lane), h.tb + 6 * c, ca);
            R[k] += sim;
            part += sim;
        }
        if (part) atomicAdd(&Cl[c], part);
    }
    assign_wave_sync();
    // second sweep: the Jaccard terms
    for (int c = 0; c < nh; ++c) {
        const int t = h.ti[c];
        if (!yh_hota_id_ok(t, nti)) continue;
        const int Cc = Cl[c];
        if (Cc == 0) continue;                        // nobody overlaps this column
#pragma unroll
        for (int k = 0; k < HOTA_K; ++k) {
            if (gid[k] < 0) continue;
            const int sim = yh_hota_pair_sim(h.gb + 5 * (k * 64 + lane), h.tb + 6 * c, ca);
            if (sim > 0) atomicAdd(&w.P[(size_t)gid[k] * nti + t], yh_hota_jaccard(sim, R[k], Cc));
        }
    }
    const long long GT = wave_sum(ngt), HYP = wave_sum(nhyp), IG = wave_sum(ign_g), IH = wave_sum(ign_h);
    if (lane == 0) {
        u64* tail = w.ctr + (size_t)p.num_thr * YH_HOTA_CTR;
        if (GT) atomicAdd(&tail[0], (u64)GT);
        if (HYP) atomicAdd(&tail[1], (u64)HYP);
        if (IG) atomicAdd(&tail[2], (u64)IG);
        if (IH) atomicAdd(&tail[3], (u64)IH);
    }
}

__global__ __launch_bounds__(64 * HOTA_MATCH_WAVES) void hota_match(const HotaEval p, int waves) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int s, f;
    if (!my_frame(p, wave, waves, s, f)) return;
    const HotaLds m = hota_lds(p.max_gt, p.max_out);
    char* wb = smem + (size_t)wave * m.match;
    const Staged h = staged_at(wb, m);
    AssignLds L;
    L.u = reinterpret_cast<int*>(wb + m.staged);
    L.ros = L.u + m.rg;
    L.sor = L.ros + m.rg;
    L.pred = L.sor + m.rt;
    L.v = nullptr;
    unsigned short* tile = reinterpret_cast<unsigned short*>(L.pred + m.rt);   // [max_gt][rt]
    const size_t sf = (size_t)s * p.F + f;
    const int ng = uniform_count(p.gt_counts, sf, p.max_gt), nh = uniform_count(p.tr_counts, sf, p.max_out);
    if (ng == 0 || nh == 0) return;
    const int ngi = p.n_gt_ids, nti = p.n_tr_ids, ca = p.class_aware, rt = m.rt;
    const WsPtr w = ws_at(p, s);
    stage(p, h, sf, ng, nh, lane);

    // the columns of this lane: their identity and its frame count
    int tid[HOTA_K];
    unsigned cnt_t[HOTA_K];
#pragma unroll
    for (int k = 0; k < HOTA_K; ++k) {
        const int c = k * 64 + lane;
        tid[k] = -1;
        cnt_t[k] = 0;
        if (k * 64 < nh && c < nh) {
            const int t = h.ti[c];
            if (yh_hota_id_ok(t, nti)) {
                tid[k] = t;
                cnt_t[k] = w.nt[t];
            }
        }
    }
    // the weight tile, a row per step
    for (int r = 0; r < ng; ++r) {
        const int g = h.gi[r];                         // one address for the wave
        const bool gok = yh_hota_id_ok(g, ngi);
        const unsigned cnt_g = gok ? w.ng[g] : 0u;
        int sim[HOTA_K];
        unsigned Pv[HOTA_K];
#pragma unroll
        for (int k = 0; k < HOTA_K; ++k) {
            sim[k] = (gok && tid[k] >= 0) ? yh_hota_pair_sim(h.gb + 5 * r, h.tb + 6 * (k * 64 + lane), ca) : 0;
            Pv[k] = sim[k] > 0 ? w.P[(size_t)g * nti + tid[k]] : 0u;
        }
#pragma unroll
        for (int k = 0; k < HOTA_K; ++k) {
            const int c = k * 64 + lane;
            if (k * 64 < nh && c < nh)
                tile[r * rt + c] = (unsigned short)yh_hota_weight(yh_hota_align(Pv[k], cnt_g, cnt_t[k]), sim[k]);
        }
    }
    assign_wave_sync();

    assign_solve<false>(L, ng, nh, lane, [&](int r, int c) { return (int)tile[r * rt + c]; });

    // the matched pairs, each under the highest level it reaches
    int level[HOTA_K], sv[HOTA_K];
#pragma unroll
    for (int k = 0; k < HOTA_K; ++k) {
        level[k] = -1;
        sv[k] = 0;
        const int r = k * 64 + lane;
        if (k * 64 >= ng || r >= ng) continue;
        const int c = L.ros[r];
        if (c < 0) continue;
        const float iou = yh_hota_iou(h.gb + 5 * r, h.tb + 6 * c);
        const int b = yh_hota_reached(iou, p.thr, p.num_thr) - 1;
        if (b < 0) continue;
        level[k] = b;
        sv[k] = yh_hota_sim(iou);
        atomicAdd(&w.H[((size_t)b * ngi + h.gi[r]) * nti + h.ti[c]], 1u);
    }
    for (int b = 0; b < p.num_thr; ++b) {
        int n = 0, loc = 0;
#pragma unroll
        for (int k = 0; k < HOTA_K; ++k) {
            if (k * 64 >= ng) continue;
            n += __popcll(__ballot(level[k] == b));
            loc += level[k] == b ? sv[k] : 0;
        }
        if (n == 0) continue;
        const long long LOC = wave_sum(loc);
        if (lane == 0) {
            atomicAdd(&w.ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_TP], (u64)n);
            atomicAdd(&w.ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_LOC], (u64)LOC);
        }
    }
}

__device__ inline u64 ctr_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(HOTA_CLOSE_THREADS) void hota_close(const HotaEval p, int tiles) {
    __shared__ int last_block;
    const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x, lane = tid & 63;
    const int ngi = p.n_gt_ids, nti = p.n_tr_ids, num_thr = p.num_thr;
    const size_t pairs = (size_t)ngi * nti, e = (size_t)tile * HOTA_CLOSE_THREADS + tid;
    const WsPtr w = ws_at(p, s);

    unsigned hl[YH_HOTA_MAX_THR], total = 0;
#pragma unroll
    for (int b = 0; b < YH_HOTA_MAX_THR; ++b) {
        hl[b] = (b < num_thr && e < pairs) ? w.H[(size_t)b * pairs + e] : 0u;
        total |= hl[b];
    }
    if (__ballot(total != 0)) {
        const unsigned cg = total ? w.ng[e / nti] : 1u, ct = total ? w.nt[e % nti] : 1u;
        unsigned mcount = 0;
        u64 a = 0, re = 0, pr = 0;
#pragma unroll
        for (int b = YH_HOTA_MAX_THR - 1; b >= 0; --b) {
            if (b >= num_thr) continue;
            mcount += hl[b];
            const u64 hit = __ballot(mcount > 0);
            if (!hit) continue;
            if (hl[b] != 0) {                         // the terms change only where the count does
                uint64_t ta, tre, tpr;
                yh_hota_terms(mcount, cg, ct, &ta, &tre, &tpr);
                a = ta, re = tre, pr = tpr;
            }
            const long long A = wave_sum((long long)a), RE = wave_sum((long long)re), PR = wave_sum((long long)pr);
            if (lane == 0) {
                u64* k = w.ctr + (size_t)b * YH_HOTA_CTR;
                atomicAdd(&k[YH_HOTA_C_ASSA], (u64)A);
                atomicAdd(&k[YH_HOTA_C_ASSRE], (u64)RE);
                atomicAdd(&k[YH_HOTA_C_ASSPR], (u64)PR);
                atomicAdd(&k[YH_HOTA_C_PAIRS], (u64)__popcll(hit));
            }
        }
    }

    // the last workgroup of the sequence writes its outputs
    __threadfence();
    __syncthreads();
    if (tid == 0) last_block = atomicAdd(w.ticket, 1u) == (unsigned)tiles - 1u;
    __syncthreads();
    if (!last_block) return;
    __threadfence();
    const u64* tail = w.ctr + (size_t)num_thr * YH_HOTA_CTR;
    const long long GT = (long long)ctr_load(&tail[0]), HYP = (long long)ctr_load(&tail[1]);
    for (int t = tid; t < num_thr; t += HOTA_CLOSE_THREADS) {
        const int rank = yh_hota_rank(p.thr, num_thr, t);
        long long tp = 0, loc = 0;
        for (int b = rank; b < num_thr; ++b) {
            tp += (long long)ctr_load(&w.ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_TP]);
            loc += (long long)ctr_load(&w.ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_LOC]);
        }
        const bool met = rank < num_thr;
        const u64* k = w.ctr + (size_t)(met ? rank : 0) * YH_HOTA_CTR;
        long long* o = p.out + ((size_t)s * num_thr + t) * YH_HOTA_OUT;
        o[YH_HOTA_TP] = tp;
        o[YH_HOTA_FP] = HYP - tp;
        o[YH_HOTA_FN] = GT - tp;
        o[YH_HOTA_LOC] = loc;
        o[YH_HOTA_ASSA] = met ? (long long)ctr_load(&k[YH_HOTA_C_ASSA]) : 0;
        o[YH_HOTA_ASSRE] = met ? (long long)ctr_load(&k[YH_HOTA_C_ASSRE]) : 0;
        o[YH_HOTA_ASSPR] = met ? (long long)ctr_load(&k[YH_HOTA_C_ASSPR]) : 0;
        o[YH_HOTA_PAIRS] = met ? (long long)ctr_load(&k[YH_HOTA_C_PAIRS]) : 0;
    }
    if (tid == 0) {
        p.rows[2 * s] = GT;
        p.rows[2 * s + 1] = HYP;
        p.ignored[2 * s] = (int)ctr_load(&tail[2]);
        p.ignored[2 * s + 1] = (int)ctr_load(&tail[3]);
    }
}

}  // namespace

int launch_hota_eval(const HotaEval& p, hipStream_t st) {
    // arguments were checked by yh_hota_eval (yh_hota_check, the workspace): the caps of include/yolo_hip.h hold
    if (p.sequences <= 0) return 0;
    const HotaLds m = hota_lds(p.max_gt, p.max_out);
    const size_t n16 = (size_t)p.sequences * yh_hota_layout(p.num_thr, p.n_gt_ids, p.n_tr_ids).bytes / 16;
    const size_t zero_blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(hota_zero, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(p.ws), n16);
    if (p.F > 0) {
        const int ga = (p.F + HOTA_COUNT_WAVES - 1) / HOTA_COUNT_WAVES;
        hipLaunchKernelGGL(hota_count, dim3((unsigned)p.sequences * ga), dim3(64 * HOTA_COUNT_WAVES),
                           HOTA_COUNT_WAVES * m.count, st, p);
    }
    if (p.F > 0 && p.max_gt > 0 && p.max_out > 0) {   // a side without rows has nothing to match
        if (int rc = lds_optin(reinterpret_cast<const void*>(hota_match), HOTA_LDS)) return rc;
        const int waves = m.match_waves < p.F ? m.match_waves : p.F;
        const int gb = (p.F + waves - 1) / waves;
        hipLaunchKernelGGL(hota_match, dim3((unsigned)p.sequences * gb), dim3(64 * waves), waves * m.match, st, p, waves);
    }
    const size_t pairs = (size_t)p.n_gt_ids * p.n_tr_ids;
    const int tiles = pairs ? (int)((pairs + HOTA_CLOSE_THREADS - 1) / HOTA_CLOSE_THREADS) : 1;
    hipLaunchKernelGGL(hota_close, dim3((unsigned)p.sequences * tiles), dim3(HOTA_CLOSE_THREADS), 0, st, p, tiles);
    return (int)hipGetLastError();
}

}  // namespace yh
