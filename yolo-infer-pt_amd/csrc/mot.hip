// Tracking evaluation (yh_mot_eval): the CLEAR-MOT counts and IDF1 of a batch of sequences at a
// list of IoU thresholds, in one launch. The rules are stated in include/yolo_hip.h, the pair
// arithmetic is csrc/mot_host.h's (shared with the host twin csrc/mot_host.cpp), the assignments
// are csrc/assign.h's solver (shared with yh_assign and the tracker).
//
// Work split. One workgroup per sequence, one wave per threshold. The frames of a sequence depend
// on each other (the carry, the last matched id), the thresholds do not: a wave walks the frames
// of its threshold alone and meets the others only where the next frame is staged.
//
// Staging. While the waves work on frame f, all of them copy frame f + 1 - boxes, classes and ids
// of both sides as they lie in memory, and a byte map "track id -> row" - into the other half of a
// double buffer in LDS: 16-byte loads for the whole quads of a frame whose address allows them,
// single words for the rest, so that nothing beyond a frame's counts is read. One barrier per
// frame hands the half over. The id map is never cleared: a wave checks the row it names against
// the staged ids, so what an earlier frame left there is harmless.
//
// A wave's words in LDS: the solver's (u, ros, sor, pred, v: LEAN mode), `last` (per ground-truth
// id the last matched track id, int16, with a flag "matched in the previous live frame": the
// carry's condition), the ground-truth ids of the previous frame's matches (to drop that flag), the
// compacted slot and column lists (a byte per row), and one byte per hypothesis row "taken by the
// carry", which borrows the solver's pred words: they are dead between two solves.
//
// A frame, per wave: (1) every ground-truth row looks its carried partner up and bumps the overlap
// counts C of its allowed pairs; (2) last frame's flags are dropped and the rows the carry left are
// compacted with ballot prefix sums; (3) assign_solve<true> matches them, its weight functor reading
// the staged boxes; (4) every ground-truth row reads its match back, counts, and writes `last`.
// C lives in the caller's workspace, one uint16 block per wave, zeroed by the wave before the
// first frame; ids are distinct within a frame, so a bump is a plain load and store, ordered
// against the other frames' by the wave's fences. After the last frame the per-frame words are
// dead and assign_solve<false> solves the identity assignment on C in the same LDS, as many waves
// side by side as fit, the rest in further rounds.
//
// No atomics, no scratch; every loop is bounded by a count the whole wave shares.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign.h"
#include "common.h"
#include "mot_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int MOT_K = YH_MOT_MAX_ROWS / 64;   // rows per lane at the cap
constexpr int MOT_FLAG = 0x4000;              // in a `last` word: matched in the previous live frame
constexpr int MOT_ID = 0x3FF;                 // and the track id below it
static_assert(YH_MOT_MAX_ROWS % 64 == 0 && YH_MOT_MAX_IDS <= MOT_ID + 1, "a last word holds id and flag");

__host__ __device__ constexpr int up(int v, int m) { return (v + m - 1) / m * m; }

// The LDS map. Shared: two halves of {gt boxes, hypothesis boxes, gt ids, hypothesis ids, id map};
// then one block per wave. After the frames: one closing block per wave of a round, from 0.
struct MotLds {
    int rg, rt;             // rows per side, rounded up to quads
    int half, wave, close;  // bytes of a half, of a wave's block, of a closing solve
    int frame_total, close_waves, total;
};
__host__ __device__ constexpr MotLds mot_lds(int max_gt, int max_out, int n_gt_ids, int n_tr_ids, int num_thr) {
    MotLds m{};
    m.rg = up(max_gt, 4);
    m.rt = up(max_out, 4);
    m.half = (m.rg * 5 + m.rt * 6 + m.rg + m.rt) * 4 + up(n_tr_ids, 16);
    m.wave = up((2 * m.rg + 3 * m.rt) * 4 + up(n_gt_ids * 2, 4) + m.rg * 2 + m.rg + m.rt, 16);
    m.close = (int)assign_lds_words(n_gt_ids, n_tr_ids) * 4;
    m.frame_total = 2 * m.half + num_thr * m.wave;
    const int fit = m.close ? m.frame_total / m.close : num_thr;
    m.close_waves = fit < 1 ? 1 : (fit > num_thr ? num_thr : fit);
    m.total = m.frame_total > m.close ? m.frame_total : m.close;
    return m;
}
static_assert(mot_lds(YH_MOT_MAX_ROWS, YH_MOT_MAX_ROWS, YH_MOT_MAX_IDS, YH_MOT_MAX_IDS, YH_MOT_MAX_THR).total == YH_MOT_LDS_AT_CAPS &&
                  YH_MOT_LDS_AT_CAPS <= 160 * 1024,
              "the budget stated in the header");

// a staged frame
struct Half {
    float* gb;           // [rg][5]
    float* tb;           // [rt][6]
    int* gi;             // [rg]
    int* ti;             // [rt]
    unsigned char* row;  // [n_tr_ids] track id -> row, to be checked against ti
};
__device__ inline Half half_at(char* base, const MotLds& m) {
    Half h;
    h.gb = reinterpret_cast<float*>(base);
    h.tb = h.gb + m.rg * 5;
    h.gi = reinterpret_cast<int*>(h.tb + m.rt * 6);
    h.ti = h.gi + m.rg;
    h.row = reinterpret_cast<unsigned char*>(h.ti + m.rt);
    return h;
}

// n words from global memory to LDS by the whole workgroup; dst is 16-byte aligned
__device__ inline void copy_words(int* dst, const int* src, int n, int tid, int nthreads) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {   // one address for the workgroup: uniform
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += nthreads) reinterpret_cast<int4*>(dst)[i] = reinterpret_cast<const int4*>(src)[i];
        done = n4 * 4;
    }
    for (int i = done + tid; i < n; i += nthreads) dst[i] = src[i];
}

__device__ inline int uniform_count(const int* counts, size_t at, int cap) {
    return __builtin_amdgcn_readfirstlane(yh_mot_clampi(counts[at], cap));
}

__device__ inline void stage(const MotEval& p, const Half& h, size_t sf, int tid, int nthreads) {
    const int ng = uniform_count(p.gt_counts, sf, p.max_gt), nh = uniform_count(p.tr_counts, sf, p.max_out);
    const int* ids = p.tr_ids + sf * p.max_out;
    copy_words(reinterpret_cast<int*>(h.gb), reinterpret_cast<const int*>(p.gt + sf * p.max_gt * 5), ng * 5, tid, nthreads);
    copy_words(reinterpret_cast<int*>(h.tb), reinterpret_cast<const int*>(p.tr + sf * p.max_out * 6), nh * 6, tid, nthreads);
    copy_words(h.gi, p.gt_ids + sf * p.max_gt, ng, tid, nthreads);
    copy_words(h.ti, ids, nh, tid, nthreads);
    for (int c = tid; c < nh; c += nthreads) {
        const int id = ids[c];
        if (yh_mot_id_ok(id, p.n_tr_ids)) h.row[id] = (unsigned char)c;
    }
}

// position of this lane among the set lanes of a wave-wide predicate, and their number
__device__ inline int prefix(bool set, int lane, int& total) {
    const unsigned long long m = __ballot(set);
    total = __popcll(m);
    return __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(64 * YH_MOT_MAX_THR) void mot_kernel(const MotEval p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const MotLds m = mot_lds(p.max_gt, p.max_out, p.n_gt_ids, p.n_tr_ids, p.num_thr);
    // the wave's block
    char* wb = smem + 2 * m.half + wave * m.wave;
    AssignLds L;
    L.u = reinterpret_cast<int*>(wb);
    L.ros = L.u + m.rg;
    L.sor = L.ros + m.rg;
    L.pred = L.sor + m.rt;
    L.v = L.pred + m.rt;
    short* last = reinterpret_cast<short*>(L.v + m.rt);
    unsigned short* prevg = reinterpret_cast<unsigned short*>(last + up(p.n_gt_ids * 2, 4) / 2);
    unsigned char* slist = reinterpret_cast<unsigned char*>(prevg + m.rg);
    unsigned char* clist = slist + m.rg;
    unsigned char* taken = reinterpret_cast<unsigned char*>(L.pred);

    const int F = p.F;
    int nf = p.frames ? p.frames[s] : F;
    nf = __builtin_amdgcn_readfirstlane(yh_mot_clampi(nf, F));
    const float a = p.thr[wave];
    const int ngi = p.n_gt_ids, nti = p.n_tr_ids, ca = p.class_aware;
    const size_t cbytes = yh_mot_c_bytes(ngi, nti);
    unsigned short* C = reinterpret_cast<unsigned short*>(p.C + ((size_t)s * p.num_thr + wave) * cbytes);

    for (int i = lane; i < ngi; i += 64) last[i] = -1;
    for (int i = lane; i < m.rt / 4; i += 64) L.pred[i] = 0;
    for (size_t i = lane; i < cbytes / 16; i += 64) reinterpret_cast<uint4*>(C)[i] = uint4{0, 0, 0, 0};
    if (nf > 0) stage(p, half_at(smem, m), (size_t)s * F, tid, nthreads);
    __syncthreads();

    int tp = 0, idsw = 0, ngt = 0, nhyp = 0, ign_g = 0, ign_h = 0, nprev = 0;
    long long siou = 0;
    for (int f = 0; f < nf; ++f) {
        const size_t sf = (size_t)s * F + f;
        if (f + 1 < nf) stage(p, half_at(smem + ((f + 1) & 1) * m.half, m), sf + 1, tid, nthreads);
        const Half h = half_at(smem + (f & 1) * m.half, m);
        const int ng = uniform_count(p.gt_counts, sf, p.max_gt), nh = uniform_count(p.tr_counts, sf, p.max_out);
        auto weight = [&](int r, int c) { return yh_mot_weight(h.gb + 5 * r, h.tb + 6 * c, ca, a); };

        // (1) the carry and the overlap counts
        int gid[MOT_K], crow[MOT_K], spos[MOT_K];
#pragma unroll
        for (int k = 0; k < MOT_K; ++k) {
            gid[k] = crow[k] = spos[k] = -1;
            const int r = k * 64 + lane;
            if (k * 64 >= ng || r >= ng) continue;
            const int g = h.gi[r];
            if (!yh_mot_id_ok(g, ngi)) {
                ++ign_g;
                continue;
            }
            gid[k] = g;
            ++ngt;
            const int lw = last[g];
            if (lw >= 0 && (lw & MOT_FLAG)) {
                const int t = lw & MOT_ID, c = h.row[t];
                if (c < nh && h.ti[c] == t) {
                    const int w = weight(r, c);
                    if (w > 0) {
                        crow[k] = c;
                        taken[c] = 1;
                        ++tp;
                        siou += w - 1;
                    }
                }
            }
        }
        for (int c = 0; c < nh; ++c) {
            const int t = h.ti[c];                 // one address for the wave
            if (!yh_mot_id_ok(t, nti)) continue;
#pragma unroll
            for (int k = 0; k < MOT_K; ++k)
                if (gid[k] >= 0 && weight(k * 64 + lane, c) > 0) ++C[(size_t)gid[k] * nti + t];
        }
        assign_wave_sync();

        // (2) last frame's matches lose their flag; the rows the carry left, in ascending order
        int ns = 0, nc = 0;
#pragma unroll
        for (int k = 0; k < MOT_K; ++k) {
            const int i = k * 64 + lane;
            if (i < nprev) {
                const int g = prevg[i];
                if (g != 0xFFFF) last[g] &= ~MOT_FLAG;
            }
            if (k * 64 < ng) {
                const bool rest = gid[k] >= 0 && crow[k] < 0;
                int n;
                const int at = ns + prefix(rest, lane, n);
                if (rest) {
                    slist[at] = (unsigned char)i;
                    spos[k] = at;
                }
                ns += n;
            }
            if (k * 64 < nh) {
                const bool live = i < nh && yh_mot_id_ok(h.ti[i], nti);
                nhyp += live;
                ign_h += i < nh && !live;
                const bool rest = live && !taken[i];
                int n;
                const int at = nc + prefix(rest, lane, n);
                if (rest) clist[at] = (unsigned char)i;
                nc += n;
            }
        }
        assign_wave_sync();

        // (3) the assignment of the rest
        const bool solved = ns > 0 && nc > 0;
        if (solved) assign_solve<true>(L, ns, nc, lane, [&](int sl, int cl) { return weight(slist[sl], clist[cl]); });

        // (4) the counts
#pragma unroll
        for (int k = 0; k < MOT_K; ++k) {
            const int r = k * 64 + lane;
            if (k * 64 >= ng || r >= ng) continue;
            int c = crow[k];
            if (c < 0 && solved && spos[k] >= 0) {
                const int col = L.ros[spos[k]];
                if (col >= 0) {
                    c = clist[col];
                    ++tp;
                    siou += weight(r, c) - 1;
                }
            }
            if (c >= 0) {
                const int t = h.ti[c], lw = last[gid[k]];
                if (lw >= 0 && (lw & MOT_ID) != t) ++idsw;
                last[gid[k]] = (short)(t | MOT_FLAG);
            }
            prevg[r] = c >= 0 ? (unsigned short)gid[k] : (unsigned short)0xFFFF;
        }
        nprev = ng;
        for (int i = lane; i < m.rt / 4; i += 64) L.pred[i] = 0;   // nobody is taken in the next frame yet
        __syncthreads();
    }

    // the identity assignment on C, in the LDS the frames have left
    long long idtp = 0;
    const int rounds = (p.num_thr + m.close_waves - 1) / m.close_waves;
    for (int round = 0; round < rounds; ++round) {
        if (wave / m.close_waves == round && ngi > 0 && nti > 0) {
            AssignLds I;
            I.u = reinterpret_cast<int*>(smem + (size_t)(wave % m.close_waves) * m.close);
            I.ros = I.u + ngi;
            I.sor = I.ros + ngi;
            I.pred = I.sor + nti;
            I.v = nullptr;
            assign_solve<false>(I, ngi, nti, lane, [&](int g, int t) { return yh_assign_clamp((int)C[(size_t)g * nti + t]); });
            for (int g = lane; g < ngi; g += 64) {
                const int t = I.ros[g];
                if (t >= 0) idtp += C[(size_t)g * nti + t];
            }
        }
        if (round + 1 < rounds) __syncthreads();
    }

    const long long TP = wave_sum(tp), GT = wave_sum(ngt), HYP = wave_sum(nhyp), SW = wave_sum(idsw);
    const long long SI = wave_sum(siou), ID = wave_sum(idtp), IG = wave_sum(ign_g), IH = wave_sum(ign_h);
    if (lane == 0) {
        long long* o = p.out + ((size_t)s * p.num_thr + wave) * YH_MOT_OUT;
        o[YH_MOT_TP] = TP;
        o[YH_MOT_FP] = HYP - TP;
        o[YH_MOT_FN] = GT - TP;
        o[YH_MOT_IDSW] = SW;
        o[YH_MOT_SIOU] = SI;
        o[YH_MOT_IDTP] = ID;
        o[YH_MOT_GT] = GT;
        o[YH_MOT_HYP] = HYP;
        if (wave == 0) {
            p.ignored[2 * s] = (int)IG;
            p.ignored[2 * s + 1] = (int)IH;
        }
    }
}

}  // namespace

int launch_mot_eval(const MotEval& p, hipStream_t s) {
    // arguments were checked by yh_mot_eval (yh_mot_check): the caps of include/yolo_hip.h hold
    if (p.sequences <= 0) return 0;
    const MotLds m = mot_lds(p.max_gt, p.max_out, p.n_gt_ids, p.n_tr_ids, p.num_thr);
    if (int rc = lds_optin(reinterpret_cast<const void*>(mot_kernel), YH_MOT_LDS_AT_CAPS)) return rc;
    hipLaunchKernelGGL(mot_kernel, dim3(p.sequences), dim3(64 * p.num_thr), m.total, s, p);
    return (int)hipGetLastError();
}

}  // namespace yh
