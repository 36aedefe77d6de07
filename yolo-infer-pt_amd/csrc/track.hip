// Multi-stream tracker (yh_track): one launch advances every video stream of a batch by one frame
// through its track table - predict, three IoU associations, Kalman update, births, output. The
// semantics are stated in include/yolo_hip.h; the host twin is csrc/track_host.cpp, and the
// arithmetic of a track and the state layout are shared with it through csrc/track_host.h.
//
// One workgroup of TRACK_T threads per batch row, no communication between workgroups, no
// atomics. TRACK_T equals both caps, so thread i owns slot i (its Kalman state stays in registers
// from the load to the single store at the end) and detection row i.
//   phase 1  the owners predict their slots and classify their rows; predicted boxes, classes and
//            the rows go to LDS;
//   phase 2  three associations, each in rounds of mutual best matching instead of the sorted
//            walk. A round compacts the slots and rows still live into index lists (one workgroup
//            prefix sum for both), then (A) every live slot finds its best live row, (B) every
//            live row finds its best live slot and matches it when that slot chose the row, (C)
//            the matched pairs leave both sides; until a round matches nothing or a side is
//            empty. A slot (row) is scanned by a
//            group of G consecutive lanes, G the largest power of two that keeps all 1024 threads
//            at most busy, and the group's best is reduced with lane exchanges. "Best" is the
//            largest 64-bit key (ordered IoU bits above the inverted index), i.e. the strict pair
//            order of the specification, under which a mutually best pair is exactly one the
//            sorted greedy walk takes (no pair sharing a side with it comes earlier), so the
//            rounds end in the walk's matching. IoUs are recomputed each round: there is no
//            slots x rows matrix, and because the lists shrink with every round the groups grow:
//            late rounds are short. Five barriers per round;
//   phase 3  the owners update or age their slots; two prefix sums (free slots, eligible rows)
//            hand the k-th eligible row to the k-th free slot;
//   phase 4  a prefix sum over the rows that own an output (matched, or born in frame 1) gives
//            the output order; the tails are zeroed, the state is stored.
// Every loop bound and every exit around a barrier is workgroup-uniform: read from LDS after a
// barrier (prefix-sum totals, the round word, the header words) or derived from kernel arguments.
// Rows at or beyond the count are never read: they are uninitialised memory.
// LDS: 9 words per slot + 7 per row (64 KiB at the caps, 18 KiB at 256 x 300), requested per
// launch. In the scans all groups of a wave read the same list entries (broadcasts) and a group's
// lanes consecutive ones.
// Built with -ffp-contract=off: every formula must round exactly as in the host twin.
//
// yh_track_reid is the same kernel, instantiated with APP: its first association takes a pair's
// candidacy and sort value from yh_trk_pair_reid, with the dot products the similarity launch in
// front of it (csrc/reid.hip) left in the workspace, as sim (T, D) and as its transpose, so that a
// slot's walk over the rows and a row's walk over the slots both read neighbouring entries, four
// of them in flight per lane. Which slots and rows have a feature comes from the workspace too (a
// word more per slot and per row in LDS). The galleries are not touched here: the kernel leaves
// each slot's row of this frame in the workspace for the gallery launch behind it.
//
// OPT (yh_track2 / yh_track_reid2 in YH_ASSIGN_OPTIMAL mode): a second instance of each, whose
// associations keep the candidate pairs but choose among them with yh_assign's solver
// (csrc/assign.h) instead of the rounds: the live slots and rows are compacted as above, wave 0
// solves the assignment over the two lists - the weights come from the boxes in LDS (and sim) as
// the solver asks for them, there is no slots x rows matrix here either - while the other waves
// wait at the barrier behind it; then the slot owners note their rows. Three words more per row in
// LDS (the solver's column links and duals). The greedy instances are compiled as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign.h"
#include "common.h"
#include "track_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int TRACK_T = 1024;                 // threads per workgroup (16 waves)
constexpr int TRACK_WAVES = TRACK_T / 64;
static_assert(YH_TRACK_MAX_TRACKS <= TRACK_T && YH_TRACK_MAX_DET <= TRACK_T, "a thread owns one slot and one row");

// app: the appearance instance (yh_track_reid) keeps a word more per slot and per row
// opt: the assignment instance keeps the solver's three words per row (its per-slot words reuse sact and best)
constexpr size_t track_lds(int T, int D, bool app = false, bool opt = false) {
    return ((size_t)(app ? 10 : 9) * T + (size_t)((app ? 8 : 7) + (opt ? 3 : 0)) * D + 2 * TRACK_WAVES + 4) * 4;
}
// above the 64 KiB a workgroup gets by default at the caps: launch_track requests the size with the
// attribute csrc/merge.hip uses (up to 160 KiB per workgroup on gfx950)
static_assert(track_lds(YH_TRACK_MAX_TRACKS, YH_TRACK_MAX_DET, true, true) <= 160 * 1024, "LDS plan");

struct Lds {
    float *sx1, *sy1, *sx2, *sy2, *scls;   // [T] slot box and class
    int *sact, *mrow, *best, *slist;       // [T] still live in this association, matched row, best row / id, live list
    float *rx1, *ry1, *rx2, *ry2, *rcls;   // [D] row box and class
    int *mslot, *rlist;                    // [D] matched slot, live list
    int* wsum;                             // [2][TRACK_WAVES] prefix-sum wave totals
    int* ctl;                              // [0] last round that matched, [1] f, [2] ids handed out, [3] rows
    int *gnz, *qfl;                        // appearance only: [T] the gallery row is non-zero, [D] the row's flags
    int *asor, *apred, *av;                // assignment only: [D] the solver's column -> slot, predecessor, dual
};

// One pair of an association: a candidate, and with which sort value? APP: the first association
// of yh_track_reid; dot is the pair's entry of the similarity matrix (whatever the memory holds
// where a side has no feature: it is not used then).
template <bool APP>
__device__ inline bool pair_value(const Lds& L, const TrackReid& rd, int dot, int t, int d, const yh_track_box& tb,
                                  const yh_track_box& db, float thr, float& val) {
    if constexpr (APP) {
        const bool feat = L.gnz[t] && (L.qfl[d] & 2);
        return yh_trk_pair_reid(tb, db, thr, feat, dot, rd.cos_min, rd.iou_min, val);
    } else {
        return yh_trk_pair(tb, db, thr, val);
    }
}

// exclusive ranks of two flags over the workgroup (thread order) and their totals; the totals
// are read from LDS after a barrier: workgroup-uniform
__device__ inline void scan2(bool fa, bool fb, int* wsum, int lane, int wave, int& ra, int& na, int& rb, int& nb,
                             bool tail = true) {
    const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
    const unsigned long long below = (1ull << lane) - 1ull;
    ra = __popcll(ma & below);
    rb = __popcll(mb & below);
    if (lane == 0) {
        wsum[wave] = __popcll(ma);
        wsum[TRACK_WAVES + wave] = __popcll(mb);
    }
    __syncthreads();
    na = nb = 0;
    for (int w = 0; w < TRACK_WAVES; ++w) {
        const int ca = wsum[w], cb = wsum[TRACK_WAVES + w];
        if (w < wave) {
            ra += ca;
            rb += cb;
        }
        na += ca;
        nb += cb;
    }
    if (tail) __syncthreads();   // the next scan rewrites wsum (tail = false: the caller's next barrier does this)
}

// the largest key of a group of g consecutive lanes (g a power of two <= 64), in all of them
__device__ inline unsigned long long group_max(unsigned long long k, int g) {
    for (int m = g >> 1; m > 0; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, m);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        if (o > k) k = o;
    }
    return k;
}

// the pair order of the specification as one number: larger is earlier. Never 0 for a candidate.
__device__ inline unsigned long long pair_key(float iou, int index) {
    return ((unsigned long long)float_order(iou) << 32) | (0xFFFFFFFFu - (uint32_t)index);
}
__device__ inline int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// threads per scanned entity: all of a wave for a few entities, one for TRACK_T of them
__device__ inline int group_size(int n) {
    int g = 64;
    while (g > 1 && n * g > TRACK_T) g >>= 1;
    return g;
}

// assoc(T, D, thr) of the specification. slive / rlive: this thread's slot / row takes part (false
// for a thread without one). round: the workgroup's running round number (uniform). APP: pairs by
// pair_value<true> (sim (T, D): this batch row's similarities, sim_t (D, T): their transpose, so
// that the walk along a row of either scan reads neighbouring entries).
template <bool APP>
__device__ void assoc(const Lds& L, bool slive, bool rlive, float thr, int class_aware, int tid, int lane,
                      int wave, int& round, const TrackReid& rd, const int* __restrict__ sim,
                      const int* __restrict__ sim_t, int T, int D) {
    // APP: a lane takes U pairs at a time, so that their U similarities, which come from global
    // memory, are in flight together; the plain instance walks pair by pair as before
    constexpr int U = 4;
    if (slive) L.sact[tid] = 1;         // cleared by the row that takes the slot
    for (;;) {
        // the lists of the slots and rows still live: as pairs retire, more lanes share a scan
        int rs, ns, rr, nr;
        scan2(slive, rlive, L.wsum, lane, wave, rs, ns, rr, nr, false);
        if (slive) L.slist[rs] = tid;
        if (rlive) L.rlist[rr] = tid;
        __syncthreads();                // also frees wsum for the next scan
        if (ns == 0 || nr == 0) return;
        const int gs = group_size(ns), gr = group_size(nr);
        ++round;
        // (A) best live row of every live slot
        for (int e0 = 0; e0 < ns; e0 += TRACK_T / gs) {
            const int e = e0 + tid / gs, g = tid & (gs - 1);
            const int t = e < ns ? L.slist[e] : -1;
            unsigned long long bk = 0;
            if (t >= 0) {
                const yh_track_box tb{L.sx1[t], L.sy1[t], L.sx2[t], L.sy2[t]};
                const float tc = L.scls[t];
                auto consider = [&](int d, int dot) {
                    if (class_aware && !(tc == L.rcls[d])) return;
                    const yh_track_box db{L.rx1[d], L.ry1[d], L.rx2[d], L.ry2[d]};
                    float iou;
                    if (!pair_value<APP>(L, rd, dot, t, d, tb, db, thr, iou)) return;
                    const unsigned long long key = pair_key(iou, d);
                    if (key > bk) bk = key;
                };
                if constexpr (APP) {   // row t of sim: a group's lanes read neighbouring entries
                    for (int j0 = g; j0 < nr; j0 += gs * U) {
                        int dd[U], dot[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) dd[u] = j0 + u * gs < nr ? L.rlist[j0 + u * gs] : -1;
#pragma unroll
                        for (int u = 0; u < U; ++u) dot[u] = dd[u] >= 0 ? sim[(size_t)t * D + dd[u]] : 0;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (dd[u] >= 0) consider(dd[u], dot[u]);
                    }
                } else {
                    for (int j = g; j < nr; j += gs) consider(L.rlist[j], 0);
                }
            }
            bk = group_max(bk, gs);
            if (t >= 0 && g == 0) L.best[t] = bk ? key_index(bk) : -1;
        }
        __syncthreads();
        // (B) best live slot of every live row; a mutual choice is a match
        for (int e0 = 0; e0 < nr; e0 += TRACK_T / gr) {
            const int e = e0 + tid / gr, g = tid & (gr - 1);
            const int d = e < nr ? L.rlist[e] : -1;
            unsigned long long bk = 0;
            if (d >= 0) {
                const yh_track_box db{L.rx1[d], L.ry1[d], L.rx2[d], L.ry2[d]};
                const float dc = L.rcls[d];
                auto consider = [&](int t, int dot) {
                    if (class_aware && !(L.scls[t] == dc)) return;
                    const yh_track_box tb{L.sx1[t], L.sy1[t], L.sx2[t], L.sy2[t]};
                    float iou;
                    if (!pair_value<APP>(L, rd, dot, t, d, tb, db, thr, iou)) return;
                    const unsigned long long key = pair_key(iou, t);
                    if (key > bk) bk = key;
                };
                if constexpr (APP) {   // row d of the transpose: neighbouring entries again
                    for (int j0 = g; j0 < ns; j0 += gr * U) {
                        int tt[U], dot[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) tt[u] = j0 + u * gr < ns ? L.slist[j0 + u * gr] : -1;
#pragma unroll
                        for (int u = 0; u < U; ++u) dot[u] = tt[u] >= 0 ? sim_t[(size_t)d * T + tt[u]] : 0;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (tt[u] >= 0) consider(tt[u], dot[u]);
                    }
                } else {
                    for (int j = g; j < ns; j += gr) consider(L.slist[j], 0);
                }
            }
            bk = group_max(bk, gr);
            if (d >= 0 && g == 0 && bk) {
                const int t = key_index(bk);
                if (L.best[t] == d) {
                    L.mslot[d] = t;
                    L.ctl[0] = round;
                }
            }
        }
        __syncthreads();
        if (L.ctl[0] != round) break;   // nothing matched: the same word for every thread
        // (C) the row owners retire the new pairs (a live row has no slot until (B) gives it one)
        if (rlive && L.mslot[tid] >= 0) {
            const int t = L.mslot[tid];
            rlive = false;
            L.sact[t] = 0;
            L.mrow[t] = tid;
        }
        __syncthreads();
        slive = slive && L.sact[tid];
    }
}

// assoc(T, D, thr) of the specification in YH_ASSIGN_OPTIMAL mode: the same candidate pairs, the
// matching of yh_assign on their weights over the live slots and rows in ascending order.
template <bool APP>
__device__ void assoc_opt(const Lds& L, bool slive, bool rlive, float thr, int class_aware, int tid, int lane,
                          int wave, const TrackReid& rd, const int* __restrict__ sim, int D) {
    int rs, ns, rr, nr;
    scan2(slive, rlive, L.wsum, lane, wave, rs, ns, rr, nr, false);
    if (slive) L.slist[rs] = tid;
    if (rlive) L.rlist[rr] = tid;
    __syncthreads();                    // also frees wsum for the next scan
    if (ns == 0 || nr == 0) return;     // prefix-sum totals: the same for every thread
    const AssignLds A{L.best, L.sact, L.asor, L.apred, L.av};
    if (wave == 0) {
        assign_solve<true>(A, ns, nr, lane, [&](int a, int c) {
            const int t = L.slist[a], d = L.rlist[c];
            if (class_aware && !(L.scls[t] == L.rcls[d])) return 0;
            const yh_track_box tb{L.sx1[t], L.sy1[t], L.sx2[t], L.sy2[t]};
            const yh_track_box db{L.rx1[d], L.ry1[d], L.rx2[d], L.ry2[d]};
            int dot = 0;
            if constexpr (APP) dot = sim[(size_t)t * D + d];
            float val;
            if (!pair_value<APP>(L, rd, dot, t, d, tb, db, thr, val)) return 0;
            return yh_trk_weight(val);
        });
    }
    __syncthreads();
    if (slive) {                        // a live slot is the rs-th of the list
        const int c = A.ros[rs];
        if (c >= 0) {
            const int d = L.rlist[c];
            L.mrow[tid] = d;
            L.mslot[d] = tid;
        }
    }
    __syncthreads();
}

// APP: yh_track_reid. A stream's state is then stream_bytes long, its gallery behind the words
// of yh_track's state; rd is not read otherwise.
template <bool APP, bool OPT>
__global__ __launch_bounds__(TRACK_T) void track_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        int D, const int* __restrict__ stream_ids,
                                                        char* __restrict__ state, size_t stream_bytes, int streams,
                                                        int T, yh_track_params p, int max_out,
                                                        float* __restrict__ out, int* __restrict__ ids,
                                                        int* __restrict__ det_index, int* __restrict__ out_counts,
                                                        TrackReid rd) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Lds L;
    {
        float* at = reinterpret_cast<float*>(smem);
        L.sx1 = at; at += T;
        L.sy1 = at; at += T;
        L.sx2 = at; at += T;
        L.sy2 = at; at += T;
        L.scls = at; at += T;
        L.sact = reinterpret_cast<int*>(at); at += T;
        L.mrow = reinterpret_cast<int*>(at); at += T;
        L.best = reinterpret_cast<int*>(at); at += T;
        L.slist = reinterpret_cast<int*>(at); at += T;
        L.rx1 = at; at += D;
        L.ry1 = at; at += D;
        L.rx2 = at; at += D;
        L.ry2 = at; at += D;
        L.rcls = at; at += D;
        L.mslot = reinterpret_cast<int*>(at); at += D;
        L.rlist = reinterpret_cast<int*>(at); at += D;
        L.wsum = reinterpret_cast<int*>(at); at += 2 * TRACK_WAVES;
        L.ctl = reinterpret_cast<int*>(at); at += 4;
        L.gnz = reinterpret_cast<int*>(at);            // beyond the request unless APP: never touched then
        L.qfl = L.gnz + T;
        if constexpr (APP) at += T + D;
        L.asor = reinterpret_cast<int*>(at);           // likewise unless OPT
        L.apred = L.asor + D;
        L.av = L.apred + D;
    }
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    float* orow = out + (size_t)b * max_out * 6;
    int* oid = ids + (size_t)b * max_out;
    int* odet = det_index + (size_t)b * max_out;
    const int s = stream_ids ? stream_ids[b] : b;      // one address for the workgroup: uniform
    if (s < 0 || s >= streams) {                       // no such stream: zero rows, no state touched
        for (int i = tid; i < max_out * 6; i += TRACK_T) orow[i] = 0.0f;
        for (int i = tid; i < max_out; i += TRACK_T) {
            oid[i] = 0;
            odet[i] = 0;
        }
        if (tid == 0) out_counts[b] = 0;
        if constexpr (APP)
            for (int i = tid; i < T; i += TRACK_T) rd.code[(size_t)b * T + i] = -1;   // no gallery to update
        return;
    }
    uint32_t* w = reinterpret_cast<uint32_t*>(state + (size_t)s * stream_bytes);
    const int* sim = APP ? rd.sim + (size_t)b * T * D : nullptr;
    const int* sim_t = APP ? rd.sim_t + (size_t)b * T * D : nullptr;
    uint32_t* fld = w + YH_TRACK_HDR + tid;            // field i of this thread's slot: fld[i * T]
    if (tid == 0) {
        int n = counts[b];
        n = n < 0 ? 0 : (n > D ? D : n);
        L.ctl[0] = 0;
        L.ctl[1] = (int)w[0];
        L.ctl[2] = (int)w[1];
        L.ctl[3] = n;
    }
    __syncthreads();
    const int f = L.ctl[1] + 1;        // step 1: this frame
    const int nid = L.ctl[2];          // ids handed out so far
    const int n = L.ctl[3];            // rows of this frame, <= D

    // phase 1: this thread's slot ...
    const bool has_slot = tid < T;
    int st0 = 0, sid = 0, slast = 0;
    float scl = 0.0f;
    yh_track_kal k = {};
    if (has_slot) st0 = (int)fld[(size_t)YH_TRK_STATUS * T];
    if (st0 != 0) {
        sid = (int)fld[(size_t)YH_TRK_ID * T];
        slast = (int)fld[(size_t)YH_TRK_LAST * T];
        scl = __uint_as_float(fld[(size_t)YH_TRK_CLS * T]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k.x[i] = __uint_as_float(fld[(size_t)(YH_TRK_X + i) * T]);
            k.v[i] = __uint_as_float(fld[(size_t)(YH_TRK_V + i) * T]);
            k.a[i] = __uint_as_float(fld[(size_t)(YH_TRK_A + i) * T]);
            k.b[i] = __uint_as_float(fld[(size_t)(YH_TRK_B + i) * T]);
            k.c[i] = __uint_as_float(fld[(size_t)(YH_TRK_C + i) * T]);
        }
        yh_trk_predict(k, st0);
    }
    if (has_slot) {
        const yh_track_box pb = yh_trk_box(k);
        L.sx1[tid] = pb.x1;
        L.sy1[tid] = pb.y1;
        L.sx2[tid] = pb.x2;
        L.sy2[tid] = pb.y2;
        L.scls[tid] = scl;
        L.mrow[tid] = -1;
    }
    // ... and its row
    const bool has_row = tid < n;
    yh_track_box rb{0.0f, 0.0f, 0.0f, 0.0f};
    float rsc = 0.0f, rcl = 0.0f;
    int band = 0;                      // 2 high, 1 low, 0 neither
    if (has_row) {
        const float* d = dets + ((size_t)b * D + tid) * 6;
        rb.x1 = d[0]; rb.y1 = d[1]; rb.x2 = d[2]; rb.y2 = d[3];
        rsc = d[4];
        rcl = d[5];
        band = rsc >= p.track_high ? 2 : (rsc >= p.track_low ? 1 : 0);
    }
    if (tid < D) {
        L.rx1[tid] = rb.x1;
        L.ry1[tid] = rb.y1;
        L.rx2[tid] = rb.x2;
        L.ry2[tid] = rb.y2;
        L.rcls[tid] = rcl;
        L.mslot[tid] = -1;
    }
    if constexpr (APP) {
        // the rows' flags, and which slots hold a feature (found by the similarity launch, which
        // read every gallery row; without features nothing asks)
        if (tid < D) L.qfl[tid] = has_row ? rd.flags[(size_t)b * D + tid] : 0;
        if (has_slot) L.gnz[tid] = rd.gnz ? rd.gnz[(size_t)b * T + tid] : 0;
    }
    // phase 2 (the first barrier of each association's prefix sum orders the writes above)
    if constexpr (OPT) {
        assoc_opt<APP>(L, st0 == 2 || st0 == 3, band == 2, p.iou_first, p.class_aware, tid, lane, wave, rd, sim, D);
        assoc_opt<false>(L, st0 == 2 && L.mrow[tid] < 0, band == 1, p.iou_second, p.class_aware, tid, lane, wave, rd, sim,
                         D);
        assoc_opt<false>(L, st0 == 1, band == 2 && L.mslot[tid] < 0, p.iou_tentative, p.class_aware, tid, lane, wave, rd,
                         sim, D);
    } else {
        int round = 0;
        assoc<APP>(L, st0 == 2 || st0 == 3, band == 2, p.iou_first, p.class_aware, tid, lane, wave, round, rd, sim, sim_t,
                   T, D);
        assoc<false>(L, st0 == 2 && L.mrow[tid] < 0, band == 1, p.iou_second, p.class_aware, tid, lane, wave, round, rd,
                     sim, sim_t, T, D);
        assoc<false>(L, st0 == 1, band == 2 && L.mslot[tid] < 0, p.iou_tentative, p.class_aware, tid, lane, wave, round,
                     rd, sim, sim_t, T, D);
    }

    // phase 3: step 4 ...
    int st = st0;
    int myrow = -1;                    // the row this slot puts out
    if (st0 != 0) {
        const int d = L.mrow[tid];
        if (d >= 0) {
            yh_trk_update(k, yh_track_box{L.rx1[d], L.ry1[d], L.rx2[d], L.ry2[d]});
            st = 2;
            slast = f;
            scl = L.rcls[d];
            myrow = d;
        } else if (st0 == 2) {
            st = 3;
        } else if (st0 == 1) {
            st = 0;
        }
        if (st == 3 && f - slast > p.max_age) st = 0;
    }
    // ... and step 5: the k-th eligible row takes the k-th free slot
    const bool isfree = has_slot && st == 0;
    const bool elig = band == 2 && L.mslot[tid] < 0 && rsc >= p.track_new;
    int kf, nfree, ke, nelig;
    scan2(isfree, elig, L.wsum, lane, wave, kf, nfree, ke, nelig);
    if (elig) L.rlist[ke] = tid;
    __syncthreads();
    const int nborn = nfree < nelig ? nfree : nelig;
    const bool born = isfree && kf < nborn;
    if (born) {
        const int d = L.rlist[kf];
        yh_trk_birth(k, yh_track_box{L.rx1[d], L.ry1[d], L.rx2[d], L.ry2[d]});
        sid = nid + 1 + kf;
        slast = f;
        scl = L.rcls[d];
        st = f == 1 ? 2 : 1;
        if (f == 1) {                  // only these births are output: the others are tentative
            myrow = d;
            L.mslot[d] = tid;
        }
    }
    if constexpr (APP) {
        // the gallery's work of this slot, for the launch behind this one: its row of this frame,
        // born slots tagged
        if (has_slot) {
            int code = st0 != 0 ? L.mrow[tid] : -1;
            if (born) code = L.rlist[kf] | (1 << 30);
            rd.code[(size_t)b * T + tid] = code;
        }
    }
    // phase 4: step 6
    if (myrow >= 0) {
        const yh_track_box pb = yh_trk_box(k);
        L.sx1[tid] = pb.x1;
        L.sy1[tid] = pb.y1;
        L.sx2[tid] = pb.x2;
        L.sy2[tid] = pb.y2;
        L.best[tid] = sid;
    }
    __syncthreads();
    const bool emits = has_row && L.mslot[tid] >= 0;
    int ro, nout, unused0, unused1;
    scan2(emits, false, L.wsum, lane, wave, ro, nout, unused0, unused1);
    if (emits && ro < max_out) {
        const int t = L.mslot[tid];
        float* o = orow + (size_t)ro * 6;
        o[0] = L.sx1[t]; o[1] = L.sy1[t]; o[2] = L.sx2[t]; o[3] = L.sy2[t];
        o[4] = rsc; o[5] = rcl;
        oid[ro] = L.best[t];
        odet[ro] = tid;
    }
    const int cnt = nout < max_out ? nout : max_out;
    for (int i = cnt * 6 + tid; i < max_out * 6; i += TRACK_T) orow[i] = 0.0f;
    for (int i = cnt + tid; i < max_out; i += TRACK_T) {
        oid[i] = 0;
        odet[i] = 0;
    }
    // the state: every slot that held a track before or holds one now (a freed slot keeps its
    // predicted values, as in the host twin)
    if (st0 != 0 || born) {
        fld[(size_t)YH_TRK_STATUS * T] = (uint32_t)st;
        fld[(size_t)YH_TRK_ID * T] = (uint32_t)sid;
        fld[(size_t)YH_TRK_LAST * T] = (uint32_t)slast;
        fld[(size_t)YH_TRK_CLS * T] = __float_as_uint(scl);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fld[(size_t)(YH_TRK_X + i) * T] = __float_as_uint(k.x[i]);
            fld[(size_t)(YH_TRK_V + i) * T] = __float_as_uint(k.v[i]);
            fld[(size_t)(YH_TRK_A + i) * T] = __float_as_uint(k.a[i]);
            fld[(size_t)(YH_TRK_B + i) * T] = __float_as_uint(k.b[i]);
            fld[(size_t)(YH_TRK_C + i) * T] = __float_as_uint(k.c[i]);
        }
    }
    if (tid == 0) {
        out_counts[b] = cnt;
        w[0] = (uint32_t)f;
        w[1] = (uint32_t)(nid + nborn);
    }
}

// yh_track_warp: one workgroup per batch row, slots over threads; a slot's fields are a column of the
// field-major state, so neighbouring threads read and write neighbouring words. Free slots, the
// header and (behind the words) the gallery are not touched.
constexpr int WARP_T = 256;
__global__ __launch_bounds__(WARP_T) void track_warp_kernel(char* __restrict__ state, size_t stream_bytes, int streams,
                                                            int T, const float* __restrict__ motion,
                                                            const int* __restrict__ stream_ids) {
    const int b = blockIdx.x;
    const int s = stream_ids ? stream_ids[b] : b;      // one address for the workgroup: uniform
    if (s < 0 || s >= streams) return;
    const float m[3] = {motion[(size_t)b * 3], motion[(size_t)b * 3 + 1], motion[(size_t)b * 3 + 2]};
    if (!yh_trk_warp_valid(m)) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(state + (size_t)s * stream_bytes);
    for (int t = threadIdx.x; t < T; t += WARP_T) {
        uint32_t* fld = w + YH_TRACK_HDR + t;
        if (fld[(size_t)YH_TRK_STATUS * T] == 0u) continue;
        yh_track_kal k;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k.x[i] = __uint_as_float(fld[(size_t)(YH_TRK_X + i) * T]);
            k.v[i] = __uint_as_float(fld[(size_t)(YH_TRK_V + i) * T]);
            k.a[i] = __uint_as_float(fld[(size_t)(YH_TRK_A + i) * T]);
            k.b[i] = __uint_as_float(fld[(size_t)(YH_TRK_B + i) * T]);
            k.c[i] = __uint_as_float(fld[(size_t)(YH_TRK_C + i) * T]);
        }
        yh_trk_warp(k, m[0], m[1], m[2]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fld[(size_t)(YH_TRK_X + i) * T] = __float_as_uint(k.x[i]);
            fld[(size_t)(YH_TRK_V + i) * T] = __float_as_uint(k.v[i]);
            fld[(size_t)(YH_TRK_A + i) * T] = __float_as_uint(k.a[i]);
            fld[(size_t)(YH_TRK_B + i) * T] = __float_as_uint(k.b[i]);
            fld[(size_t)(YH_TRK_C + i) * T] = __float_as_uint(k.c[i]);
        }
    }
}

}  // namespace

int launch_track_warp(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                      const int* stream_ids, int batch, hipStream_t s) {
    // arguments were checked by yh_track_warp (yh_track_warp_check)
    if (batch <= 0 || streams <= 0) return 0;
    hipLaunchKernelGGL(track_warp_kernel, dim3(batch), dim3(WARP_T), 0, s, static_cast<char*>(state),
                       yh_track_warp_stride(max_tracks, reid_dim), streams, max_tracks, motion, stream_ids);
    return (int)hipGetLastError();
}

template <bool APP, bool OPT>
int launch(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
           size_t stream_bytes, int streams, int max_tracks, const yh_track_params& p, int max_out, float* out, int* ids,
           int* det_index, int* out_counts, const TrackReid& rd, hipStream_t s) {
    // arguments were checked by yh_track (yh_track_check): 1 <= max_tracks <= YH_TRACK_MAX_TRACKS,
    // 0 <= max_det <= YH_TRACK_MAX_DET
    if (batch <= 0) return 0;
    if (int rc = lds_optin(reinterpret_cast<const void*>(track_kernel<APP, OPT>),
                           (int)track_lds(YH_TRACK_MAX_TRACKS, YH_TRACK_MAX_DET, APP, OPT)))
        return rc;
    hipLaunchKernelGGL((track_kernel<APP, OPT>), dim3(batch), dim3(TRACK_T), track_lds(max_tracks, max_det, APP, OPT), s,
                       dets, counts, max_det, stream_ids, static_cast<char*>(state), stream_bytes, streams, max_tracks, p,
                       max_out, out, ids, det_index, out_counts, rd);
    return (int)hipGetLastError();
}

int launch_track(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                 int streams, int max_tracks, const yh_track_params& p, int max_out, float* out, int* ids,
                 int* det_index, int* out_counts, bool optimal, hipStream_t s) {
    const auto run = optimal ? launch<false, true> : launch<false, false>;
    return run(dets, counts, batch, max_det, stream_ids, state, yh_track_stream_words(max_tracks) * 4, streams, max_tracks,
               p, max_out, out, ids, det_index, out_counts, TrackReid{}, s);
}

int launch_track_reid(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                      int streams, int max_tracks, const yh_track_params& p, int max_out, float* out, int* ids,
                      int* det_index, int* out_counts, const TrackReid& rd, bool optimal, hipStream_t s) {
    const auto run = optimal ? launch<true, true> : launch<true, false>;
    return run(dets, counts, batch, max_det, stream_ids, state, yh_track_reid_stream_bytes(max_tracks, rd.dim), streams,
               max_tracks, p, max_out, out, ids, det_index, out_counts, rd, s);
}

}  // namespace yh
