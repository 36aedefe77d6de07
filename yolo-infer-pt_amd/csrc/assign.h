// The assignment solver on the device, written once for yh_assign (csrc/assign.hip) and for the
// tracker's OPTIMAL associations (csrc/track.hip). The algorithm is stated at yh_assign in
// include/yolo_hip.h; csrc/assign_host.h's yh_assign_solve is the same thing sequentially.
//
// One wave solves one problem. Lane l owns the columns l, l + 64, ...: their distance, their dual
// and whether the search has scanned them stay in its registers (ASSIGN_K of each). What the wave
// addresses by a value it only learns in a step lives in LDS: the slots' duals, the matching in
// both directions and the predecessor links. A step of the search is: every lane relaxes its
// columns with the row of the slot that entered the tree, the wave finds the nearest column with a
// lane-exchange minimum over one 32-bit key per lane, and all lanes go on from that column - no
// barrier, since nothing leaves the wave. A key is (distance, column) packed; distances above
// MAX_WEIGHT all count as MAX_WEIGHT + 1, because the root's private column ends the search at
// MAX_WEIGHT at the latest, so such a column is never the choice.
//
// Every value that steers a branch is the same in all 64 lanes (read with a broadcast from LDS or
// the result of the wave minimum), and the loops are bounded by the column and slot counts.
#ifndef YH_ASSIGN_H
#define YH_ASSIGN_H

#include <hip/hip_runtime.h>

#include "assign_host.h"

namespace yh {

constexpr int ASSIGN_K = YH_ASSIGN_MAX_SIZE / 64;   // columns per lane at the cap
static_assert(YH_ASSIGN_MAX_SIZE % 64 == 0 && YH_ASSIGN_MAX_SIZE <= 1024, "a key holds a 10-bit column");
static_assert(((long long)(YH_ASSIGN_MAX_WEIGHT + 1) << 10 | 1023) < (1ll << 31), "a key is a positive int");

// the solver's words in LDS
struct AssignLds {
    int* u;      // [nt] slot duals
    int* ros;    // [nt] slot -> column or -1
    int* sor;    // [nd] column -> slot or -1
    int* pred;   // [nd] the slot a column was reached from
    int* v;      // [nd] column duals (LEAN only)
};
constexpr size_t assign_lds_words(int T, int D) { return 2 * (size_t)T + 2 * (size_t)D; }

// LDS written by one lane of the wave, read by another: order the two (the wave's LDS
// instructions execute in order; this keeps the compiler from moving them and waits for them)
__device__ inline void assign_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline int assign_wave_min(int k) {
    for (int m = 32; m > 0; m >>= 1) {
        const int o = __shfl_xor(k, m);
        k = o < k ? o : k;
    }
    return __builtin_amdgcn_readfirstlane(k);
}

// Called by all 64 lanes of one wave (lane: 0 .. 63). weight(t, d): the clamped weight of slot
// t < nt and column d < nd. On return L.ros / L.sor hold the matching, visible to the wave.
// LEAN = false (yh_assign): a lane fetches the weights of all its columns before it relaxes any, so
// that weights that come from global memory are in flight together, and keeps its columns' duals
// in registers. LEAN = true (the tracker, which computes its weights and has a track's state in
// registers besides): a weight is taken where it is used and the column duals live in L.v, each
// word touched by its owner lane only.
template <bool LEAN, class W>
__device__ void assign_solve(const AssignLds& L, int nt, int nd, int lane, W weight) {
    constexpr int M = YH_ASSIGN_MAX_WEIGHT;
    constexpr bool AHEAD = !LEAN;
    int dist[ASSIGN_K], v[LEAN ? 1 : ASSIGN_K];
#pragma unroll
    for (int k = 0; k < (LEAN ? 1 : ASSIGN_K); ++k) v[k] = 0;
    for (int t = lane; t < nt; t += 64) {
        L.u[t] = 0;
        L.ros[t] = -1;
    }
    for (int d = lane; d < nd; d += 64) {
        L.sor[d] = -1;
        if constexpr (LEAN) L.v[d] = 0;
    }
    assign_wave_sync();
    for (int root = 0; root < nt; ++root) {
#pragma unroll
        for (int k = 0; k < ASSIGN_K; ++k) dist[k] = YH_ASSIGN_INF;
        unsigned done = 0;                        // bit k: column lane + 64 k is scanned
        int i = root, base = 0;                   // the slot that entered the tree last, at which distance
        int pdist = YH_ASSIGN_INF, pslot = -1;    // the nearest private column
        int end = -1, total = 0;
        for (int step = 0; step <= nd; ++step) {
            const int ui = __builtin_amdgcn_readfirstlane(L.u[i]);
            const int pd = base + M - ui;
            if (pd < pdist || (pd == pdist && i < pslot)) {
                pdist = pd;
                pslot = i;
            }
            int ahead[AHEAD ? ASSIGN_K : 1];
            if constexpr (AHEAD) {
#pragma unroll
                for (int k = 0; k < ASSIGN_K; ++k) {
                    const int d = k * 64 + lane;
                    ahead[k] = (k * 64 < nd && d < nd && !((done >> k) & 1u)) ? weight(i, d) : 0;
                }
            }
            int key = INT_MAX;
#pragma unroll
            for (int k = 0; k < ASSIGN_K; ++k) {
                if (k * 64 >= nd) continue;       // the same for the wave
                const int d = k * 64 + lane;
                if (d >= nd || ((done >> k) & 1u)) continue;
                int w;
                if constexpr (AHEAD) w = ahead[k];
                else w = weight(i, d);
                if (w > 0) {
                    int vd;
                    if constexpr (LEAN) vd = L.v[d];
                    else vd = v[k];
                    const int cand = base + (M - w) - ui - vd;
                    if (cand < dist[k]) {
                        dist[k] = cand;
                        L.pred[d] = i;
                    }
                }
                const int kk = ((dist[k] > M ? M + 1 : dist[k]) << 10) | d;
                key = kk < key ? kk : key;
            }
            key = assign_wave_min(key);
            const int best = key == INT_MAX ? YH_ASSIGN_INF : key >> 10;
            if (best > pdist) {                   // a real column wins a tie with a private one
                total = pdist;
                break;
            }
            const int bj = key & 1023;
            if ((bj & 63) == lane) done |= 1u << (bj >> 6);
            const int owner = __builtin_amdgcn_readfirstlane(L.sor[bj]);
            if (owner < 0) {
                end = bj;
                total = best;
                break;
            }
            i = owner;
            base = best;
        }
        // the duals
        if (lane == 0) L.u[root] += total;
#pragma unroll
        for (int k = 0; k < ASSIGN_K; ++k) {
            const int d = k * 64 + lane;
            if (!((done >> k) & 1u) || d == end) continue;
            const int delta = total - dist[k];
            if constexpr (LEAN) L.v[d] -= delta;
            else v[k] -= delta;
            L.u[L.sor[d]] += delta;               // a column's slot is its own: no two lanes meet
        }
        assign_wave_sync();
        // the flip, from the end of the path back to the root
        if (lane == 0) {
            int d = end;
            bool more = true;
            if (d < 0) {
                d = L.ros[pslot];
                L.ros[pslot] = -1;
                more = pslot != root;
            }
            for (int guard = 0; more && guard <= nt; ++guard) {
                const int t = L.pred[d];
                const int next = L.ros[t];
                L.ros[t] = d;
                L.sor[d] = t;
                more = t != root;
                d = next;
            }
        }
        assign_wave_sync();
    }
}

}  // namespace yh

#endif
