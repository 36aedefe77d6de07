// Internal interface of csrc/assign_host.cpp (HIP-free): the argument check shared by yh_assign
// and yh_assign_host, the weight arithmetic shared by the kernel (csrc/assign.h, csrc/track.hip)
// and the host twins, and the sequential solver itself as a template over the weight lookup, so
// that the tracker's host twin (csrc/track_host.cpp) runs the very code yh_assign_host runs. The
// algorithm is stated at yh_assign in include/yolo_hip.h.
#ifndef YH_ASSIGN_HOST_H
#define YH_ASSIGN_HOST_H

#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "box_math.h"
#include "yolo_hip.h"

// Every dual and every tentative distance stays below this: a root's path is never longer than its
// private column's cost MAX_WEIGHT, a dual moves by at most that per augmentation, there are at
// most YH_ASSIGN_MAX_SIZE augmentations, and a tentative distance is a path length plus a reduced
// cost (cost + |dual|).
constexpr int YH_ASSIGN_BOUND = 1 << 27;
constexpr int YH_ASSIGN_INF = INT_MAX;   // the distance of a column no edge has reached
static_assert(YH_ASSIGN_MAX_WEIGHT == (1 << 16), "the weight of yh_trk_weight's value 1.0");
static_assert((long long)(YH_ASSIGN_MAX_SIZE + 2) * YH_ASSIGN_MAX_WEIGHT < YH_ASSIGN_BOUND, "duals and distances fit");
static_assert(YH_ASSIGN_BOUND < YH_ASSIGN_INF / 2, "a distance never reaches the infinity mark");
static_assert(YH_ASSIGN_MAX_SIZE >= YH_TRACK_MAX_TRACKS && YH_ASSIGN_MAX_SIZE >= YH_TRACK_MAX_DET, "the tracker's caps");

// a weight as the solver reads it
YH_HD int yh_assign_clamp(int w) { return w < 0 ? 0 : (w > YH_ASSIGN_MAX_WEIGHT ? YH_ASSIGN_MAX_WEIGHT : w); }

// the tracker's weight of a candidate pair of sort value val (OPTIMAL mode): one fp32 multiply,
// a truncation, the clamp to [1, MAX_WEIGHT]
YH_HD int yh_trk_weight(float val) {
    const float s = val * 65535.0f;
    if (!(s > 0.0f)) return 1;
    if (s >= 65535.0f) return YH_ASSIGN_MAX_WEIGHT;
    return 1 + (int)s;
}

// The solver, sequentially. weight(t, d) -> the clamped weight of slot t < nt and row d < nd.
// row_of_slot[0 .. nt) and slot_of_row[0 .. nd) are written (-1: unmatched).
template <class W>
void yh_assign_solve(int nt, int nd, W weight, int* row_of_slot, int* slot_of_row) {
    constexpr int M = YH_ASSIGN_MAX_WEIGHT;
    std::vector<int> u(nt, 0), v(nd, 0), dist(nd), pred(nd);
    std::vector<char> done(nd);
    for (int t = 0; t < nt; ++t) row_of_slot[t] = -1;
    for (int d = 0; d < nd; ++d) slot_of_row[d] = -1;
    for (int root = 0; root < nt; ++root) {
        for (int d = 0; d < nd; ++d) {
            dist[d] = YH_ASSIGN_INF;
            pred[d] = -1;
            done[d] = 0;
        }
        int i = root, base = 0;           // the slot that entered the tree last, and at which distance
        int pdist = YH_ASSIGN_INF, pslot = -1;   // the nearest private column
        int end = -1, total = 0;          // the free real column the path ends at (-1: pslot's private one)
        for (int step = 0; step <= nd; ++step) {
            const int ui = u[i];
            const int pd = base + M - ui;
            if (pd < pdist || (pd == pdist && i < pslot)) {
                pdist = pd;
                pslot = i;
            }
            int best = YH_ASSIGN_INF, bj = -1;
            for (int d = 0; d < nd; ++d) {
                if (done[d]) continue;
                const int w = weight(i, d);
                if (w > 0) {
                    const int nd2 = base + (M - w) - ui - v[d];
                    if (nd2 < dist[d]) {
                        dist[d] = nd2;
                        pred[d] = i;
                    }
                }
                if (dist[d] < best) {
                    best = dist[d];
                    bj = d;
                }
            }
            if (bj < 0 || best > pdist) {   // a real column wins a tie with a private one
                total = pdist;
                break;
            }
            done[bj] = 1;
            if (slot_of_row[bj] < 0) {
                end = bj;
                total = best;
                break;
            }
            i = slot_of_row[bj];
            base = best;
        }
        // the duals: the root and every slot of the tree move up by what its entry lay below the end
        u[root] += total;
        for (int d = 0; d < nd; ++d) {
            if (!done[d] || d == end) continue;
            const int delta = total - dist[d];
            u[slot_of_row[d]] += delta;
            v[d] -= delta;
        }
        // the flip, from the end of the path back to the root
        int d = end;
        if (d < 0) {
            const int t = pslot;
            d = row_of_slot[t];
            row_of_slot[t] = -1;
            if (t == root) continue;
        }
        for (int guard = 0; guard <= nt; ++guard) {
            const int t = pred[d];
            const int next = row_of_slot[t];
            row_of_slot[t] = d;
            slot_of_row[d] = t;
            if (t == root) break;
            d = next;
        }
    }
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_assign_check(const void* weights, int problems, int T, int D, const void* row_of_slot,
                            const void* slot_of_row);
const char* yh_assign_params_check(const yh_assign_params* ap);

// The host twin proper; arguments already checked. Problems run in parallel over `threads`.
int yh_assign_host_run(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts,
                       const int32_t* d_counts, int32_t* row_of_slot, int32_t* slot_of_row, int threads);

#endif
