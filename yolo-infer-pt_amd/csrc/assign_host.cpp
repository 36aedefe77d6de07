// Host (CPU) twin of the batched assignment solver (csrc/assign.hip), and the argument check both
// entry points share. HIP-free on purpose: this file compiles alone with any C++17 compiler. The
// algorithm - stated at yh_assign in include/yolo_hip.h - is csrc/assign_host.h's template; here it
// runs on a weight matrix in memory.
#include "assign_host.h"

#include <algorithm>

#include "host_parallel.h"

const char* yh_assign_check(const void* weights, int problems, int T, int D, const void* row_of_slot,
                            const void* slot_of_row) {
    if (problems < 0) return "problems must be >= 0";
    if (T < 0 || D < 0) return "T and D must be >= 0";
    if (T > YH_ASSIGN_MAX_SIZE || D > YH_ASSIGN_MAX_SIZE) return "T or D exceeds YH_ASSIGN_MAX_SIZE (" YH_STR(YH_ASSIGN_MAX_SIZE) ")";
    if (problems > 0 && T > 0 && D > 0 && !weights) return "null weights";
    if (problems > 0 && T > 0 && !row_of_slot) return "null row_of_slot";
    if (problems > 0 && D > 0 && !slot_of_row) return "null slot_of_row";
    return nullptr;
}

const char* yh_assign_params_check(const yh_assign_params* ap) {
    if (!ap) return "null assign params";
    if (ap->mode != YH_ASSIGN_GREEDY && ap->mode != YH_ASSIGN_OPTIMAL) return "assign mode must be YH_ASSIGN_GREEDY or YH_ASSIGN_OPTIMAL";
    return nullptr;
}

int yh_assign_host_run(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts,
                       const int32_t* d_counts, int32_t* row_of_slot, int32_t* slot_of_row, int threads) {
    yh::parallel_strided(problems, threads, [&](int p) {
        const int nt = t_counts ? std::min(std::max(t_counts[p], 0), T) : T;
        const int nd = d_counts ? std::min(std::max(d_counts[p], 0), D) : D;
        const int32_t* w = weights + (size_t)p * T * D;
        int32_t* ros = row_of_slot + (size_t)p * T;
        int32_t* sor = slot_of_row + (size_t)p * D;
        yh_assign_solve(nt, nd, [&](int t, int d) { return yh_assign_clamp(w[(size_t)t * D + d]); }, ros, sor);
        std::fill(ros + nt, ros + T, -1);
        std::fill(sor + nd, sor + D, -1);
    });
    return 0;
}
