// Batched assignment (yh_assign): one workgroup of one wave per problem solves a maximum-weight
// matching of its (T, D) weight matrix by successive shortest augmenting paths. The semantics are
// stated in include/yolo_hip.h, the solver is csrc/assign.h's (shared with the tracker), the host
// twin is csrc/assign_host.cpp. A step reads one row of the matrix: lane l its columns l, l + 64,
// ..., all of a lane's loads in flight together. No atomics, nothing passes between workgroups,
// no barrier: a single wave.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "assign.h"
#include "common.h"
#include "yolo_hip.h"

namespace yh {

namespace {

__global__ __launch_bounds__(64) void assign_kernel(const int* __restrict__ weights, int T, int D,
                                                    const int* __restrict__ t_counts,
                                                    const int* __restrict__ d_counts, int* __restrict__ row_of_slot,
                                                    int* __restrict__ slot_of_row) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AssignLds L;
    L.u = reinterpret_cast<int*>(smem);
    L.ros = L.u + T;
    L.sor = L.ros + T;
    L.pred = L.sor + D;
    L.v = nullptr;
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    int nt = t_counts ? t_counts[p] : T;     // one address for the wave: uniform
    int nd = d_counts ? d_counts[p] : D;
    nt = nt < 0 ? 0 : (nt > T ? T : nt);
    nd = nd < 0 ? 0 : (nd > D ? D : nd);
    const int* w = weights + (size_t)p * T * D;
    assign_solve<false>(L, nt, nd, lane, [w, D](int t, int d) { return yh_assign_clamp(w[(size_t)t * D + d]); });
    int* ros = row_of_slot + (size_t)p * T;
    int* sor = slot_of_row + (size_t)p * D;
    for (int t = lane; t < T; t += 64) ros[t] = t < nt ? L.ros[t] : -1;
    for (int d = lane; d < D; d += 64) sor[d] = d < nd ? L.sor[d] : -1;
}

}  // namespace

int launch_assign(const int* weights, int problems, int T, int D, const int* t_counts, const int* d_counts,
                  int* row_of_slot, int* slot_of_row, hipStream_t s) {
    // arguments were checked by yh_assign (yh_assign_check): 0 <= T, D <= YH_ASSIGN_MAX_SIZE
    if (problems <= 0 || (T == 0 && D == 0)) return 0;
    hipLaunchKernelGGL(assign_kernel, dim3(problems), dim3(64), assign_lds_words(T, D) * 4, s, weights, T, D, t_counts,
                       d_counts, row_of_slot, slot_of_row);
    return (int)hipGetLastError();
}

}  // namespace yh
