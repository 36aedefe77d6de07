// Appearance features for re-identification: yh_embed_quantize (f32 rows -> unit int8 rows of
// length 127), yh_embed_similarity (a batched A . B^T in exact int32 on the int8 MFMA), and the
// quantise-and-scatter and gallery-update launches of yh_track_reid. The semantics are stated in include/yolo_hip.h;
// the host twins are in csrc/track_host.cpp and the shared arithmetic in csrc/track_host.h.
//
// quantise: one workgroup of QUANT_T threads per row, an element every QUANT_T in registers
// (dim <= YH_REID_MAX_DIM = 8 * QUANT_T); the maximum and the integer sum of squares are reduced
// over the workgroup. The maximum is taken on the bit patterns of |e| (they order like the
// values, and anything at or above the pattern of infinity is not finite). fp64 for the two
// scalings, as the host twin: built with -ffp-contract=off.
//
// similarity: one wave per 64 x 64 tile of out[b], four v_mfma_i32_32x32x32_i8 accumulators, the
// fragments of four K steps loaded a group ahead of their MFMAs. Both
// operands are K-contiguous, so lane l (r = l & 31, h = l >> 5) loads the 16 bytes k0 + 16 h ..
// of row r of its A tile and of its B tile straight from global memory: no LDS. Whatever order
// the instruction gives the 16 bytes of the two lane halves inside its K = 32, A and B get the
// same one, and an integer dot product does not depend on the order of its terms; the C/D map
// (column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h) is the 32x32 one of every dtype. Rows
// at or beyond ra / rb are loaded as zeros, never read, and nothing is stored outside out[b].
// Workgroups are dealt to the XCDs round robin and every XCD has its own L2, so the tiles of one
// batch row are mapped to workgroups of one XCD: its operands cross the fabric once.
//
// gallery: yh_track_reid's gallery update, a wave per slot behind the track kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "mfma_i8.h"
#include "track_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int QUANT_T = 256;
constexpr int QUANT_PER = YH_REID_MAX_DIM / QUANT_T;
static_assert(QUANT_PER * QUANT_T == YH_REID_MAX_DIM, "a thread holds dim / QUANT_T elements");

__device__ inline unsigned wave_max(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// One row by the whole workgroup: e (dim) f32, or NULL for "no feature" -> q (dim) int8.
// Returns whether q is non-zero (the same value in every thread). red: QUANT_T / 64 + 1 words
// of 8 bytes of LDS.
__device__ bool quantize_row(const float* __restrict__ e, int8_t* __restrict__ q, int dim, unsigned long long* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!e) {   // workgroup-uniform
        for (int i = tid; i < dim; i += QUANT_T) q[i] = 0;
        return false;
    }
    float v[QUANT_PER];
    unsigned mx = 0;
#pragma unroll
    for (int j = 0; j < QUANT_PER; ++j) {
        const int i = tid + j * QUANT_T;
        v[j] = i < dim ? e[i] : 0.0f;
        const unsigned a = __float_as_uint(v[j]) & 0x7FFFFFFFu;
        mx = a > mx ? a : mx;
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = 0;
    for (int w = 0; w < QUANT_T / 64; ++w) mx = (unsigned)red[w] > mx ? (unsigned)red[w] : mx;
    __syncthreads();
    if (mx == 0 || mx >= 0x7F800000u) {   // all zero, or an element that is not finite
        for (int i = tid; i < dim; i += QUANT_T) q[i] = 0;
        return false;
    }
    const double r = 16384.0 / (double)__uint_as_float(mx);
    int pv[QUANT_PER];
    long long S = 0;
#pragma unroll
    for (int j = 0; j < QUANT_PER; ++j) {
        pv[j] = (int)rint((double)v[j] * r);
        S += (long long)pv[j] * pv[j];
    }
    S = wave_sum(S);
    if (lane == 0) red[wave] = (unsigned long long)S;
    __syncthreads();
    S = 0;
    for (int w = 0; w < QUANT_T / 64; ++w) S += (long long)red[w];
    const double scale = yh_reid_scale(S);   // S >= 16384^2: the largest element
#pragma unroll
    for (int j = 0; j < QUANT_PER; ++j) {
        const int i = tid + j * QUANT_T;
        if (i < dim) q[i] = (int8_t)yh_reid_round(pv[j], scale);
    }
    // the largest element gives |q_i| = rint(127 * 16384 / sqrt(S)) >= rint(127 / sqrt(dim)) >= 3
    return true;
}

__global__ __launch_bounds__(QUANT_T) void quantize_kernel(const float* __restrict__ e, int rows, int dim,
                                                           const int* __restrict__ count, int8_t* __restrict__ q) {
    __shared__ unsigned long long red[QUANT_T / 64];
    const int r = blockIdx.x;
    int n = rows;
    if (count) {
        n = *count;
        n = n < 0 ? 0 : (n > rows ? rows : n);
    }
    quantize_row(r < n ? e + (size_t)r * dim : nullptr, q + (size_t)r * dim, dim, red);
}

// yh_track_reid's features: workgroup (r, b) quantises the feature of row r of batch row b into
// q (batch, max_det, dim) and writes its flags (bit 0: has a feature, bit 1: q is non-zero).
// embed NULL: no row has a feature, and only the flags are written (nothing reads q then).
__global__ __launch_bounds__(QUANT_T) void scatter_kernel(const float* __restrict__ embed, int capacity, int dim,
                                                          const int* __restrict__ counts,
                                                          const int* __restrict__ feat_counts,
                                                          const int* __restrict__ embed_total, int max_det,
                                                          int8_t* __restrict__ q, int* __restrict__ flags) {
    __shared__ unsigned long long red[QUANT_T / 64];
    __shared__ long long slot0;
    __shared__ int nrow;
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t job = (size_t)b * max_det + r;
    if (!embed) {
        if (tid == 0) flags[job] = 0;
        return;
    }
    if (tid < 64) {   // n_0 + ... + n_(b-1), and n_b
        long long sum = 0;
        int mine = 0;
        for (int i = tid; i <= b; i += 64) {
            int c = counts[i];
            c = c < 0 ? 0 : (c > max_det ? max_det : c);
            int n = c;
            if (feat_counts) {
                n = feat_counts[i];
                n = n < 0 ? 0 : (n > c ? c : n);
            }
            if (i < b) sum += n;
            else mine = n;
        }
        sum = wave_sum(sum);
        mine = (int)wave_sum(mine);
        if (tid == 0) {
            slot0 = sum;
            nrow = mine;
        }
    }
    __syncthreads();
    long long limit = capacity;
    if (embed_total) {
        const long long t = *embed_total;
        limit = t < limit ? t : limit;
    }
    const long long s = slot0 + r;
    const bool has = r < nrow && s < limit;   // workgroup-uniform
    const bool nz = quantize_row(has ? embed + (size_t)s * dim : nullptr, q + job * dim, dim, red);
    if (tid == 0) flags[job] = has ? (nz ? 3 : 1) : 0;
}

// the lane's 16 results of a 32 x 32 tile at (m0, n0) of out (ra, rb)
__device__ __forceinline__ void store_tile(int32_t* __restrict__ out, const i32x16& c, int m0, int n0, int ra, int rb,
                                           int r, int h) {
    const int n = n0 + r;
    if (n >= rb) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int m = m0 + tile_row(reg, h);
        if (m < ra) out[(size_t)m * rb + n] = c[reg];
    }
}

constexpr int SIM_KU = 4;   // K steps of 32 loaded together: 16 loads of 16 bytes in flight per lane

// a_nonzero: NULL, or (batch, ra) int32 that receives "row m of the A block has a non-zero byte"
// (yh_track_reid's "the gallery row holds a feature"), written by the tiles of the first column.
// the same tile into the transposed matrix out_t (rb, ra)
__device__ __forceinline__ void store_tile_t(int32_t* __restrict__ out_t, const i32x16& c, int m0, int n0, int ra, int rb,
                                             int r, int h) {
    typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));
    const int n = n0 + r;
    if (n >= rb) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3 are the rows m .. m + 3
        const int m = m0 + tile_row(4 * g, h);
        int32_t* o = out_t + (size_t)n * ra + m;
        if (m + 3 < ra) {
            *reinterpret_cast<i32x4u*>(o) = i32x4u{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (m + i < ra) o[i] = c[4 * g + i];
        }
    }
}

__global__ __launch_bounds__(64) void similarity_kernel(const int8_t* __restrict__ a, size_t a_block_stride, int nblocks,
                                                        const int* __restrict__ a_index, int b_base,
                                                        const int8_t* __restrict__ b, int ra, int rb, int dim,
                                                        int32_t* __restrict__ out, int* __restrict__ a_nonzero,
                                                        int32_t* __restrict__ out_t, int batch, int tiles_n,
                                                        int tiles) {
    // Workgroups go to the XCDs round robin, and each XCD has an L2 of its own: the tiles of one
    // batch row, which share its A block and its B rows, are given to workgroups of one XCD
    // (batch row = 8 * group + XCD), so each operand crosses the fabric to one L2 only.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bz = (slot / tiles) * 8 + xcd;
    if (bz >= batch) return;
    const int tile = slot % tiles;
    const int m0 = (tile / tiles_n) * 64, n0 = (tile % tiles_n) * 64;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int k = a_index ? a_index[bz] : b_base + bz;   // b_base: the launch's first batch row
    const bool block_ok = k >= 0 && k < nblocks;
    const int8_t* ablk = a + (block_ok ? (size_t)k * a_block_stride : 0);
    const int8_t* bblk = b + (size_t)bz * rb * dim;
    const bool aok0 = block_ok && m0 + r < ra, aok1 = block_ok && m0 + 32 + r < ra;
    const bool bok0 = n0 + r < rb, bok1 = n0 + 32 + r < rb;
    const int8_t* ap0 = ablk + (size_t)(m0 + r) * dim + 16 * h;
    const int8_t* ap1 = ap0 + (size_t)32 * dim;
    const int8_t* bp0 = bblk + (size_t)(n0 + r) * dim + 16 * h;
    const int8_t* bp1 = bp0 + (size_t)32 * dim;
    // the fragments of SIM_KU steps are loaded a group ahead of the MFMAs that use them; a step at
    // or beyond dim loads zeros (dim is a multiple of 64, not of 32 SIM_KU) and adds nothing
    struct Frags {
        i32x4 a0[SIM_KU], a1[SIM_KU], b0[SIM_KU], b1[SIM_KU];
    };
    auto load = [&](Frags& f, int k0) {
#pragma unroll
        for (int u = 0; u < SIM_KU; ++u) {
            const int kk = k0 + 32 * u;
            const bool in = kk < dim;
            f.a0[u] = load16(ap0 + kk, aok0 && in);
            f.a1[u] = load16(ap1 + kk, aok1 && in);
            f.b0[u] = load16(bp0 + kk, bok0 && in);
            f.b1[u] = load16(bp1 + kk, bok1 && in);
        }
    };
    i32x16 c00 = {}, c01 = {}, c10 = {}, c11 = {};
    i32x4 or0 = {}, or1 = {};
    Frags cur;
    load(cur, 0);
    for (int k0 = 0; k0 < dim; k0 += 32 * SIM_KU) {
        Frags nxt;
        load(nxt, k0 + 32 * SIM_KU);
#pragma unroll
        for (int u = 0; u < SIM_KU; ++u) {
            or0 |= cur.a0[u];
            or1 |= cur.a1[u];
            c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a0[u], cur.b0[u], c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a0[u], cur.b1[u], c01, 0, 0, 0);
            c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a1[u], cur.b0[u], c10, 0, 0, 0);
            c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a1[u], cur.b1[u], c11, 0, 0, 0);
        }
        cur = nxt;
    }
    int32_t* o = out + (size_t)bz * ra * rb;
    store_tile(o, c00, m0, n0, ra, rb, r, h);
    store_tile(o, c01, m0, n0 + 32, ra, rb, r, h);
    store_tile(o, c10, m0 + 32, n0, ra, rb, r, h);
    store_tile(o, c11, m0 + 32, n0 + 32, ra, rb, r, h);
    if (out_t) {   // the transpose as well (yh_track_reid scans it by row): four consecutive m per store
        int32_t* ot = out_t + (size_t)bz * ra * rb;
        store_tile_t(ot, c00, m0, n0, ra, rb, r, h);
        store_tile_t(ot, c01, m0, n0 + 32, ra, rb, r, h);
        store_tile_t(ot, c10, m0 + 32, n0, ra, rb, r, h);
        store_tile_t(ot, c11, m0 + 32, n0 + 32, ra, rb, r, h);
    }
    if (a_nonzero && n0 == 0) {   // the two lane halves hold the two halves of every K step of a row
        int z0 = or0[0] | or0[1] | or0[2] | or0[3], z1 = or1[0] | or1[1] | or1[2] | or1[3];
        z0 |= __shfl_xor(z0, 32);
        z1 |= __shfl_xor(z1, 32);
        if (h == 0) {
            if (m0 + r < ra) a_nonzero[(size_t)bz * ra + m0 + r] = z0 != 0;
            if (m0 + 32 + r < ra) a_nonzero[(size_t)bz * ra + m0 + 32 + r] = z1 != 0;
        }
    }
}

// yh_track_reid's gallery update, behind the track kernel: one wave per slot, a lane per word of
// four elements. code (batch, T): the slot's row of this frame, bit 30 set for a slot born in it,
// negative for "nothing to do" (the track kernel writes it; a batch row without a stream has none).
__global__ __launch_bounds__(64) void gallery_kernel(char* __restrict__ state, size_t stream_bytes, size_t gallery_offset,
                                                     const int* __restrict__ stream_ids, int T, int D, int dim,
                                                     const int8_t* __restrict__ q, const int* __restrict__ flags,
                                                     const int* __restrict__ code) {
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int c = code[(size_t)b * T + t];
    if (c < 0) return;
    const int d = c & ~(1 << 30);
    const bool born = (c >> 30) != 0;
    const int s = stream_ids ? stream_ids[b] : b;
    const int gw = dim >> 2;
    uint32_t* g = reinterpret_cast<uint32_t*>(state + (size_t)s * stream_bytes + gallery_offset) + (size_t)t * gw;
    constexpr int PER = YH_REID_MAX_DIM / 4 / 64;   // words per lane
    if (!(flags[(size_t)b * D + d] & 1)) {          // no feature: only a birth clears its row
        if (born)
            for (int j = lane; j < gw; j += 64) g[j] = 0;
        return;
    }
    const uint32_t* qr = reinterpret_cast<const uint32_t*>(q + ((size_t)b * D + d) * dim);
    uint32_t gv[PER], qv[PER];
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int j = lane + 64 * i;
        gv[i] = j < gw ? g[j] : 0;
        qv[i] = j < gw ? qr[j] : 0;
        any |= gv[i];
    }
    if (born || !__any(any != 0)) {                 // a new track, or no feature so far: take the row's
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (lane + 64 * i < gw) g[lane + 64 * i] = qv[i];
        return;
    }
    long long S = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 7 * (int)(int8_t)(gv[i] >> (8 * e)) + (int)(int8_t)(qv[i] >> (8 * e));
            S += (long long)v * v;
        }
    S = wave_sum(S);
    const double scale = S ? yh_reid_scale(S) : 0.0;   // S == 0: every element is 0
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        uint32_t o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 7 * (int)(int8_t)(gv[i] >> (8 * e)) + (int)(int8_t)(qv[i] >> (8 * e));
            o |= (uint32_t)(uint8_t)(int8_t)yh_reid_round(v, scale) << (8 * e);
        }
        if (lane + 64 * i < gw) g[lane + 64 * i] = o;
    }
}

}  // namespace

int launch_embed_quantize(const float* e, int rows, int dim, const int* count, int8_t* q, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(quantize_kernel, dim3(rows), dim3(QUANT_T), 0, s, e, rows, dim, count, q);
    return (int)hipGetLastError();
}

int launch_embed_scatter(const float* embed, int capacity, int dim, const int* counts, const int* feat_counts,
                         const int* embed_total, int batch, int max_det, int8_t* q, int* flags, hipStream_t s) {
    if (batch <= 0 || max_det <= 0) return 0;
    hipLaunchKernelGGL(scatter_kernel, dim3(max_det, batch), dim3(QUANT_T), 0, s, embed, capacity, dim, counts,
                       feat_counts, embed_total, max_det, q, flags);
    return (int)hipGetLastError();
}

int launch_gallery_update(void* state, size_t stream_bytes, size_t gallery_offset, const int* stream_ids, int batch,
                          int max_tracks, int max_det, int dim, const int8_t* q, const int* flags, const int* code,
                          hipStream_t s) {
    if (batch <= 0) return 0;
    hipLaunchKernelGGL(gallery_kernel, dim3(max_tracks, batch), dim3(64), 0, s, static_cast<char*>(state), stream_bytes,
                       gallery_offset, stream_ids, max_tracks, max_det, dim, q, flags, code);
    return (int)hipGetLastError();
}

int launch_embed_similarity(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                            int batch, int ra, int rb, int dim, int32_t* out, int* a_nonzero, int32_t* out_t,
                            hipStream_t s) {
    if (batch <= 0 || ra <= 0 || rb <= 0) return 0;
    const int tiles_n = (rb + 63) / 64;
    const long long tiles_ll = (long long)tiles_n * ((ra + 63) / 64);
    if (tiles_ll > (1ll << 27)) return (int)hipErrorInvalidValue;   // an output of more than 2^39 elements
    const int tiles = (int)tiles_ll;
    // batch rows per launch: a multiple of 8 that keeps the grid at or below 2^30 workgroups
    long long fit = ((1ll << 30) / tiles) & ~7ll;
    const int step = (int)(fit < 8 ? 8 : (fit > 65536 ? 65536 : fit));
    for (int b0 = 0; b0 < batch; b0 += step) {
        const int nb = batch - b0 < step ? batch - b0 : step;
        const unsigned grid = (unsigned)((nb + 7) / 8) * 8u * (unsigned)tiles;
        hipLaunchKernelGGL(similarity_kernel, dim3(grid), dim3(64), 0, s, a, a_block_stride, nblocks,
                           a_index ? a_index + b0 : nullptr, b0, b + (size_t)b0 * rb * dim, ra, rb, dim,
                           out + (size_t)b0 * ra * rb, a_nonzero ? a_nonzero + (size_t)b0 * ra : nullptr,
                           out_t ? out_t + (size_t)b0 * ra * rb : nullptr, nb, tiles_n, tiles);
        if (hipError_t err = hipGetLastError()) return (int)err;
    }
    return 0;
}

}  // namespace yh
