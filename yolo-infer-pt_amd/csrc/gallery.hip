// Identity search over a gallery of unit int8 features: yh_gallery_search (the k best rows per
// query, the exact int32 products on v_mfma_i32_32x32x32_i8, the (nq, n) score matrix never
// written) and yh_gallery_enrol (append rows without a read-back). The semantics are stated in
// include/yolo_hip.h; the host twins are in csrc/gallery_host.cpp, and the order of two
// candidates, the chunking and the workspace layout in csrc/gallery_host.h.
//
// search: a workgroup of NW waves owns one chunk of gallery rows and one tile of 64 queries. The
// query tile sits in LDS (rows padded by 16 bytes: the 16 lanes of a ds_read_b128 group then fall
// on 16 different bank quads). Each wave streams 64 gallery rows per step with mfma_i8.h's
// K-contiguous 16-byte loads straight from global memory (A = gallery, B = queries: lane (r, h)
// holds query r or 32 + r against 16 gallery rows per accumulator, four accumulators), the
// fragments of four K steps loaded a group ahead of their MFMAs, across the steps too. Each
// (wave, query) keeps its k best so far in LDS as gallery_host.h's 64-bit keys, in no order, and
// each lane the score of its queries' k-th key in a register, raised to the largest such score
// of the workgroup's waves: a step whose 64 scores all lie below it costs 64 compares. Otherwise
// the wave offers the scores that pass to the lists (a key that beats a list's smallest takes
// its place, found in one pass over the list), the lane half h = 0 first and then h = 1, since
// the two halves hold the same queries. Rows at or beyond n are loaded as zeros and never
// offered, nor are rows with a negative label: a step reads its 64 labels once, a lane each, and
// a ballot makes them a mask. At the end the workgroup merges its waves' lists per query and
// writes k keys per query, descending, to the workspace; a second kernel, a wave per query,
// merges the chunks. Workgroups go to the XCDs round robin, and the query tiles of one chunk are
// given to workgroups of one XCD (chunk = 8 * group + XCD), so a gallery row crosses the fabric
// once.
//
// enrol: one workgroup. Per block of ENROL_T query rows: a wave per row finds whether it is
// non-zero, a workgroup prefix sum over the flags gives every enrolled row its gallery row and
// its label, then a wave per row copies.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "gallery_host.h"
#include "mfma_i8.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int GAL_KU = 4;          // K steps of 32 loaded together
constexpr int GAL_QT = 64;         // queries of a tile
constexpr int GAL_PAD = 16;        // bytes behind a query row in LDS
constexpr int GAL_MAX_WAVES = 8;
constexpr int GAL_LDS_MAX = 160 * 1024;

__host__ __device__ inline int gal_tile_bytes(int dim) { return GAL_QT * (dim + GAL_PAD); }
// the tile, the lists of the waves, a key per wave and query for their merge, the queries' flags
// and the queries' shared thresholds
inline int gal_lds_bytes(int dim, int k, int waves) {
    return gal_tile_bytes(dim) + waves * GAL_QT * k * 8 + waves * GAL_QT * 8 + 2 * GAL_QT * 4;
}

// The 16 scores of one accumulator against the list L of their query (k keys in no order, 0 for a
// free place), gallery rows base + tile_row(reg, h). A key that beats the list's smallest takes its
// place: one pass over the list finds the smallest, its place and the second smallest, which says
// what the smallest is afterwards. ts: the score below which nothing enters, kept up to date.
// valid: bit b says that gallery row row0 + b exists and is a candidate; off: 0 or 32, the
// accumulator's first row. The scores that pass are marked first, then taken one by one, so the
// pass over the list exists once per accumulator and not once per register.
__device__ __forceinline__ void gal_offer(const i32x16& c, unsigned long long* L, int k, int& ts, int row0, int off, int h,
                                          unsigned long long valid) {
    unsigned pass = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
        pass |= (unsigned)(c[reg] >= ts && ((valid >> (off + tile_row(reg, h))) & 1)) << reg;
    while (pass) {
        const int reg = __builtin_ctz(pass);
        pass &= pass - 1;
        int s = c[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) s = reg == i ? c[i] : s;
        if (s < ts) continue;   // the list has moved on meanwhile
        const unsigned long long key = yh_gal_key(s, row0 + off + tile_row(reg, h));
        unsigned long long lo = ~0ull, lo2 = ~0ull;
        int at = 0;
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const unsigned long long v = L[j];
            if (v < lo) {
                lo2 = lo;
                lo = v;
                at = j;
            } else if (v < lo2) {
                lo2 = v;
            }
        }
        if (key > lo) {
            L[at] = key;
            lo = key < lo2 ? key : lo2;
        }
        const int t = yh_gal_key_score(lo);
        ts = t > ts ? t : ts;
    }
}

__device__ __forceinline__ bool gal_any_at_least(const i32x16& c, int ts) {
    bool hit = false;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) hit |= c[reg] >= ts;
    return hit;
}

__global__ __launch_bounds__(64 * GAL_MAX_WAVES) void gallery_search_kernel(
    const int8_t* __restrict__ gallery, const int* __restrict__ labels, const int* __restrict__ size, int capacity,
    int dim, const int8_t* __restrict__ q, int nq, const int* __restrict__ nq_count, int k, int chunk_rows, int chunks,
    int qtiles, unsigned long long* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int chunk = (slot / qtiles) * 8 + xcd;
    if (chunk >= chunks) return;
    const int n = yh_gal_clamp(size, capacity);
    const long long c0 = (long long)chunk * chunk_rows;
    if (c0 >= n) return;   // the merge reads the chunks below n only
    const int row_lo = (int)c0;
    const int n_end = c0 + chunk_rows < n ? (int)(c0 + chunk_rows) : n;
    const int q0 = (slot % qtiles) * GAL_QT;
    const int m = yh_gal_clamp(nq_count, nq);
    const int tid = threadIdx.x, nthreads = blockDim.x, waves = nthreads >> 6;
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int ldq = dim + GAL_PAD;
    int8_t* tile = reinterpret_cast<int8_t*>(lds);
    unsigned long long* lists = reinterpret_cast<unsigned long long*>(lds + gal_tile_bytes(dim));
    unsigned long long* cand = lists + (size_t)waves * GAL_QT * k;
    int* qok = reinterpret_cast<int*>(cand + (size_t)waves * GAL_QT);
    volatile int* thr = qok + GAL_QT;

    // the query tile; a row at or beyond m is zeros and is never read
    const int cpr = dim >> 4;   // 16-byte pieces per row
    for (int i = tid; i < GAL_QT * cpr; i += nthreads) {
        const int row = i / cpr, piece = i - row * cpr;
        const i32x4 v = load16(q + (size_t)(q0 + row) * dim + 16 * piece, q0 + row < m);
        *reinterpret_cast<i32x4*>(tile + row * ldq + 16 * piece) = v;
    }
    for (int i = tid; i < waves * GAL_QT * k; i += nthreads) lists[i] = 0;
    __syncthreads();
    if (tid < GAL_QT) {   // "no feature": a query whose bytes are all zero has no candidates
        i32x4 any = {0, 0, 0, 0};
        for (int piece = 0; piece < cpr; ++piece) any |= *reinterpret_cast<const i32x4*>(tile + tid * ldq + 16 * piece);
        qok[tid] = (any[0] | any[1] | any[2] | any[3]) != 0;
        thr[tid] = INT32_MIN;
    }
    __syncthreads();

    unsigned long long* L0 = lists + ((size_t)wave * GAL_QT + r) * k;
    unsigned long long* L1 = L0 + (size_t)32 * k;
    const bool ok0 = qok[r] != 0, ok1 = qok[32 + r] != 0;
    // The score below which nothing enters the query's list; a query without candidates never
    // passes. Once a wave's list is full, its smallest score bounds the workgroup's k best from
    // below, so the waves share the largest such score per query through thr: plain loads and
    // stores, where a lost or a late store only leaves a smaller, still valid bound.
    int ts0 = ok0 ? INT32_MIN : INT32_MAX, ts1 = ok1 ? INT32_MIN : INT32_MAX;

    const int8_t* bp0 = tile + r * ldq + 16 * h;
    const int8_t* bp1 = bp0 + 32 * ldq;
    struct Frags {
        i32x4 a0[GAL_KU], a1[GAL_KU];
    };
    // the gallery fragments of GAL_KU steps from k0 of the 64 rows at row0; a row at or beyond n_end
    // and a step at or beyond dim (dim is a multiple of 64, not of 32 GAL_KU) load zeros
    auto load = [&](Frags& f, int row0, int k0) {
        const bool in0 = row0 + r < n_end, in1 = row0 + 32 + r < n_end;
        const int8_t* ap0 = gallery + (size_t)(row0 + r) * dim + 16 * h;
        const int8_t* ap1 = ap0 + (size_t)32 * dim;
#pragma unroll
        for (int u = 0; u < GAL_KU; ++u) {
            const int kk = k0 + 32 * u;
            const bool in = kk < dim;
            f.a0[u] = load16(ap0 + kk, in0 && in);
            f.a1[u] = load16(ap1 + kk, in1 && in);
        }
    };
    const int stride = 64 * waves;
    int row0 = row_lo + 64 * wave;
    Frags cur;
    load(cur, row0, 0);
    // row0 stays below 2^31: n_end - row_lo <= chunk_rows and the loop ends at the first row0 >= n_end
    while (row0 < n_end) {
        i32x16 c00 = {}, c01 = {}, c10 = {}, c11 = {};
        // lane l: is row row0 + l a candidate? One load per step, long before its use: a label read
        // per score that passes would put a memory latency into every offer
        const bool live = row0 + lane < n_end && (!labels || labels[row0 + lane] >= 0);
        for (int k0 = 0; k0 < dim; k0 += 32 * GAL_KU) {
            int nk = k0 + 32 * GAL_KU, nrow = row0;
            if (nk >= dim) {
                nk = 0;
                nrow = n_end - row0 > stride ? row0 + stride : n_end;   // n_end: nothing to load
            }
            Frags nxt;
            load(nxt, nrow, nk);
#pragma unroll
            for (int u = 0; u < GAL_KU; ++u) {
                const int kk = k0 + 32 * u;
                if (kk < dim) {   // wave-uniform
                    const i32x4 b0 = *reinterpret_cast<const i32x4*>(bp0 + kk);
                    const i32x4 b1 = *reinterpret_cast<const i32x4*>(bp1 + kk);
                    c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a0[u], b0, c00, 0, 0, 0);
                    c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a0[u], b1, c01, 0, 0, 0);
                    c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a1[u], b0, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a1[u], b1, c11, 0, 0, 0);
                }
            }
            cur = nxt;
        }
        if (ok0) ts0 = max(ts0, thr[r]);
        if (ok1) ts1 = max(ts1, thr[32 + r]);
        const bool hit = gal_any_at_least(c00, ts0) | gal_any_at_least(c10, ts0) | gal_any_at_least(c01, ts1) |
                         gal_any_at_least(c11, ts1);
        if (__any(hit)) {
            const unsigned long long valid = __ballot(live);
            // the two lane halves hold the same queries: one after the other (a wave runs in step,
            // and LDS serves one wave's accesses in order)
#pragma nounroll
            for (int hh = 0; hh < 2; ++hh) {
                if (h == hh) {
                    gal_offer(c00, L0, k, ts0, row0, 0, h, valid);
                    gal_offer(c10, L0, k, ts0, row0, 32, h, valid);
                    gal_offer(c01, L1, k, ts1, row0, 0, h, valid);
                    gal_offer(c11, L1, k, ts1, row0, 32, h, valid);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (ok0 && ts0 > thr[r]) thr[r] = ts0;
            if (ok1 && ts1 > thr[32 + r]) thr[32 + r] = ts1;
        }
        row0 = n_end - row0 > stride ? row0 + stride : n_end;
    }
    __syncthreads();

    // The waves' lists of a query into the chunk's k best, descending: thread (wave, lane) owns the
    // list of wave `wave` for query `lane`; in round j each offers its largest key below the last one
    // taken and the largest offer is taken. Keys are distinct, and 0 ("no candidate") ends a list.
    const unsigned long long* mine = lists + ((size_t)wave * GAL_QT + lane) * k;
    unsigned long long* o = ws + ((size_t)chunk * nq + q0 + lane) * k;
    unsigned long long prev = ~0ull;
    for (int j = 0; j < k; ++j) {   // workgroup-uniform
        unsigned long long best = 0;
#pragma unroll 4
        for (int e = 0; e < k; ++e) {
            const unsigned long long v = mine[e];
            best = v < prev && v > best ? v : best;
        }
        cand[wave * GAL_QT + lane] = best;
        __syncthreads();
        unsigned long long top = 0;
        for (int w = 0; w < waves; ++w) {
            const unsigned long long v = cand[w * GAL_QT + lane];
            top = v > top ? v : top;
        }
        if (wave == 0 && q0 + lane < nq) o[j] = top;
        prev = top;
        __syncthreads();
    }
}

__device__ inline unsigned long long wave_max64(unsigned long long v) {
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// One wave per query: the lists of the chunks below n -> scores and index. Lane l gathers the k
// best of the chunks l, l + 64, ... in LDS (entry j of lane l at [j][l]), then k rounds take the
// largest head of the 64 lists. Keys are distinct (a row is in one chunk), 0 is "no candidate".
__global__ __launch_bounds__(64) void gallery_merge_kernel(const unsigned long long* __restrict__ ws,
                                                           const int* __restrict__ size, int capacity, int nq, int k,
                                                           int chunk_rows, int32_t* __restrict__ scores,
                                                           int32_t* __restrict__ index) {
    __shared__ unsigned long long best[YH_GALLERY_MAX_K * 64];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int n = yh_gal_clamp(size, capacity);
    const int live = (int)(((long long)n + chunk_rows - 1) / chunk_rows);
    for (int j = 0; j < k; ++j) best[j * 64 + lane] = 0;
    for (int c = lane; c < live; c += 64) {
        const unsigned long long* in = ws + ((size_t)c * nq + i) * k;
        // no early exit at the first key that does not enter: the loads then do not wait for one another
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const unsigned long long key = in[j];
            if (key <= best[(k - 1) * 64 + lane]) continue;
            int t = k - 1;
            for (; t > 0 && best[(t - 1) * 64 + lane] < key; --t) best[t * 64 + lane] = best[(t - 1) * 64 + lane];
            best[t * 64 + lane] = key;
        }
    }
    int head = 0;
    for (int j = 0; j < k; ++j) {
        const unsigned long long mine = head < k ? best[head * 64 + lane] : 0;
        const unsigned long long top = wave_max64(mine);
        if (top != 0 && mine == top) ++head;
        if (lane == 0) {
            scores[(size_t)i * k + j] = yh_gal_key_score(top);
            index[(size_t)i * k + j] = yh_gal_key_row(top);
        }
    }
}

constexpr int ENROL_T = 256;

__global__ __launch_bounds__(ENROL_T) void gallery_enrol_kernel(int8_t* __restrict__ gallery, int* __restrict__ labels,
                                                                int* __restrict__ size, int capacity, int dim,
                                                                const int8_t* __restrict__ q, int nq,
                                                                const int* __restrict__ nq_count,
                                                                const int* __restrict__ take,
                                                                const int* __restrict__ labels_in,
                                                                int* __restrict__ next_label, int* __restrict__ rows_out) {
    __shared__ int flag[ENROL_T];   // the row is to be enrolled, then its gallery row or -1
    __shared__ int wsum[ENROL_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = yh_gal_clamp(nq_count, nq);
    const int n0 = yh_gal_clamp(size, capacity);
    const int next0 = labels_in ? 0 : *next_label;
    const int cpr = dim >> 4;
    int done = 0;   // rows flagged in the blocks before this one (nq <= 2^31 - 1)
    for (int i0 = 0; i0 < nq; i0 += ENROL_T) {
        for (int j = wave; j < ENROL_T; j += ENROL_T / 64) {
            const int i = i0 + j;
            bool nz = false;
            if (i < m && (!take || take[i] != 0)) {   // wave-uniform
                i32x4 any = {0, 0, 0, 0};
                for (int piece = lane; piece < cpr; piece += 64) any |= load16(q + (size_t)i * dim + 16 * piece, true);
                nz = __any((any[0] | any[1] | any[2] | any[3]) != 0);
            }
            if (lane == 0) flag[j] = nz;
        }
        __syncthreads();
        // the exclusive prefix sum of the flags over the workgroup
        const int f = flag[tid];
        int incl = f;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = done, total = 0;
        for (int w = 0; w < ENROL_T / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        const int ord = before + incl - f;                 // flagged rows before this one
        const bool fits = ord < capacity - n0;             // the gallery is not full
        const int row = f && fits ? n0 + ord : -1;
        if (i0 + tid < nq) rows_out[i0 + tid] = row;
        if (row >= 0) labels[row] = labels_in ? labels_in[i0 + tid] : next0 + ord;
        __syncthreads();
        flag[tid] = row;
        __syncthreads();
        for (int j = wave; j < ENROL_T; j += ENROL_T / 64) {
            const int dst = flag[j];
            if (dst < 0) continue;   // wave-uniform
            const int8_t* src = q + (size_t)(i0 + j) * dim;
            for (int piece = lane; piece < cpr; piece += 64)
                *reinterpret_cast<i32x4*>(gallery + (size_t)dst * dim + 16 * piece) = load16(src + 16 * piece, true);
        }
        __syncthreads();
        done += total;
    }
    if (tid == 0) {
        const int room = capacity - n0;
        const int added = done < room ? done : room;
        *size = n0 + added;
        if (!labels_in) *next_label = next0 + added;
    }
}

}  // namespace

int launch_gallery_search(const int8_t* gallery, const int* labels, const int* size, int capacity, int dim,
                          const int8_t* q, int nq, const int* nq_count, int k, int chunk_rows, int32_t* scores,
                          int32_t* index, void* workspace, hipStream_t s) {
    if (nq <= 0) return 0;
    const int rows = yh_gal_chunk_rows(capacity, nq, chunk_rows);
    const int chunks = (int)yh_gal_chunks(capacity, nq, chunk_rows);
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    if (chunks > 0) {
        int waves = GAL_MAX_WAVES;
        while (waves > 1 && (gal_lds_bytes(dim, k, waves) > GAL_LDS_MAX || 64 * (waves / 2) >= rows)) waves >>= 1;
        const int lds = gal_lds_bytes(dim, k, waves);
        if (int rc = lds_optin(reinterpret_cast<const void*>(gallery_search_kernel), GAL_LDS_MAX)) return rc;
        const int qtiles = (nq + GAL_QT - 1) / GAL_QT;
        const unsigned grid = (unsigned)((chunks + 7) / 8) * 8u * (unsigned)qtiles;
        hipLaunchKernelGGL(gallery_search_kernel, dim3(grid), dim3(64 * waves), lds, s, gallery, labels, size, capacity,
                           dim, q, nq, nq_count, k, rows, chunks, qtiles, ws);
        if (hipError_t err = hipGetLastError()) return (int)err;
    }
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(nq), dim3(64), 0, s, ws, size, capacity, nq, k, rows, scores, index);
    return (int)hipGetLastError();
}

int launch_gallery_enrol(int8_t* gallery, int* labels, int* size, int capacity, int dim, const int8_t* q, int nq,
                         const int* nq_count, const int* take, const int* labels_in, int* next_label, int* rows_out,
                         hipStream_t s) {
    hipLaunchKernelGGL(gallery_enrol_kernel, dim3(1), dim3(ENROL_T), 0, s, gallery, labels, size, capacity, dim, q, nq,
                       nq_count, take, labels_in, next_label, rows_out);
    return (int)hipGetLastError();
}

}  // namespace yh
