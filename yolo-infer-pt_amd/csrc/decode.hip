// Detect-head decode: DFL + anchors + dist2bbox + sigmoid (nets/nn.py:255-270, 222-225;
// utils/util.py:85-96) into the caller's (B, 4 + nc, A).
//   head_decode      any dtype and class count, per-anchor loads from the head tensors
//   head_decode_lds  16-bit, 80 classes: the head tile staged through LDS
//   set_io           publishes the caller's x / y pointers for graph replay (read through io_global)
// The value arithmetic is head_math.h's, shared with head.hip's box_dfl and head_cls.
#include "common.h"
#include "dtypes.h"
#include "head_math.h"

namespace yh {

namespace {

constexpr int DEC_A = 256;   // anchors per workgroup, one per thread

// Rows r0 .. r0 + rows - 1 of the workgroup's LDS tile [4 + nc][DEC_A] (anchors a0 ..) into the
// image's channel-major output as 16-B (fp32: 32-B) chunks of 8 anchors (A % 8 == 0, a0 % 8 == 0).
// (p.A is read from the arguments at each use: by value it cost head_decode<T, true> an SGPR.)
template <typename T>
__device__ __forceinline__ void tile_rows_out(const T* tile, gptr<T> yimg, int r0, int rows, int a0, const DecodeArgs& p) {
    for (int c = threadIdx.x; c < rows * (DEC_A / 8); c += 256) {
        const int r = r0 + (c >> 5), k = c & 31;   // DEC_A / 8 = 32 chunks per row
        const int a8 = a0 + 8 * k;
        if (a8 >= p.A) continue;
        const T* srow = tile + r * DEC_A + 8 * k;
        const gptr<T> drow = yimg + (long long)r * p.A + a8;
        if (a8 + 8 <= p.A) st_chunk(drow, ld_chunk(srow));
        else for (int e = 0; a8 + e < p.A; ++e) drow[e] = srow[e];
    }
}

// One workgroup = 256 consecutive anchors of one image. Each thread decodes its
// anchor into a column of an LDS tile [4 + nc][256]; the tile then leaves as
// 16-B (fp32: 32-B) row chunks of the channel-major output instead of 4 + nc
// scalar stores per thread. Needs A % 8 == 0 (aligned row chunks); otherwise
// every value is stored directly (ROWS = false).
template <typename T, bool ROWS>
__global__ __launch_bounds__(256) void head_decode(const DecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    T* tile = reinterpret_cast<T*>(dsm);              // [(4 + nc)][256]
    const int n = blockIdx.y, a0 = p.a_lo + blockIdx.x * DEC_A;
    const int a = a0 + threadIdx.x;
    const bool live = a < p.A;
    const gptr<T> yimg = io_global<T>(p.io[1]) + (long long)n * (4 + p.nc) * p.A;
    auto put = [&](int r, float v) {
        if constexpr (ROWS) tile[r * DEC_A + threadIdx.x] = fromf<T>(v);
        else if (live) yimg[(long long)r * p.A + a] = fromf<T>(v);
    };
    {
        const int aa = live ? a : p.A - 1;   // dead lanes decode a valid anchor that is never stored
        const auto [l, loc] = anchor_level(p.H[0] * p.W[0], p.H[1] * p.W[1], aa);
        const int H = p.H[l], W = p.W[l];
        const int gy = loc / W, gx = loc - gy * W;
        const T* src = reinterpret_cast<const T*>(p.lvl[l]) + ((long long)n * H * W + loc) * p.ldc;
        float dist[4];
#pragma unroll
        for (int sd = 0; sd < 4; ++sd) {
            float v[16];
#pragma unroll
            for (int c = 0; c < 16; c += 8) chunk_to_f(ld_chunk(src + sd * 16 + c), reinterpret_cast<float(&)[8]>(v[c]));
            dist[sd] = dfl16<T>(v);
        }
        const float st = p.stride[l];
        if (p.box) {
            float b[4];
            dist2bbox(gx, gy, st, dist, b);
            put(0, b[0]), put(1, b[1]), put(2, b[2]), put(3, b[3]);
        }
        // class scores: all chunks of a batch of DEC_CB loaded before any is used (a
        // load inside the runtime-bound loop would be waited for one round trip at a time)
        constexpr int DEC_CB = 10;
        const T* cls = src + 64;
        const int ncc = (p.nc + 7) / 8;
        for (int c0 = 0; c0 < ncc; c0 += DEC_CB) {
            Chunk<T> v[DEC_CB];
#pragma unroll
            for (int u = 0; u < DEC_CB; ++u) v[u] = ld_chunk(cls + 8 * min(c0 + u, ncc - 1));
#pragma unroll
            for (int u = 0; u < DEC_CB; ++u) {
                const int c = 8 * (c0 + u);
                if (c >= p.nc) break;
                float f[8];
                chunk_to_f(v[u], f);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c + e < p.nc) put(4 + c + e, sigmoid<T>(f[e]));
            }
        }
    }
    if constexpr (ROWS) {
        __syncthreads();
        const int r0 = p.box ? 0 : 4;
        tile_rows_out<T>(tile, yimg, r0, 4 + p.nc - r0, a0, p);
    }
}

// 16-bit decode with the head tile staged through LDS. The head tensor's pixels are
// ldc channels apart (box 64 | cls nc | padding), so per-anchor 16-B chunk loads
// touch a new 128-B line per lane and every load instruction gathers 64 lines;
// here the workgroup first copies its 256 anchors' box+cls chunks (CH per anchor)
// as lane-consecutive 16-B pieces (each wave instruction reads whole lines), then
// each thread decodes its anchor from LDS into registers, and the (4 + nc) x 256
// output tile, written over the input tile, leaves as 512-B row runs.
// BOX = false: class rows only (the box rows come from box_dfl), anchors [a_lo, A).
template <typename T, int NCC, bool BOX>   // NCC = nc / 8 class chunks
__global__ __launch_bounds__(256, 2) void head_decode_lds(const DecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint4 dsm4[];
    constexpr int CB = BOX ? 8 : 0;              // box chunks per anchor
    constexpr int CH = CB + NCC, CHP = CH + 1;   // chunks per anchor, padded LDS row
    const int n = blockIdx.y, a0 = p.a_lo + blockIdx.x * DEC_A;
    const int tid = threadIdx.x;
    const int l0 = p.H[0] * p.W[0], l1 = p.H[1] * p.W[1];
    auto src_of = [&](int a) {   // first chunk of anchor a of image n
        const auto [l, loc] = anchor_level(l0, l1, a);
        return reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.lvl[l]) +
                                              ((long long)n * p.H[l] * p.W[l] + loc) * p.ldc);
    };
    {
        constexpr int BATCH = 6;
        const int total = DEC_A * CH;
        for (int q0 = 0; q0 < total; q0 += 256 * BATCH) {
            uint4 r[BATCH];
            int dst[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int q = q0 + u * 256 + tid;
                const int ai = q / CH, c = q - ai * CH;
                const int a = min(a0 + ai, p.A - 1);
                dst[u] = q < total ? ai * CHP + c : -1;
                r[u] = q < total ? src_of(a)[c + 8 - CB] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (dst[u] >= 0) dsm4[dst[u]] = r[u];
        }
    }
    __syncthreads();
    const auto [l, loc] = anchor_level(l0, l1, min(a0 + tid, p.A - 1));
    const int W = p.W[l];
    const int gy = loc / W, gx = loc - gy * W;
    const uint4* row = dsm4 + tid * CHP;
    float dist[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sd = 0; sd < (BOX ? 4 : 0); ++sd) {
        float v[16];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            Chunk<T> ch;
            ch.v[0] = row[sd * 2 + c];
            chunk_to_f(ch, reinterpret_cast<float(&)[8]>(v[8 * c]));
        }
        dist[sd] = dfl16<T>(v);
    }
    uint4 cls[NCC];
#pragma unroll
    for (int c = 0; c < NCC; ++c) cls[c] = row[CB + c];
    __syncthreads();           // the input tile is dead: the output tile reuses it
    T* tile = reinterpret_cast<T*>(dsm4);   // [(4 + nc)][DEC_A]
    if constexpr (BOX) {
        float b[4];
        dist2bbox(gx, gy, p.stride[l], dist, b);
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[r * DEC_A + tid] = fromf<T>(b[r]);
    }
#pragma unroll
    for (int c = 0; c < NCC; ++c) {
        Chunk<T> ch;
        ch.v[0] = cls[c];
        float f[8];
        chunk_to_f(ch, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[(4 + 8 * c + e) * DEC_A + tid] = fromf<T>(sigmoid<T>(f[e]));
    }
    __syncthreads();
    const gptr<T> yimg = io_global<T>(p.io[1]) + (long long)n * (4 + p.nc) * p.A;
    constexpr int R0 = BOX ? 0 : 4;
    tile_rows_out<T>(tile, yimg, R0, 4 + p.nc - R0, a0, p);
}

template <typename T>
int launch_decode_t(const DecodeArgs& a, hipStream_t s) {
    if (a.a_lo < 0 || a.a_lo >= a.A || (!a.box && sizeof(T) != 2)) return (int)hipErrorInvalidValue;
    const dim3 g((unsigned)((a.A - a.a_lo + DEC_A - 1) / DEC_A), (unsigned)a.B);
    if constexpr (sizeof(T) == 2) {
        // instantiated for the 80-class heads (COCO); other class counts take head_decode
        constexpr int NCC = 10;
        if (a.nc == 8 * NCC && a.A % 8 == 0 && a.a_lo % 8 == 0 && a.ldc % 8 == 0 && a.ldc >= 64 + a.nc) {
            const int lds_in = DEC_A * ((a.box ? 8 : 0) + NCC + 1) * 16, lds_out = (4 + a.nc) * DEC_A * 2;
            const int lds = lds_in > lds_out ? lds_in : lds_out;
            auto kern = a.box ? &head_decode_lds<T, NCC, true> : &head_decode_lds<T, NCC, false>;
            if (int rc = lds_optin(reinterpret_cast<const void*>(kern), 80 * 1024)) return rc;
            hipLaunchKernelGGL(kern, g, dim3(256), lds, s, a);
            return (int)hipGetLastError();
        }
    }
    const int lds = (4 + a.nc) * DEC_A * (int)sizeof(T);
    if (a.A % 8 == 0 && a.a_lo % 8 == 0 && lds <= 64 * 1024) {
        hipLaunchKernelGGL((head_decode<T, true>), g, dim3(256), lds, s, a);
    } else {
        hipLaunchKernelGGL((head_decode<T, false>), g, dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

__global__ void set_io(void** io, const void* x, void* y) {
    io[0] = const_cast<void*>(x);
    io[1] = y;
}

}  // namespace

int launch_decode(int dtype, const DecodeArgs& a, hipStream_t s) {
    switch (dtype) {
        case F32: return launch_decode_t<float>(a, s);
        case F16: return launch_decode_t<_Float16>(a, s);
        case BF16: return launch_decode_t<__bf16>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

int launch_set_io(void** io, const void* x, void* y, hipStream_t s) {
    hipLaunchKernelGGL(set_io, dim3(1), dim3(1), 0, s, io, x, y);
    return (int)hipGetLastError();
}

}  // namespace yh
