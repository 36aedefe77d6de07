// SPPF's three chained 5x5/s1/p2 max-pools (nets/nn.py:83-94):
//   maxpool5    one pool per launch, any dtype
//   sppf_fused  all three in one launch from an LDS copy of the plane (16-bit handles)
#include "common.h"
#include "dtypes.h"

namespace yh {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void maxpool5(const T* src, T* dst, int ldc, int C, int H, int W, int M) {
    // One thread = one pixel x 8 channels; -inf padding == skip out-of-range taps.
    const int cpp = C / 8;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)M * cpp) return;
    const int m = (int)(idx / cpp), cc = (int)(idx - (long long)m * cpp);
    const int HW = H * W;
    const int n = m / HW, r = m - n * HW;
    const int h = r / W, w = r - h * W;
    const T* base = src + (long long)n * HW * ldc + cc * 8;
    float mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mx[e] = -INFINITY;
    for (int dh = -2; dh <= 2; ++dh) {
        const int hi = h + dh;
        if (hi < 0 || hi >= H) continue;
        for (int dw = -2; dw <= 2; ++dw) {
            const int wi = w + dw;
            if (wi < 0 || wi >= W) continue;
            float f[8];
            chunk_to_f(ld_chunk(base + ((long long)hi * W + wi) * ldc), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) mx[e] = fmaxf(mx[e], f[e]);
        }
    }
    st_chunk(dst + (long long)m * ldc + cc * 8, f_to_chunk<T>(mx));
}

// All three pools in one launch: a workgroup owns CPW consecutive 8-channel chunks of one
// image (CPW * 16 contiguous bytes of every pixel per load and store), staged in LDS once;
// y1 = mp(x), y2 = mp(y1), y3 = mp(y2), each as a 1 x 5 row max into a scratch plane and a
// 5 x 1 column max of that (10 LDS reads per output instead of 25), stored to its concat
// slice. Max is exact and associative, so this is bit-identical to three maxpool5 launches
// (which it replaces whenever three planes fit in LDS).
// running max of 8 channels from -inf (fmaxf: NaN taps are skipped, as in maxpool5)
template <typename T>
__device__ __forceinline__ void sppf_acc(float (&mx)[8], uint4 v) {
    Chunk<T> c;
    c.v[0] = v;
    float f[8];
    chunk_to_f(c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) mx[e] = fmaxf(mx[e], f[e]);
}
constexpr int SP_LB = 4;
template <typename T>
__global__ __launch_bounds__(256) void sppf_fused(const PoolArgs a, int cpw, int xcd) {
    extern __shared__ __attribute__((aligned(16))) uint4 pln[];
    const int cpp = a.C / 8, ng = cpp / cpw;
    // xcd: an image's chunk workgroups on one XCD (consecutive logical ids), so the four 16-B
    // chunks of a 64-B segment are fetched into one L2 instead of four
    const int L = xcd ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n = L / ng, cc = (L - n * ng) * cpw;
    const int HW = a.H * a.W, NI = HW * cpw;
    T* img = reinterpret_cast<T*>(a.buf) + (long long)n * HW * a.ldc + cc * 8;
    uint4* p0 = pln;         // pool input / output planes (ping-pong)
    uint4* p1 = pln + NI;
    uint4* rm = pln + 2 * NI;   // row maxima
    // item i = (pixel i / cpw, chunk i % cpw): consecutive threads, consecutive 16 B of a pixel;
    // SP_LB loads in flight per thread before their LDS stores
    for (int i0 = threadIdx.x; i0 < NI; i0 += SP_LB * 256) {
        uint4 v[SP_LB];
#pragma unroll
        for (int u = 0; u < SP_LB; ++u) {
            const int i = min(i0 + u * 256, NI - 1), px = i / cpw, c = i - px * cpw;
            v[u] = *reinterpret_cast<const uint4*>(img + (long long)px * a.ldc + 8 * c);
        }
#pragma unroll
        for (int u = 0; u < SP_LB; ++u)
            if (i0 + u * 256 < NI) p0[i0 + u * 256] = v[u];
    }
    __syncthreads();
    // window taps clamped into the map instead of skipped: a repeated tap leaves a max unchanged,
    // so every item reads a fixed five
    for (int it = 0; it < 3; ++it) {
        const uint4* src = (it & 1) ? p1 : p0;
        uint4* dst = (it & 1) ? p0 : p1;
#pragma unroll 2
        for (int i = threadIdx.x; i < NI; i += 256) {
            const int px = i / cpw, c = i - px * cpw;
            const int h = px / a.W, w = px - h * a.W;
            float mx[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) mx[e] = -INFINITY;
#pragma unroll
            for (int d = -2; d <= 2; ++d) sppf_acc<T>(mx, src[(h * a.W + min(max(w + d, 0), a.W - 1)) * cpw + c]);
            rm[i] = f_to_chunk<T>(mx).v[0];
        }
        __syncthreads();
#pragma unroll 2
        for (int i = threadIdx.x; i < NI; i += 256) {
            const int px = i / cpw, c = i - px * cpw;
            const int h = px / a.W, w = px - h * a.W;
            float mx[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) mx[e] = -INFINITY;
#pragma unroll
            for (int d = -2; d <= 2; ++d) sppf_acc<T>(mx, rm[(min(max(h + d, 0), a.H - 1) * a.W + w) * cpw + c]);
            const uint4 m = f_to_chunk<T>(mx).v[0];
            dst[i] = m;
            *reinterpret_cast<uint4*>(img + (long long)px * a.ldc + (it + 1) * a.C + 8 * c) = m;
        }
        __syncthreads();
    }
}

template <typename T>
int launch_sppf_t(const PoolArgs& a, const LaunchCtx& ctx, hipStream_t s) {
    T* b = reinterpret_cast<T*>(a.buf);
    const int M = a.B * a.H * a.W;
    const Tuning& tune = ctx.tune;
    if constexpr (sizeof(T) == 2) {
        // sppf_fused off: the three maxpool5 launches (the tests compare both)
        if (3 * a.H * a.W * 16 <= 160 * 1024 && a.C % 8 == 0 && tune.sppf_fused) {
            if (int rc = lds_optin(reinterpret_cast<const void*>(&sppf_fused<T>), 160 * 1024)) return rc;
            // chunks per workgroup: 1 while that gives at most 3 workgroups per CU (v11_n b32: 21.2
            // against 22.8 us for 2; v11_x b16 1280: 81.9 against 90.4), else 2 (v11_s b64: 39.4
            // against 57.7 us for 1; 4 / 8 ran 47 / 86 us at v11_n in round 4); sppf_cpw
            // overrides. Halved until it divides the channels and the three planes fit the LDS.
            int cpw = tune.sppf_cpw > 0 ? tune.sppf_cpw : (a.B * (a.C / 8) <= 3 * ctx.num_cus ? 1 : 2);
            while (cpw > 1 && ((a.C / 8) % cpw || 3 * a.H * a.W * cpw * 16 > 160 * 1024))
                cpw >>= 1;
            // an image's chunk workgroups on one XCD (sppf_xcd = 0: hardware order). r06, v11_n b32:
            // 20.4 -> 16.3 us, PMC traffic 2.34x -> 0.67x algorithmic; v11_x b16 1280: 83 -> 56 us
            hipLaunchKernelGGL((sppf_fused<T>), dim3((unsigned)(a.B * (a.C / 8 / cpw))), dim3(256),
                               3 * a.H * a.W * cpw * (int)sizeof(uint4), s, a, cpw, tune.sppf_xcd);
            return (int)hipGetLastError();
        }
    }
    const long long n = (long long)M * (a.C / 8);
    const dim3 g((unsigned)((n + 255) / 256));
    for (int i = 0; i < 3; ++i) {
        hipLaunchKernelGGL((maxpool5<T>), g, dim3(256), 0, s, b + i * a.C, b + (i + 1) * a.C, a.ldc, a.C, a.H, a.W, M);
    }
    return (int)hipGetLastError();
}

}  // namespace

int launch_sppf(int dtype, const PoolArgs& a, const LaunchCtx& ctx, hipStream_t s) {
    switch (dtype) {
        case F32: return launch_sppf_t<float>(a, ctx, s);
        case F16: return launch_sppf_t<_Float16>(a, ctx, s);
        case BF16: return launch_sppf_t<__bf16>(a, ctx, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace yh
