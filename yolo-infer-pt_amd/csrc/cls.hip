// Classifier head (nets/nn.py Classify): conv 1x1 -> CLS_EMBED channels (+ folded BN, SiLU), the
// global average pool, the linear layer and the softmax.
//   cls_pool   a (B, HW, C) in the handle dtype -> e (B, C) fp32: the per-layer path's pool
//   cls_head   x (B, HW, K) -> e (B, N): the 1x1 conv on v_mfma_f32_32x32x16 with the pool in the
//              epilogue, so the (B, HW, N) activations never reach HBM (16-bit handles)
//   cls_fc     z = W e + b in fp32 (W in the handle dtype), tiled over the batch
//   cls_softmax  per row: stable fp32 softmax, the count mask, and the caller's probs / logits /
//              embed written once each
//
// The mean's summation order (both kernels; include/yolo_hip.h): for each (image, channel) one
// fp32 chain from zero over the image's pixels in ascending row-major order, s = (..((a_0 + a_1) +
// a_2) ..) + a_{HW-1}, then e = s * (float)(1.0 / HW). a_p is the conv output rounded to the handle
// dtype, exactly what the per-layer conv stores. Nothing in the order depends on the batch size, on
// the image's place in the batch or on the conv plan.
#include "common.h"
#include "mfma32.h"

namespace yh {

namespace {

// v as an fp32 register value. Without it the compiler folds SiLU's last multiplication and the
// conversion to fp16 into one v_fma_mixlo_f16, i.e. one rounding, where the per-layer conv rounds
// the product to fp32 and then to fp16: the two differ in about one output in 10^4.
__device__ __forceinline__ float keep_f32(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// ---------------------------------------------------------------- cls_pool
// one thread per (image, channel): the chain over the image's pixels
template <typename T>
__global__ __launch_bounds__(256) void cls_pool(const ClsPoolArgs A) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= A.C) return;
    const T* p = reinterpret_cast<const T*>(A.a) + (long long)b * A.HW * A.lda + c;
    float run = 0.f;
    for (int i = 0; i < A.HW; ++i) run += tof(p[(long long)i * A.lda]);
    A.e[(long long)b * A.C + c] = run * A.inv;
}

// ---------------------------------------------------------------- cls_head
// A workgroup owns images [b0, b0 + G) = P <= 128 consecutive pixels of the flattened map, staged
// once into LDS (pixel stride K + 8 elements; the rows that pad P to whole 32-pixel B tiles are
// zero and never enter a sum). Wave w computes the A tiles (32 couts) w, w + 4, ..: per tile the
// canonical K walk of conv_mx.h (one MFMA step per 16-channel block, ascending, from a zero fp32
// accumulator) against every B tile, A fragments from the fragment-ordered weights (one KB per
// load), then bias, SiLU and the rounding to T as the per-layer conv's epilogue does them. The
// rounded values of one 32 x 32 tile go to the wave's LDS scratch, and lanes 0..31 (one cout each)
// walk its pixels in ascending order, carrying the chain across the B tiles and closing it at
// every image's last pixel.
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void cls_head(const ClsHeadArgs A) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.x * A.G;
    const int nimg = A.B - b0 < A.G ? A.B - b0 : A.G;
    const int P = nimg * A.HW;
    const int nt = (P + 31) >> 5;   // 1..4
    const long long m0 = (long long)b0 * A.HW;
    const int row = A.K + 8;

    // stage the input: 16-B chunks, zero rows past P
    const int cpp = A.K >> 3, total = nt * 32 * cpp;
    for (int q = threadIdx.x; q < total; q += CLS_THREADS) {
        const int px = q / cpp, c = q - px * cpp;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (px < P) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(A.x) + (m0 + px) * A.ldx + c * 8);
        *reinterpret_cast<uint4*>(sm + ((size_t)px * row + c * 8) * 2) = v;
    }
    __syncthreads();

    float* scr = reinterpret_cast<float*>(sm + (size_t)nt * 32 * row * 2) + wv * (32 * 33);
    const bool silu_act = A.act == ACT_SILU;
    const int npc = A.K >> 7, na = A.N >> 5;
    for (int a = wv; a < na; a += CLS_THREADS / 64) {
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
        float4 bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const float4*>(A.bias + a * 32 + 8 * q + 4 * h);
        for (int pc = 0; pc < npc; ++pc) {
            // 8 K blocks of the tile's 32 couts: fragment (a, kb) is one KB, lane-major
            const char* wb = reinterpret_cast<const char*>(A.w) + (((long long)a * (A.wld >> 4) + pc * 8) * 64 + lane) * 16;
            uint4 f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = *reinterpret_cast<const uint4*>(wb + i * 1024);
            // lane (l32, h) of B tile j: pixel 32 j + l32, channels 16 kb + 8 h ..
            const char* xb = sm + ((size_t)l32 * row + pc * 128 + 8 * h) * 2;
#pragma unroll
            for (int ih = 0; ih < 2; ++ih) {
                uint4 x[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nt) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            x[j][i] = *reinterpret_cast<const uint4*>(xb + (size_t)j * 32 * row * 2 + (ih * 4 + i) * 32);
                    }
                // per accumulator the K blocks in ascending order; the B tiles interleaved
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nt) acc[j] = Mfma32<T>::step(f[ih * 4 + i], x[j][i], acc[j]);
            }
        }
        // register i of lane (l32, h): cout 32 a + (i & 3) + 8 (i >> 2) + 4 h, pixel 32 j + l32
        float run = 0.f;
        int inimg = 0, img = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nt) break;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bb = bq[q];
                const float v[4] = {acc[j][4 * q] + bb.x, acc[j][4 * q + 1] + bb.y, acc[j][4 * q + 2] + bb.z,
                                    acc[j][4 * q + 3] + bb.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    scr[l32 * 33 + 8 * q + 4 * h + e] = tof(fromf<T>(keep_f32(silu_act ? silu<T>(v[e]) : v[e])));
            }
            __syncthreads();
            if (lane < 32) {
                const int np = P - j * 32 < 32 ? P - j * 32 : 32;
                for (int p = 0; p < np; ++p) {
                    run += scr[p * 33 + lane];
                    if (++inimg == A.HW) {
                        A.e[(long long)(b0 + img) * A.N + a * 32 + lane] = run * A.inv;
                        run = 0.f;
                        inimg = 0;
                        ++img;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- cls_fc
template <typename T> struct FcLoad;
template <> struct FcLoad<float> {
    static __device__ __forceinline__ void ld8(const void* w, long long i, float (&f)[8]) {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(w) + i);
        const float4 a = p[0], b = p[1];
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
};
template <typename T> struct FcLoad {
    static __device__ __forceinline__ void ld8(const void* w, long long i, float (&f)[8]) {
        const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(w) + i);
        const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = tof(e[k]);
    }
};

// A workgroup holds the embeddings of CLS_FC_TB images in LDS and computes CLS_FC_TN classes for
// them, so a weight row is read once per CLS_FC_TB images. A wave owns a class at a time: lane l
// accumulates the 8-channel chunks l, l + 64, .. with fmaf in ascending order, then the lanes'
// partials are added in a fixed xor butterfly (32, 16, .., 1) and the bias last.
template <typename T>
__global__ __launch_bounds__(256) void cls_fc(const ClsFcArgs A) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    float* es = reinterpret_cast<float*>(sm);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.y * CLS_FC_TB;
    const int nb = A.B - b0 < CLS_FC_TB ? A.B - b0 : CLS_FC_TB;
    const int K4 = A.K >> 2;
    for (int q = threadIdx.x; q < CLS_FC_TB * K4; q += 256) {
        const int b = q / K4, c = q - b * K4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < nb) v = *reinterpret_cast<const float4*>(A.e + (long long)(b0 + b) * A.K + c * 4);
        *reinterpret_cast<float4*>(es + (size_t)b * A.K + c * 4) = v;
    }
    __syncthreads();
    constexpr int CPW = CLS_FC_TN / 4;
    const int n0 = blockIdx.x * CLS_FC_TN + wv * CPW;
    const int nch = A.K >> 3;
    for (int cn = 0; cn < CPW; ++cn) {
        const int n = n0 + cn;
        if (n >= A.nc) break;   // wave-uniform
        float acc[CLS_FC_TB];
#pragma unroll
        for (int b = 0; b < CLS_FC_TB; ++b) acc[b] = 0.f;
        for (int c = lane; c < nch; c += 64) {
            float wf[8];
            FcLoad<T>::ld8(A.w, (long long)n * A.wld + c * 8, wf);
#pragma unroll
            for (int b = 0; b < CLS_FC_TB; ++b) {
                const float4 e0 = *reinterpret_cast<const float4*>(es + (size_t)b * A.K + c * 8);
                const float4 e1 = *reinterpret_cast<const float4*>(es + (size_t)b * A.K + c * 8 + 4);
                float s = acc[b];
                s = fmaf(wf[0], e0.x, s); s = fmaf(wf[1], e0.y, s); s = fmaf(wf[2], e0.z, s); s = fmaf(wf[3], e0.w, s);
                s = fmaf(wf[4], e1.x, s); s = fmaf(wf[5], e1.y, s); s = fmaf(wf[6], e1.z, s); s = fmaf(wf[7], e1.w, s);
                acc[b] = s;
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int b = 0; b < CLS_FC_TB; ++b) {
            float s = acc[b];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == b) mine = s;
        }
        if (lane < nb) A.z[(long long)(b0 + lane) * A.ldz + n] = mine + A.bias[n];
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// one wave per image: probs = exp(z - max z) / sum, every output element written exactly once;
// rows at or beyond n = clamp(*count, 0, B) are zero in all three outputs
__global__ __launch_bounds__(64) void cls_softmax(const ClsFcArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float* probs = reinterpret_cast<float*>(const_cast<void*>(A.io[2]));
    float* logits = reinterpret_cast<float*>(const_cast<void*>(A.io[3]));
    float* embed = reinterpret_cast<float*>(const_cast<void*>(A.io[4]));
    const int* count = reinterpret_cast<const int*>(A.io[5]);
    int n = A.B;
    if (count) {
        n = *count;
        n = n < 0 ? 0 : (n > A.B ? A.B : n);
    }
    const bool live = b < n;
    const float* z = A.z + (long long)b * A.ldz;
    const float* e = A.e + (long long)b * A.K;
    if (embed)
        for (int i = lane; i < A.K; i += 64) embed[(long long)b * A.K + i] = live ? e[i] : 0.f;
    if (logits)
        for (int i = lane; i < A.nc; i += 64) logits[(long long)b * A.nc + i] = live ? z[i] : 0.f;
    if (!live) {
        for (int i = lane; i < A.nc; i += 64) probs[(long long)b * A.nc + i] = 0.f;
        return;
    }
    float m = -3.0e38f;
    for (int i = lane; i < A.nc; i += 64) m = fmaxf(m, z[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < A.nc; i += 64) s += expf(z[i] - m);
    s = wave_sum(s);
    for (int i = lane; i < A.nc; i += 64) probs[(long long)b * A.nc + i] = expf(z[i] - m) / s;
}

__global__ void set_io_cls(void** io, const void* x, float* probs, float* logits, float* embed, const int* count) {
    io[0] = const_cast<void*>(x);
    io[1] = nullptr;
    io[2] = probs;
    io[3] = logits;
    io[4] = embed;
    io[5] = const_cast<int*>(count);
}

template <typename T>
int launch_cls_pool_t(const ClsPoolArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.HW <= 0 || a.C <= 0 || a.B > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((cls_pool<T>), dim3((unsigned)((a.C + 255) / 256), (unsigned)a.B), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

template <typename T>
int launch_cls_head_t(const ClsHeadArgs& a, hipStream_t s) {
    const int lds = cls_head_lds(a.K, a.HW);
    if (a.B <= 0 || lds <= 0 || a.G != cls_head_group(a.K, a.HW) || a.G * a.HW > 128 || a.N % 128 || a.wld < a.K ||
        a.wld % 16 || a.ldx % 8)
        return (int)hipErrorInvalidValue;
    if (int rc = lds_optin(reinterpret_cast<const void*>(&cls_head<T>), 160 * 1024)) return rc;
    hipLaunchKernelGGL((cls_head<T>), dim3((unsigned)((a.B + a.G - 1) / a.G)), dim3(CLS_THREADS), lds, s, a);
    return (int)hipGetLastError();
}

template <typename T>
int launch_cls_fc_t(const ClsFcArgs& a, hipStream_t s) {
    const int lds = CLS_FC_TB * a.K * 4;
    if (a.B <= 0 || a.nc <= 0 || a.K % 8 || a.wld < a.K || a.wld % 8 || a.ldz < a.nc || lds > 160 * 1024 ||
        (a.B + CLS_FC_TB - 1) / CLS_FC_TB > 65535)
        return (int)hipErrorInvalidValue;
    if (int rc = lds_optin(reinterpret_cast<const void*>(&cls_fc<T>), 160 * 1024)) return rc;
    hipLaunchKernelGGL((cls_fc<T>), dim3((unsigned)((a.nc + CLS_FC_TN - 1) / CLS_FC_TN), (unsigned)((a.B + CLS_FC_TB - 1) / CLS_FC_TB)),
                       dim3(256), lds, s, a);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(cls_softmax, dim3((unsigned)a.B), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_cls_pool(int dtype, const ClsPoolArgs& a, hipStream_t s) {
    switch (dtype) {
        case F32: return launch_cls_pool_t<float>(a, s);
        case F16: return launch_cls_pool_t<_Float16>(a, s);
        case BF16: return launch_cls_pool_t<__bf16>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

int launch_cls_head(int dtype, const ClsHeadArgs& a, hipStream_t s) {
    switch (dtype) {
        case F16: return launch_cls_head_t<_Float16>(a, s);
        case BF16: return launch_cls_head_t<__bf16>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

int launch_cls_fc(int dtype, const ClsFcArgs& a, hipStream_t s) {
    switch (dtype) {
        case F32: return launch_cls_fc_t<float>(a, s);
        case F16: return launch_cls_fc_t<_Float16>(a, s);
        case BF16: return launch_cls_fc_t<__bf16>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

int launch_set_io_cls(void** io, const void* x, float* probs, float* logits, float* embed, const int* count,
                      hipStream_t s) {
    hipLaunchKernelGGL(set_io_cls, dim3(1), dim3(1), 0, s, io, x, probs, logits, embed, count);
    return (int)hipGetLastError();
}

}  // namespace yh
