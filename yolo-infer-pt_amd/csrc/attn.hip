// C2PSA attention core (nets/nn.py:111-123): softmax(q^T k * scale) v + pe(v) per head.
//   psa_attention       fp32 handles: one query per lane, pe(v) in its epilogue
//   psa_attention_mfma  16-bit: one wave per 16 queries, K / V straight from the qkv buffer
//   psa_attention_lds   16-bit: K / V through LDS in chunks, once per workgroup
//   psa_attention_full  16-bit: a head's whole K / V in LDS, pe(v) in its epilogue
//   pe_add              the positional depthwise conv pe(v) added after _mfma / _lds
// The three 16-bit kernels differ in how K and V reach the MFMAs and in nothing else: the
// per-16-key-block softmax (softmax_step) and the normalised, rounded output (store_o / pack4)
// are written once below, which makes their outputs bit-identical (tests/test_gpu_fusion.py).
// The two LDS kernels keep a token-row staging loop each: one templated loop (1 or AF_LB loads per
// batch) changed psa_attention_lds's registers (50 VGPRs -> 48 .. 51, 36 SGPRs -> 38 .. 42), and
// sharing only the chunk's LDS store cost psa_attention_full 5 VGPRs (62 -> 67).
#include "common.h"
#include "dtypes.h"
#include <algorithm>

namespace yh {

namespace {

constexpr int ATT_Q = 64;   // queries per block (one wave, one query per lane)
constexpr int ATT_KB = 64;  // keys staged per LDS tile
constexpr int DK = 32, DH = 64;

template <typename T>
__global__ __launch_bounds__(ATT_Q) void psa_attention(const AttnArgs p) {
    __shared__ float ks[ATT_KB][DK];
    __shared__ float vs[ATT_KB][DH];
    const int qi = blockIdx.x * ATT_Q + threadIdx.x;
    const int head = blockIdx.y, n = blockIdx.z;
    const int per = 2 * DK + DH;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long long)n * p.T * p.ldq + head * per;
    const bool live = qi < p.T;

    float q[DK];
    if (live) {
#pragma unroll
        for (int c = 0; c < DK; c += 8) {
            float f[8];
            chunk_to_f(ld_chunk(base + (long long)qi * p.ldq + c), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[c + e] = f[e];
        }
    } else {
#pragma unroll
        for (int c = 0; c < DK; ++c) q[c] = 0.f;
    }
    float acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.f;
    float mrun = -INFINITY, lrun = 0.f;

    for (int kb = 0; kb < p.T; kb += ATT_KB) {
        const int nk = min(ATT_KB, p.T - kb);
        __syncthreads();
        if ((int)threadIdx.x < nk) {
            const T* row = base + (long long)(kb + threadIdx.x) * p.ldq;
#pragma unroll
            for (int c = 0; c < DK; c += 8) {
                float f[8];
                chunk_to_f(ld_chunk(row + DK + c), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) ks[threadIdx.x][c + e] = f[e];
            }
#pragma unroll
            for (int c = 0; c < DH; c += 8) {
                float f[8];
                chunk_to_f(ld_chunk(row + 2 * DK + c), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) vs[threadIdx.x][c + e] = f[e];
            }
        }
        __syncthreads();
        float s[ATT_KB];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < ATT_KB; ++j) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < DK; ++c) d = fmaf(q[c], ks[j][c], d);
            d = (j < nk) ? d * p.scale : -INFINITY;
            s[j] = d;
            mx = fmaxf(mx, d);
        }
        const float mnew = fmaxf(mrun, mx);
        const float corr = expf(mrun - mnew);
        lrun *= corr;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] *= corr;
#pragma unroll
        for (int j = 0; j < ATT_KB; ++j) {
            const float pj = (j < nk) ? expf(s[j] - mnew) : 0.f;
            lrun += pj;
#pragma unroll
            for (int d = 0; d < DH; ++d) acc[d] = fmaf(pj, vs[j][d], acc[d]);
        }
        mrun = mnew;
    }
    if (!live) return;

    // epilogue: normalise, add pe(v) = depthwise 3x3 over v (+ bias), store.
    const float inv = 1.0f / lrun;
    const int hq = qi / p.Ws, wq = qi - hq * p.Ws;
    const int C = p.heads * DH;
    float o[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] = acc[d] * inv + p.pe_b[head * DH + d];
    for (int kh = 0; kh < 3; ++kh) {
        const int hi = hq - 1 + kh;
        if (hi < 0 || hi >= p.Hs) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int wi = wq - 1 + kw;
            if (wi < 0 || wi >= p.Ws) continue;
            const T* v = base + (long long)(hi * p.Ws + wi) * p.ldq + 2 * DK;
            const float* wt = p.pe_w + (kh * 3 + kw) * C + head * DH;
#pragma unroll
            for (int c = 0; c < DH; c += 8) {
                float f[8];
                chunk_to_f(ld_chunk(v + c), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[c + e] = fmaf(wt[c + e], f[e], o[c + e]);
            }
        }
    }
    T* out = reinterpret_cast<T*>(p.out) + ((long long)n * p.T + qi) * p.ldo + head * DH;
#pragma unroll
    for (int c = 0; c < DH; c += 8) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = o[c + e];
        st_chunk(out + c, f_to_chunk<T>(f));
    }
}

// 16-bit attention on MFMA. One wave = 16 queries of one (image, head); keys in
// blocks of 16:
//   S^T = K_blk . Q^T        one v_mfma_f32_16x16x32 (dk = 32): A = K rows, B = Q rows,
//                            16 B per lane; the accumulator holds
//                            S^T[key 4g+r][query li] (g = lane/16).
//   online softmax           per query = per lane column: in-lane max/sum over r plus two
//                            row swaps (16, 32); exact exp, fp32 state (softmax_step).
//   O^T += V^T_blk . P^T     four v_mfma_f32_16x16x16 (dh = 64): B = P^T is exactly the
//                            softmax'd accumulator of the S^T MFMA (no data movement),
//                            A = V^T read from an LDS copy of V_blk with
//                            ds_read_b64_tr_b16 (hardware transpose).
// pe(v) (the depthwise positional conv, nets/nn.py:122) is added by pe_add below.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

template <typename T> struct Mma16;
template <> struct Mma16<__bf16> {
    static __device__ __forceinline__ f32x4 step(s16x4 a, s16x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma16<_Float16> {
    static __device__ __forceinline__ f32x4 step(s16x4 a, s16x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
    }
};

__device__ __forceinline__ s16x4 lds_tr16(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) s16x4* lp;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(const_cast<void*>(p)));
#else
    (void)p;
    return s16x4{0, 0, 0, 0};
#endif
}

// Reductions over the four 16-lane rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) by gfx950's
// row swaps (v_permlane16_swap / v_permlane32_swap: VALU, no LDS round trip as a ds_bpermute
// shuffle has). Each step combines a lane's value with its xor-16 / xor-32 partner's, the two
// operands in a fixed order; max and + commute, so every lane gets the bits the shuffle form
// (own value op partner's) gives.
__device__ __forceinline__ float rows4_max(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(t[0]), __uint_as_float(t[1]));
#else
    return x;
#endif
}
__device__ __forceinline__ float rows4_sum(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(t[0]) + __uint_as_float(t[1]);
#else
    return x;
#endif
}

// 16 bytes from p when ok, else zeros: a branch around the load. (The `ok ? *p : zero`
// form lets the compiler load through a select of p and a stack zero, a flat load - counted
// in lgkmcnt as well as vmcnt - even when p is global or LDS.)
template <typename P>
__device__ __forceinline__ uint4 ld16_if(bool ok, const P* p) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *reinterpret_cast<const uint4*>(p);
    return v;
}

// The online-softmax step of one 16-key block, the one place the three 16-bit kernels'
// per-block arithmetic is written. s = the S^T accumulator (the lane's four keys key0 .. key0 + 3
// against its query); keys from kend on are masked. Rescales the output accumulators and returns
// the new running maximum and sum with the weights rounded to T, the B operand of the P.V MFMAs.
// (mrun and lrun come back by value: as references they cost psa_attention_lds<_Float16> a VGPR.)
struct SoftmaxStep { s16x4 pb; float mrun, lrun; };
template <typename T>
__device__ __forceinline__ SoftmaxStep softmax_step(const f32x4& s, int key0, int kend, float scale, float mrun,
                                                    float lrun, f32x4 (&o)[4]) {
    float sv[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sv[r] = (key0 + r < kend) ? s[r] * scale : -INFINITY;
        mx = fmaxf(mx, sv[r]);
    }
    mx = rows4_max(mx);
    const float mnew = fmaxf(mrun, mx);
    const float corr = __expf(mrun - mnew);
    float ps = 0.f;
    s16x4 pb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float pr = __expf(sv[r] - mnew);
        pb[r] = __builtin_bit_cast(short, fromf<T>(pr));
        ps += pr;
    }
    ps = rows4_sum(ps);
    lrun = lrun * corr + ps;
    mrun = mnew;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] *= corr;
    return SoftmaxStep{pb, mrun, lrun};
}

// four values rounded to T, as the 8 bytes a lane stores
template <typename T>
__device__ __forceinline__ uint2 pack4(const float (&v)[4]) {
    unsigned u[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) u[r] = (unsigned short)__builtin_bit_cast(short, fromf<T>(v[r]));
    return make_uint2(u[0] | (u[1] << 16), u[2] | (u[3] << 16));
}
// a lane's normalised outputs o * (1 / lrun): channels 16 t + 4 g + r of its query's row `out`
template <typename T>
__device__ __forceinline__ void store_o(T* out, int g, const f32x4 (&o)[4], float lrun) {
    const float inv = 1.0f / lrun;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float v[4] = {o[t][0] * inv, o[t][1] * inv, o[t][2] * inv, o[t][3] * inv};
        *reinterpret_cast<uint2*>(out + 16 * t + 4 * g) = pack4<T>(v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void psa_attention_mfma(const AttnArgs p) {
    __shared__ __attribute__((aligned(16))) T vlds[4][16 * DH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * 4 + wave) * 16;
    const int head = blockIdx.y, n = blockIdx.z;
    if (q0 >= p.T) return;  // wave-uniform; the kernel has no block-level barrier
    const int g = lane >> 4, li = lane & 15;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long long)n * p.T * p.ldq + head * (2 * DK + DH);
    const int q = q0 + li;
    const uint4 qf = ld16_if(q < p.T, base + (long long)q * p.ldq + 8 * g);
    f32x4 o[4] = {};
    float mrun = -INFINITY, lrun = 0.f;
    T* vl = vlds[wave];
    for (int kb = 0; kb < p.T; kb += 16) {
        const int key = kb + li;
        const uint4 kf = ld16_if(key < p.T, base + (long long)key * p.ldq + DK + 8 * g);
        uint4 vv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h, kr = c >> 3, ch = c & 7;
            vv[h] = ld16_if((kb + kr < p.T), base + (long long)(kb + kr) * p.ldq + 2 * DK + ch * 8);
        }
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        Mma<T>::step(s, &kf, &qf);
        const auto [pb, m, l] = softmax_step<T>(s, kb + 4 * g, p.T, p.scale, mrun, lrun, o);
        mrun = m, lrun = l;
        // V block -> LDS [16 keys][64 d]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            *reinterpret_cast<uint4*>(vl + (c >> 3) * DH + (c & 7) * 8) = vv[h];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const s16x4 a = lds_tr16(vl + (4 * g + (li >> 2)) * DH + 16 * t + 4 * (li & 3));
            o[t] = Mma16<T>::step(a, pb, o[t]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    if (q >= p.T) return;
    store_o(reinterpret_cast<T*>(p.out) + ((long long)n * p.T + q) * p.ldo + head * DH, g, o, lrun);
}

// The same attention with K and V staged in LDS once per workgroup (each wave read
// its (image, head)'s whole K and V from L2, 7x the algorithmic bytes). A workgroup of AT_NW
// waves owns AT_NW 16-query blocks of one (image, head); keys go through LDS in chunks of
// AT_KC (every key's K and V loaded once per workgroup, 16-B loads of whole token rows), and
// every wave calls softmax_step on the same key blocks in the same order as psa_attention_mfma,
// so the outputs are bit-identical. V rows are padded to 160 B: the 8 keys of a
// ds_read_b64_tr_b16 lane group then hit disjoint banks.
constexpr int AT_NW = 8, AT_KC = 256, AT_VS = DH + 16;   // V row stride (elements)
template <typename T>
__global__ __launch_bounds__(64 * AT_NW) void psa_attention_lds(const AttnArgs p) {
    __shared__ __attribute__((aligned(16))) T klds[AT_KC * DK];
    __shared__ __attribute__((aligned(16))) T vlds[AT_KC * AT_VS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // 1-D grid, block id = (image, head) pair + pairs x query group: the query groups of one
    // pair are 8 x k ids apart (pair count a multiple of 8), i.e. on one XCD / L2, where their
    // K / V reads meet
    const int np = (int)gridDim.x / ((p.T + 16 * AT_NW - 1) / (16 * AT_NW));
    const int qg = blockIdx.x / np, pair = blockIdx.x - qg * np;
    const int n = pair / p.heads, head = pair - n * p.heads;
    const int q0 = (qg * AT_NW + wave) * 16;
    const int g = lane >> 4, li = lane & 15;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long long)n * p.T * p.ldq + head * (2 * DK + DH);
    const int q = q0 + li;
    const bool qwave = q0 < p.T;   // wave-uniform: waves past the last query block only load
    const uint4 qf = ld16_if((qwave && q < p.T), base + (long long)q * p.ldq + 8 * g);
    f32x4 o[4] = {};
    float mrun = -INFINITY, lrun = 0.f;
    for (int k0 = 0; k0 < p.T; k0 += AT_KC) {
        const int nk = min(AT_KC, p.T - k0);
        __syncthreads();   // the previous chunk is read by every wave
        // token row [k(32) | v(64)] = 12 chunks of 16 B: 4 K chunks, 8 V chunks; the rows of the
        // last 16-key block past the end are zeros (psa_attention_mfma's V of missing keys)
        const int nk16 = (nk + 15) & ~15;
        for (int i = threadIdx.x; i < nk16 * 12; i += 64 * AT_NW) {
            const int r = i / 12, c = i - r * 12;
            const uint4 v = ld16_if(r < nk, base + (long long)(k0 + r) * p.ldq + DK + 8 * c);
            if (c < 4) *reinterpret_cast<uint4*>(klds + r * DK + 8 * c) = v;
            else *reinterpret_cast<uint4*>(vlds + r * AT_VS + 8 * (c - 4)) = v;
        }
        __syncthreads();
        if (!qwave) continue;
        for (int kb = 0; kb < nk; kb += 16) {
            const int key = kb + li;
            const uint4 kf = ld16_if(key < nk, klds + key * DK + 8 * g);
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            Mma<T>::step(s, &kf, &qf);
            const auto [pb, m, l] = softmax_step<T>(s, kb + 4 * g, nk, p.scale, mrun, lrun, o);
            mrun = m, lrun = l;
            const int kr = kb + 4 * g + (li >> 2);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s16x4 a = lds_tr16(vlds + kr * AT_VS + 16 * t + 4 * (li & 3));
                o[t] = Mma16<T>::step(a, pb, o[t]);
            }
        }
    }
    if (!qwave || q >= p.T) return;
    store_o(reinterpret_cast<T*>(p.out) + ((long long)n * p.T + q) * p.ldo + head * DH, g, o, lrun);
}

// One workgroup per (image, head) with the head's whole K and V in LDS (maps of up to
// AF_TMAX tokens: v11 at 640 x 640 has 400): every qkv byte is read once, and pe_add's
// positional term is added in the epilogue from the V already in LDS, so the attention
// output is written once (7x, then 4.96x the algorithmic bytes with the
// chunked kernel and a separate pe_add). Each wave calls softmax_step for its 16-query blocks
// on psa_attention_mfma's key blocks in the same order, rounds the output as store_o stores
// it, then adds pe_b and the 3 x 3 taps in pe_add's order with pe_add's fmaf chain:
// the result is bit-identical to psa_attention_mfma / psa_attention_lds followed by pe_add.
constexpr int AF_NW = 16, AF_TMAX = 640, AF_LB = 8;
__host__ __device__ inline int af_lds_bytes(int T) {
    const int t16 = (T + 15) & ~15;
    return t16 * (DK + AT_VS) * 2 + 10 * DH * 4;
}
template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void psa_attention_full(const AttnArgs p, int B) {
    extern __shared__ __attribute__((aligned(16))) char afs[];
    const int t16 = (p.T + 15) & ~15;
    T* klds = reinterpret_cast<T*>(afs);
    T* vlds = klds + t16 * DK;
    float* pew = reinterpret_cast<float*>(vlds + t16 * AT_VS);   // [9][DH] of this head, then pe_b
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // block id = (image, head) pair + pairs x split: the workgroups of one pair are 8 x k ids
    // apart when the pair count is a multiple of 8, i.e. on the same XCD (one L2), so the second
    // one's K / V reads meet the first one's in L2
    const int np = p.heads * B, qs = gridDim.x / np;   // workgroups per (image, head), splitting the queries
    const int split = blockIdx.x / np, pair = blockIdx.x - split * np;
    const int n = pair / p.heads, head = pair - n * p.heads;
    const int g = lane >> 4, li = lane & 15;
    const int C = p.heads * DH;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long long)n * p.T * p.ldq + head * (2 * DK + DH);
    // every token row once (zeros past the last token: the per-wave kernel's missing keys), the
    // head's positional weights and bias
    // (batches of AF_LB loads in flight per thread, then their LDS stores: a load-store pair per
    // iteration would put one memory round trip per iteration on the prologue's critical path)
    for (int i0 = threadIdx.x; i0 < t16 * 12; i0 += AF_LB * 64 * NW) {
        uint4 v[AF_LB];
#pragma unroll
        for (int u = 0; u < AF_LB; ++u) {
            const int i = i0 + u * 64 * NW, r = i / 12, c = i - r * 12;
            v[u] = ld16_if(i < t16 * 12 && r < p.T, base + (long long)r * p.ldq + DK + 8 * c);
        }
#pragma unroll
        for (int u = 0; u < AF_LB; ++u) {
            const int i = i0 + u * 64 * NW, r = i / 12, c = i - r * 12;
            if (i >= t16 * 12) break;
            if (c < 4) *reinterpret_cast<uint4*>(klds + r * DK + 8 * c) = v[u];
            else *reinterpret_cast<uint4*>(vlds + r * AT_VS + 8 * (c - 4)) = v[u];
        }
    }
    for (int i = threadIdx.x; i < 10 * DH; i += 64 * NW)
        pew[i] = i < 9 * DH ? p.pe_w[(i / DH) * C + head * DH + (i % DH)] : p.pe_b[head * DH + i - 9 * DH];
    __syncthreads();
    const int nqb = (p.T + 15) >> 4;
    for (int qb = split * NW + wave; qb < nqb; qb += qs * NW) {   // wave-uniform
        const int q = qb * 16 + li;
        const uint4 qf = ld16_if(q < p.T, base + (long long)q * p.ldq + 8 * g);
        f32x4 o[4] = {};
        float mrun = -INFINITY, lrun = 0.f;
        // K rows past the last token are zeros up to t16; reads past t16 (the block after the
        // last) are clamped: their scores are never used
        const T* kp = klds + 8 * g;
        uint4 kf = *reinterpret_cast<const uint4*>(kp + min(li, t16 - 1) * DK);
        for (int kb = 0; kb < p.T; kb += 16) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            Mma<T>::step(s, &kf, &qf);
            // the next block's K fragment and this block's V fragments: LDS reads issued ahead
            // of the softmax chain they do not depend on
            kf = *reinterpret_cast<const uint4*>(kp + min(kb + 16 + li, t16 - 1) * DK);
            const int kr = kb + 4 * g + (li >> 2);
            s16x4 va[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) va[t] = lds_tr16(vlds + kr * AT_VS + 16 * t + 4 * (li & 3));
            const auto [pb, m, l] = softmax_step<T>(s, kb + 4 * g, p.T, p.scale, mrun, lrun, o);
            mrun = m, lrun = l;
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = Mma16<T>::step(va[t], pb, o[t]);
        }
        if (q >= p.T) continue;
        const float inv = 1.0f / lrun;
        const int hq = q / p.Ws, wq = q - hq * p.Ws;
        T* out = reinterpret_cast<T*>(p.out) + ((long long)n * p.T + q) * p.ldo + head * DH;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float acc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fromf_round<T>(o[t][r] * inv) + pew[9 * DH + 16 * t + 4 * g + r];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int hi = hq - 1 + kh;
                if (hi < 0 || hi >= p.Hs) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int wi = wq - 1 + kw;
                    if (wi < 0 || wi >= p.Ws) continue;
                    const T* vr = vlds + (hi * p.Ws + wi) * AT_VS + 16 * t + 4 * g;
                    const float* wt = pew + (kh * 3 + kw) * DH + 16 * t + 4 * g;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = fmaf(wt[r], tof(vr[r]), acc[r]);
                }
            }
            *reinterpret_cast<uint2*>(out + 16 * t + 4 * g) = pack4<T>(acc);
        }
    }
}

// out[:, c] += pe_b[c] + sum_taps pe_w[tap][c] * v[nbr][c]   (c = head*dh + d; v lives in qkv)
template <typename T>
__global__ __launch_bounds__(256) void pe_add(const AttnArgs p, int B) {
    const int C = p.heads * DH, cpp = C / 8;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * p.T * cpp) return;
    const int cc = (int)(idx % cpp);
    const long long tok = idx / cpp;
    const int n = (int)(tok / p.T), t = (int)(tok - (long long)n * p.T);
    const int h = t / p.Ws, w = t - h * p.Ws;
    const int c0 = cc * 8, head = c0 / DH, d0 = c0 - head * DH;
    const T* vbase = reinterpret_cast<const T*>(p.qkv) + (long long)n * p.T * p.ldq + head * (2 * DK + DH) + 2 * DK + d0;
    T* o = reinterpret_cast<T*>(p.out) + tok * p.ldo + c0;
    float acc[8];
    chunk_to_f(ld_chunk(o), acc);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += p.pe_b[c0 + e];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int hi = h - 1 + kh;
        if (hi < 0 || hi >= p.Hs) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int wi = w - 1 + kw;
            if (wi < 0 || wi >= p.Ws) continue;
            float f[8];
            chunk_to_f(ld_chunk(vbase + (long long)(hi * p.Ws + wi) * p.ldq), f);
            const float* wt = p.pe_w + (kh * 3 + kw) * C + c0;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(wt[e], f[e], acc[e]);
        }
    }
    st_chunk(o, f_to_chunk<T>(acc));
}

template <typename T>
int launch_attention_t(const AttnArgs& a, int B, const LaunchCtx& ctx, hipStream_t s) {
    if (a.dk != DK || a.dh != DH) return (int)hipErrorInvalidValue;
    const Tuning& tune = ctx.tune;
    if constexpr (sizeof(T) == 2) {
        // attn_full off: the chunked kernel + pe_add where the full one applies; attn_lds off: the
        // per-wave chunked kernel. The tests compare all three bit for bit.
        if (a.T <= AF_TMAX && a.Ws > 0 && a.Hs * a.Ws == a.T && tune.attn_full) {
            // Every wave runs one 16-query block's serial chain over all key blocks, so the launch
            // lasts about one chain when each wave has at most one block and every workgroup a CU
            // of its own (one fits per CU: the K / V staging takes ~86 KB of LDS). Default: 8-wave
            // workgroups, ceil(blocks / 8) per (image, head), when those fit the CUs in one round
            // (v11_n, batch 32: 256 workgroups, 20 us); else 16-wave ones, two per (image, head)
            // (27-28 us there; at one, 64 workgroups, 39 us). attn_nw (8 / 16) and attn_qs
            // (workgroups per (image, head)) override.
            const int nqb = (a.T + 15) >> 4, pairs = a.heads * B, q8 = (nqb + 7) / 8;
            const int nw = tune.attn_nw ? (tune.attn_nw == 8 ? 8 : AF_NW) : (pairs * q8 <= ctx.num_cus ? 8 : AF_NW);
            const int qs = std::max(1, std::min(tune.attn_qs > 0 ? tune.attn_qs : (nw == 8 ? q8 : 2), (nqb + nw - 1) / nw));
            const void* k = nw == 8 ? reinterpret_cast<const void*>(&psa_attention_full<T, 8>)
                                    : reinterpret_cast<const void*>(&psa_attention_full<T, AF_NW>);
            if (int rc = lds_optin(k, 160 * 1024)) return rc;
            if (nw == 8)
                hipLaunchKernelGGL((psa_attention_full<T, 8>), dim3((unsigned)(a.heads * B * qs)), dim3(64 * 8),
                                   af_lds_bytes(a.T), s, a, B);
            else
                hipLaunchKernelGGL((psa_attention_full<T, AF_NW>), dim3((unsigned)(a.heads * B * qs)), dim3(64 * AF_NW),
                                   af_lds_bytes(a.T), s, a, B);
            return (int)hipGetLastError();
        }
        if (!tune.attn_lds) {
            const dim3 g((a.T + 63) / 64, a.heads, B);
            hipLaunchKernelGGL((psa_attention_mfma<T>), g, dim3(256), 0, s, a);
        } else {
            const unsigned g = (unsigned)((a.T + 16 * AT_NW - 1) / (16 * AT_NW) * a.heads * B);
            hipLaunchKernelGGL((psa_attention_lds<T>), dim3(g), dim3(64 * AT_NW), 0, s, a);
        }
        const long long n = (long long)B * a.T * (a.heads * DH / 8);
        hipLaunchKernelGGL((pe_add<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, B);
    } else {
        const dim3 g((a.T + ATT_Q - 1) / ATT_Q, a.heads, B);
        hipLaunchKernelGGL((psa_attention<T>), g, dim3(ATT_Q), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace

int launch_attention(int dtype, const AttnArgs& a, int B, const LaunchCtx& ctx, hipStream_t s) {
    switch (dtype) {
        case F32: return launch_attention_t<float>(a, B, ctx, s);
        case F16: return launch_attention_t<_Float16>(a, B, ctx, s);
        case BF16: return launch_attention_t<__bf16>(a, B, ctx, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace yh
