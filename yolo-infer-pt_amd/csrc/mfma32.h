// Device primitives shared by the kernels on v_mfma_f32_32x32x16 (conv_mx, conv_rw, c3k2, c3k,
// pwchain, head, cls, the stem): the MFMA step, the LDS-DMA copy, the LDS-only barrier, the
// counted vmcnt wait, the 16-byte LDS read, the rounding of two floats to T and FastDiv's
// evaluation, each written once. The fused kernels are bit-identical to the per-layer conv_mx
// launches because they round through the same pack2 and step through the same Mfma32.
#pragma once
#include "conv_mx.h"   // FastDiv
#include "dtypes.h"

namespace yh {

typedef __attribute__((ext_vector_type(16))) float f32x16;

// One 32(rows) x 32(cols) x 16(k) MFMA step: a / b are a lane's 8 consecutive k values of its row
// (A) / column (B), c the lane's 16 accumulators.
template <typename T> struct Mfma32;
template <> struct Mfma32<__bf16> {
    static __device__ __forceinline__ f32x16 step(const uint4& a, const uint4& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                       0, 0);
    }
};
template <> struct Mfma32<_Float16> {
    static __device__ __forceinline__ f32x16 step(const uint4& a, const uint4& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                      0);
    }
};

// LDS-DMA: the wave's 64 lanes each copy 16 B from their own global address `src` into LDS at
// lds_addr + 16 * lane. lds_addr is wave-uniform; it goes through M0, which is saved and restored
// inside the statement. The copy is hidden from the compiler's waitcnt pass: it counts in vmcnt
// like any global load, but the compiler puts no wait before a read of the destination. The
// caller owns the ordering: its own counted vm_wait<N>() for the wave's copies, then a barrier
// (lds_barrier) before other waves read them.
__device__ __forceinline__ void glds16(const void* src, unsigned lds_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_addr) : "memory");
#else
    (void)src; (void)lds_addr;
#endif
}

// s_waitcnt vmcnt(N): at most N of the wave's global loads, stores and LDS-DMA copies in flight
template <int N>
__device__ __forceinline__ void vm_wait() {
    static_assert(N >= 0 && N <= 63, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// Workgroup barrier for LDS hand-offs only: __syncthreads() also waits for every global
// load in flight (vmcnt(0)), which would drain the loads and LDS-DMA copies issued ahead of a
// phase. Two spellings, the same two instructions: in lds_barrier (c3k2, c3k, pwchain, head) the
// pair is one statement and stays together; in lds_barrier_sched (conv_mx, conv_rw) the compiler
// sees the barrier and schedules scalar work between the wait and it. Swapping either way moved
// those instructions and changed the code length of the kernels by 24 to 48 bytes, so each
// kernel keeps the spelling it was tuned with.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void lds_barrier_sched() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// 16 bytes of LDS at byte address addr (a multiple of 16): one ds_read_b128
__device__ __forceinline__ uint4 lds_rd16(unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) const uint4* lp;
    return *reinterpret_cast<lp>((size_t)addr);
#else
    (void)addr;
    return uint4{};
#endif
}

// Two floats rounded to T, a in the low half: the rounding of every conv output, per-layer
// (conv_mx's and conv_rw's epilogues) or fused. lo16 / hi16 give the halves back as floats.
template <typename T> struct Pk2;
template <> struct Pk2<__bf16> { typedef __attribute__((ext_vector_type(2))) __bf16 v2; };
template <> struct Pk2<_Float16> { typedef __attribute__((ext_vector_type(2))) _Float16 v2; };
template <typename T>
__device__ __forceinline__ unsigned pack2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, typename Pk2<T>::v2));
}
template <typename T>
__device__ __forceinline__ unsigned pack2(f32x2 v) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, typename Pk2<T>::v2));
}
template <typename T>
__device__ __forceinline__ float lo16(unsigned u) { return (float)__builtin_bit_cast(T, (unsigned short)(u & 0xffffu)); }
template <typename T>
__device__ __forceinline__ float hi16(unsigned u) { return (float)__builtin_bit_cast(T, (unsigned short)(u >> 16)); }

template <typename T>
__device__ __forceinline__ f32x2 lohi16(unsigned u) { return f32x2{lo16<T>(u), hi16<T>(u)}; }

// The epilogue of two adjacent outputs on one register pair: bias add, SiLU (silu2) where the
// layer has one, one rounding to T. acc / bias: the two accumulators and their biases.
template <typename T, bool SILU = true>
__device__ __forceinline__ unsigned bias_act_pack2(f32x2 acc, f32x2 bias) {
    const f32x2 v = acc + bias;
    if constexpr (SILU) return pack2<T>(silu2<T>(v));
    else return pack2<T>(v);
}
// the same with the activation chosen at run time: a select, not a branch
template <typename T>
__device__ __forceinline__ unsigned bias_act_pack2(f32x2 acc, f32x2 bias, bool silu_act) {
    const f32x2 v = acc + bias, s = silu2<T>(v);
    return pack2<T>(silu_act ? s : v);
}
// Residual add of two rounded outputs: pack2(lo16(w) + lo16(r), hi16(w) + hi16(r)), the sum in fp32
template <typename T>
__device__ __forceinline__ unsigned add_pack2(unsigned w, unsigned r) { return pack2<T>(lohi16<T>(w) + lohi16<T>(r)); }

// x / d for the divisor behind d (make_fastdiv)
__device__ __forceinline__ uint32_t fast_div(uint32_t x, FastDiv d) {
    return (uint32_t)(((uint64_t)__umulhi(x, d.m) + x) >> d.s);
}

}  // namespace yh
