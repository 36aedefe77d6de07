// Fused C3k2 block (nets/nn.py:66-80, n = 1, csp = False) for the 16-bit handles.
//
// One persistent workgroup (CSP_THREADS / 64 waves) per CU walks TH x TW output tiles of the block:
//   P0  input tile with a 2-pixel halo -> LDS (LDS-DMA, zeros outside the image)
//   P1  conv1 1x1 Cin -> 2c + SiLU on the whole halo tile -> T1 = [a | b]; pixels
//       outside the image are zeroed (they are the next conv's zero padding)
//   P2  Residual conv1 3x3 c -> c/2 + SiLU on b, 1-pixel halo -> R1 (zeroed outside)
//   P3  Residual conv2 3x3 c/2 -> c + SiLU, + b (nn.py:49) -> C2
//   P4  conv2 1x1 over cat [a | b | C2] (3c) -> cout + SiLU -> the block output in HBM
// The packed weights (MFMA fragments in lane order, one 1 KB image per 32-cout tile and
// K step) and biases are copied to LDS once per workgroup; the next tile's input DMA
// runs during P2-P4.
//
// Nothing in the tile loop divides or builds a 64-bit address per lane: the DMA descriptors
// (which chunk of which halo pixel a lane loads) are computed once per kernel, the tile walk
// is (image, tile row, tile column) stepped with carries, a pixel's row is an exact
// multiply-shift (cs_index_ok), and the map is addressed through a wave-uniform base per tile
// plus a 32-bit lane offset (csp_span_ok).
//
// Bit-identical to the per-layer conv_mx launches (conv_mx.h): each conv walks its K
// as  for 16-channel block: for tap: one v_mfma_f32_32x32x16 step  (channels past a
// layer's width are zero), adds the bias, applies SiLU and rounds once; the residual
// is added to the rounded value in fp32 and rounded again (mx_epi).
//
// Fragment rows are permuted like conv_mx's packed weights: lane half hh of a 32-cout
// tile a holds couts 32a + 16hh .. +15 in its 16 accumulator registers, so every
// epilogue store is two 16-B chunks.
#include "common.h"
#include "mfma32.h"

namespace yh {

namespace {

constexpr int NWV = CSP_THREADS / 64;

// s_waitcnt vmcnt(N) for the largest encodable N <= n of {8, 4, 2, 0} (n wave-uniform)
__device__ __forceinline__ void cs_wait_vm(int n) {
    if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#ifdef YH_CSP_TRACE
// experiments only (-DYH_CSP_TRACE builds; the shipped library has none of this): wave 0 of
// every workgroup stamps s_memtime per tile, read back by yh_debug_csp_trace
// (tools/csp_trace.py). Slots: 0 tile top, 1 after the top wait, 2 after the top barrier,
// 3 / 4 wave 0 done with P1 / after P1's barrier (unset in tail mode), 5 / 6 the same for P2,
// 7 / 8 for P3, 9 wave 0 done with P4, 10 s_memrealtime at the tile top, 11 = TH | TW << 16 |
// (tile + 1) << 32. One record per (instantiation, workgroup, k-th tile of the workgroup).
constexpr int CS_TR = 12, CS_TR_TILES = 16, CS_TR_WG = 256, CS_TR_OPS = 4;
__device__ unsigned long long csp_trace_buf[CS_TR_OPS * CS_TR_WG * CS_TR_TILES * CS_TR];
#define CS_STAMP(k) do { if (trp) trp[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define CS_STAMP(k) do { } while (0)
#endif

// every LDS address of this file is a multiple of 16 (region offsets, pixel strides of
// 16 (2 n + 1) bytes, 16-byte channel groups): one ds_read_b128 / ds_write_b128 per access
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 cs_rd(unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    // one native 16-byte vector load: a uint4 (four scalars) is split by the optimiser and put
    // back together in 8-byte halves
    typedef __attribute__((address_space(3))) const u32x4* lp;
    const u32x4 v = *reinterpret_cast<lp>((size_t)addr);
    return make_uint4(v[0], v[1], v[2], v[3]);
#else
    (void)addr;
    return uint4{};
#endif
}
__device__ __forceinline__ void cs_wr(unsigned addr, uint4 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) u32x4* lp;
    *reinterpret_cast<lp>((size_t)addr) = u32x4{v.x, v.y, v.z, v.w};
#else
    (void)addr; (void)v;
#endif
}
// byte offset of pixel px at a pixel stride of S elements (S * 2 bytes, a multiple of 16): the
// shift keeps the multiple of 16 visible to the compiler, which the 24-bit multiply hides
template <int S>
__device__ __forceinline__ unsigned cs_px(unsigned px) {
    static_assert(S % 8 == 0, "pixel strides are whole 16-byte chunks");
    return __umul24(px, S / 8) << 4;
}
__device__ __forceinline__ float4 cs_rdf(unsigned addr) {
    const uint4 u = cs_rd(addr);
    return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
}

// Parameter image layout (bytes), shared with the host packer through csp_prm_bytes.
struct CsLayout {
    int w1, w2, w3, w4, b1, b2, b3, b4, prm;
};
__host__ __device__ constexpr CsLayout cs_layout(int ni, int nc, int no) {
    const int nh = (nc + 1) / 2, na3 = (nc + 1) / 2;
    CsLayout L{};
    L.w1 = 0;
    L.w2 = L.w1 + nc * ni * 1024;            // conv1: nc 32-cout tiles x ni steps
    L.w3 = L.w2 + 9 * nc * 1024;             // res conv1: one tile x 9 nc steps
    L.w4 = L.w3 + na3 * 9 * nh * 1024;       // res conv2: na3 tiles x 9 nh steps
    L.b1 = L.w4 + no * 3 * nc * 1024;        // conv2: no tiles x 3 nc steps
    L.b2 = L.b1 + 32 * nc * 4;
    L.b3 = L.b2 + 32 * 4;
    L.b4 = L.b3 + 32 * na3 * 4;
    L.prm = (L.b4 + 32 * no * 4 + 1023) & ~1023;
    return L;
}
struct CsTile {
    int lx, lt, lr, lc, total;
};
__host__ __device__ inline CsTile cs_tile(int TH, int TW, int ni, int nc, int no) {
    const int nh = (nc + 1) / 2;
    const CsLayout L = cs_layout(ni, nc, no);
    const int XP = (TH + 4) * (TW + 4), MP = (TH + 2) * (TW + 2), NP = TH * TW;
    CsTile t{};
    t.lx = L.prm;
    t.lt = t.lx + (ni ? ((XP * (16 * ni + 8) * 2 + 1023) & ~1023) : 0);   // tail mode: no X region
    t.lr = t.lt + XP * (32 * nc + 8) * 2;
    t.lc = t.lr + MP * (16 * nh + 8) * 2;
    t.total = t.lc + NP * (16 * nc + 8) * 2;
    return t;
}

// Index math of the kernel. px / width runs as hc_q24 at shift CS_DIV_S; a lane keeps the DMA
// descriptors of at most cs_maxr rounds of CSP_THREADS 16-B chunks in registers (the input
// region is at most (160 KB - parameters) / 2 whole-block, where T1 is as large again, and
// about three quarters of it in tail mode). cs_index_ok is the host proof for a tile: csp_lds
// offers no tile that fails it.
constexpr int CS_DIV_S = 20;
__host__ __device__ constexpr int cs_maxr(int ni) { return ni ? 4 : 6; }
inline bool cs_index_ok(int TH, int TW, int ni, int nc) {
    const long long XW = TW + 4, MW = TW + 2, XP = (TH + 4) * XW, MP = (TH + 2) * MW, NP = (long long)TH * TW;
    const long long chunks = XP * ((ni ? 2 * ni : 4 * nc) + 1);
    return TH + 4 < 0xffff && XW < 0xffff && chunks <= (long long)cs_maxr(ni) * CSP_THREADS &&
           hc_exact(XP - 1, XW, CS_DIV_S) && hc_exact(MP - 1, MW, CS_DIV_S) && hc_exact(NP - 1, TW, CS_DIV_S);
}

// 16 consecutive outputs of one pixel (couts co0 .. co0 + 15): bias, SiLU, one rounding
template <typename T>
__device__ __forceinline__ void cs_act(const f32x16& acc, unsigned bias_addr, uint4 (&o)[2]) {
    unsigned w[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b = cs_rdf(bias_addr + 16 * q);
        w[2 * q] = bias_act_pack2<T>(f32x2{acc[4 * q], acc[4 * q + 1]}, f32x2{b.x, b.y});
        w[2 * q + 1] = bias_act_pack2<T>(f32x2{acc[4 * q + 2], acc[4 * q + 3]}, f32x2{b.z, b.w});
    }
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// the residual add of 8 rounded outputs: the sums in fp32, rounded again (nn.py:49)
template <typename T>
__device__ __forceinline__ uint4 cs_addres(const uint4& o, const uint4& r) {
    return make_uint4(add_pack2<T>(o.x, r.x), add_pack2<T>(o.y, r.y), add_pack2<T>(o.z, r.z), add_pack2<T>(o.w, r.w));
}

// A 16-cout layer in a 32-cout tile leaves lane half 1 without outputs. Lane half 0's outputs
// 8 .. 15 move over to it (v_permlane32_swap: rows 2-3 of the first operand take rows 0-1 of the
// second), and every lane finishes 8 couts (8 hh .. 8 hh + 7) of its pixel as cs_act does, so the
// epilogue issues half the exp / rcp. Both lanes of a pixel must be active. bias_addr: cout 0.
template <typename T>
__device__ __forceinline__ uint4 cs_act_half(const f32x16& acc, unsigned bias_addr, int hh) {
#if defined(__HIP_DEVICE_COMPILE__)
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        v[e] = __uint_as_float(
            __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[e]), __float_as_uint(acc[8 + e]), false, false)[0]);
    const float4 b0 = cs_rdf(bias_addr + 32 * hh), b1 = cs_rdf(bias_addr + 32 * hh + 16);
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        // the products round to f32 before they round to T, as in cs_act and conv_mx: keep the
        // compiler from folding both into v_fma_mixlo_f16, which rounds once
        f32x2 p = silu2<T>(f32x2{v[i], v[i + 1]} + f32x2{bb[i], bb[i + 1]});
        asm("" : "+v"(p));
        w[i >> 1] = pack2<T>(p);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
#else
    (void)acc; (void)bias_addr; (void)hh;
    return uint4{};
#endif
}

// One conv phase: the NA x nb work items (32-cout A tile a, 32-pixel B tile) of an
// npx-pixel region go round-robin to the waves; a wave runs two items at once (two
// independent MFMA chains) while it has two. A image a = aimg + a * NK KB (fragments in lane
// order). A region pixel px is (row r, column cc) of a region RW pixels wide: r = px / RW by
// the exact multiply-shift dv (csp_lds admits only tiles for which it is exact), once per item.
// prep(px, r, cc) = the item's B base addresses (CsB), baddr(B, k) = LDS byte address of the
// lane's 8 K values of step k (a base + an offset that is constant once k is unrolled);
// epi(a, px, r, cc, acc) for pixels < npx. The first K step takes the MFMA's zero C operand.
struct CsB {
    unsigned b[3];
};
template <typename T, int NA, int NK, typename Prep, typename BAddr, typename Epi>
__device__ __forceinline__ void cs_phase(unsigned aimg, int npx, HcDiv dv, int RW, Prep prep, BAddr baddr, Epi epi) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l32 = lane & 31;
    const int items = NA * ((npx + 31) >> 5);
    f32x16 zero;
#pragma unroll
    for (int e = 0; e < 16; ++e) zero[e] = 0.f;
    for (int i0 = wv; i0 < items; i0 += 2 * NWV) {
        const int i1 = i0 + NWV;
        const int a0 = i0 % NA, a1 = i1 % NA;
        const int p0 = (i0 / NA) * 32 + l32, p1 = (i1 / NA) * 32 + l32;
        const int c0 = p0 < npx ? p0 : npx - 1, c1 = p1 < npx ? p1 : npx - 1;
        const int r0 = hc_q24(c0, dv), cc0 = c0 - (int)__umul24(r0, RW);
        const CsB B0 = prep(c0, r0, cc0);
        const unsigned ai0 = aimg + (unsigned)(a0 * NK * 1024 + lane * 16);
        if (i1 < items) {   // wave-uniform
            const int r1 = hc_q24(c1, dv), cc1 = c1 - (int)__umul24(r1, RW);
            const CsB B1 = prep(c1, r1, cc1);
            const unsigned ai1 = aimg + (unsigned)(a1 * NK * 1024 + lane * 16);
            f32x16 acc0, acc1;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const uint4 f0 = cs_rd(ai0 + k * 1024), f1 = NA > 1 ? cs_rd(ai1 + k * 1024) : f0;
                const uint4 x0 = cs_rd(baddr(B0, k)), x1 = cs_rd(baddr(B1, k));
                acc0 = Mfma32<T>::step(f0, x0, k ? acc0 : zero);
                acc1 = Mfma32<T>::step(f1, x1, k ? acc1 : zero);
            }
            if (p0 < npx) epi(a0, p0, r0, cc0, acc0);
            if (p1 < npx) epi(a1, p1, r1, cc1, acc1);
        } else {
            f32x16 acc0;
#pragma unroll
            for (int k = 0; k < NK; ++k)
                acc0 = Mfma32<T>::step(cs_rd(ai0 + k * 1024), cs_rd(baddr(B0, k)), k ? acc0 : zero);
            if (p0 < npx) epi(a0, p0, r0, cc0, acc0);
        }
    }
}

#ifdef YH_CSP_TRACE
constexpr int cs_trace_op(int ni, int, int no) { return ni == 2 ? 0 : ni == 4 ? 1 : no == 2 ? 2 : 3; }   // YH_CSP_LIST order
#endif

template <typename T, int NI, int NC, int NO>
__global__ __launch_bounds__(CSP_THREADS) void csp_fused(const CspArgs A) {
    constexpr int NH = (NC + 1) / 2, NA3 = (NC + 1) / 2;
    constexpr int SX = 16 * NI + 8, ST = 32 * NC + 8, SR = 16 * NH + 8, SC = 16 * NC + 8;
    constexpr CsLayout L = cs_layout(NI, NC, NO);
    extern __shared__ __attribute__((aligned(16))) char sm[];
    typedef __attribute__((address_space(3))) char* lds_c;
    const unsigned lds0 = (unsigned)(size_t)(lds_c)sm;
    const int TH = A.TH, TW = A.TW, XW = TW + 4, MW = TW + 2;
    const int XP = (TH + 4) * XW, MP = (TH + 2) * MW, NP = TH * TW;
    const CsTile G = cs_tile(TH, TW, NI, NC, NO);
    const unsigned LX = lds0 + G.lx, LT = lds0 + G.lt, LR = lds0 + G.lr, LC = lds0 + G.lc;
    const int lane = threadIdx.x & 63, hh = lane >> 5;
    const int wvu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const T* x = reinterpret_cast<const T*>(A.x);
    T* y = reinterpret_cast<T*>(A.y);

    // parameters: once per workgroup
    {
        const char* prm = reinterpret_cast<const char*>(A.prm);
        for (int i0 = wvu * 64; i0 < L.prm / 16; i0 += CSP_THREADS) glds16(prm + (size_t)(i0 + lane) * 16, lds0 + i0 * 16);
    }
    // tail mode (NI == 0): the block input is conv1's output [a | b] (2c channels, computed
    // by its own launch) and lands straight in T1; P1 is skipped
    constexpr bool TAIL = NI == 0;
    constexpr int NCH = TAIL ? 4 * NC : 2 * NI;   // 16-B data chunks per pixel
    constexpr int CPX = NCH + 1;                  // + one padding chunk per stored pixel
    const unsigned LD = TAIL ? LT : LX;
    // row = px / width of the three regions without a division (hc_q24; exact: csp_lds)
    const HcDiv dxw = hc_div(XW, CS_DIV_S), dmw = hc_div(MW, CS_DIV_S), dtw = hc_div(TW, CS_DIV_S);
    // Input DMA descriptors, once per kernel: 16-B chunk q = 1024 j + thread of the halo tile is
    // chunk c of halo pixel (r, cc) whatever the tile, so the lane keeps its byte offset from
    // the tile's origin pixel and r | cc << 16 (r = 0xffff for a pad chunk or one past the end,
    // which no row window contains). At most cs_maxr rounds: csp_lds.
    constexpr int MAXR = cs_maxr(NI);
    const int total = XP * CPX;
    unsigned d_off[MAXR], d_rc[MAXR];
#pragma unroll
    for (int j = 0; j < MAXR; ++j) {
        const int q = j * CSP_THREADS + (int)threadIdx.x;
        const int px = q / CPX, c = q - px * CPX;
        const int pc = px < XP ? px : XP - 1;
        const int r = hc_q24(pc, dxw), cc = pc - (int)__umul24(r, XW);
        d_rc[j] = q < total && c < NCH ? (unsigned)r | (unsigned)cc << 16 : 0xffffu;
        d_off[j] = (__umul24(__umul24(r, A.W) + cc, A.ldx) + c * 8) * 2u;
    }
    // (n, ty, tx): image, tile row, tile column. The in-image tests are two window compares
    // against wave-uniform bounds, the source a wave-uniform 64-bit base + the lane's offset.
    auto load_x = [&](int n, int ty, int tx) {
        const int h0 = ty * TH - 2, w0 = tx * TW - 2;
        const char* base = reinterpret_cast<const char*>(x + (((long long)n * A.H + h0) * A.W + w0) * A.ldx);
        const unsigned rlo = h0 < 0 ? -h0 : 0, clo = w0 < 0 ? -w0 : 0;
        const unsigned rn = min(TH + 4, A.H - h0) - rlo, cn = min(XW, A.W - w0) - clo;
#pragma unroll
        for (int j = 0; j < MAXR; ++j) {
            const int i0 = j * CSP_THREADS + wvu * 64;
            if (i0 < total) {   // wave-uniform
                const unsigned r = d_rc[j] & 0xffffu, cc = d_rc[j] >> 16;
                const bool ok = r - rlo < rn && cc - clo < cn;
                const void* src = ok ? (const void*)(base + d_off[j]) : A.zero;
                glds16(src, LD + i0 * 16);
            }
        }
    };
    // XCD-aware: the workgroups of one XCD take neighbouring tiles (overlapping halos, one L2)
    const int t0 = xcd_remap(blockIdx.x, gridDim.x);
    // the tile walk t0, t0 + grid, ... as (n, ty, tx) with carries instead of two divisions per
    // tile: one step is (gn, gty, gtx)
    const int NG = gridDim.x;
    const int gn = NG / A.tiles, gty = (NG - gn * A.tiles) / A.ntw, gtx = NG - gn * A.tiles - gty * A.ntw;
    int n = t0 / A.tiles, ty = (t0 - n * A.tiles) / A.ntw, tx = t0 - n * A.tiles - ty * A.ntw;
    if (t0 < A.ntiles) load_x(n, ty, tx);

    // The top-of-tile wait covers the wave's input DMAs only, not the output stores issued after
    // them: vector-memory operations retire in issue order, so vmcnt(N) is enough when at least N
    // operations follow the last DMA. Those are the previous tile's P4 stores, two per work item
    // of this wave (p4_stores) when that tile lay wholly inside the map; a clipped tile may skip
    // stores, so it counts as none. Tail mode issues its DMA after P4: nothing is younger.
    const int p4_items = NO * ((NP + 31) >> 5);
    const int p4_stores = wvu < p4_items ? 2 * ((p4_items - wvu + NWV - 1) / NWV) : 0;
    int young = 0;
#ifdef YH_CSP_TRACE
    int trk = 0;
#endif
    for (int t = t0; t < A.ntiles; t += NG) {
        const int h0 = ty * TH, w0 = tx * TW;
        // the next tile of this workgroup
        int nn = n + gn, nty = ty + gty, ntx = tx + gtx;
        if (ntx >= A.ntw) { ntx -= A.ntw; ++nty; }
        if (nty >= A.nth) { nty -= A.nth; ++nn; }
        // in-image windows of the three regions (rows / columns r with r - lo < n, unsigned) and
        // the output base of the tile's origin pixel: all wave-uniform
        const unsigned rlo2 = h0 < 2 ? 2 - h0 : 0, clo2 = w0 < 2 ? 2 - w0 : 0;
        const unsigned rn2 = min(TH + 4, A.H - h0 + 2) - rlo2, cn2 = min(XW, A.W - w0 + 2) - clo2;
        const unsigned rlo1 = h0 < 1 ? 1 : 0, clo1 = w0 < 1 ? 1 : 0;
        const unsigned rn1 = min(TH + 2, A.H - h0 + 1) - rlo1, cn1 = min(MW, A.W - w0 + 1) - clo1;
        const unsigned rn0 = min(TH, A.H - h0), cn0 = min(TW, A.W - w0);
        char* ybase = reinterpret_cast<char*>(y + (((long long)n * A.H + h0) * A.W + w0) * A.ldy);
#ifdef YH_CSP_TRACE
        unsigned long long* trp = nullptr;
        if (threadIdx.x == 0 && blockIdx.x < CS_TR_WG && trk < CS_TR_TILES) {
            trp = csp_trace_buf + ((size_t)(cs_trace_op(NI, NC, NO) * CS_TR_WG + blockIdx.x) * CS_TR_TILES + trk) * CS_TR;
            trp[10] = __builtin_amdgcn_s_memrealtime();
            trp[11] = (unsigned long long)TH | (unsigned long long)TW << 16 | (unsigned long long)(t + 1) << 32;
        }
        ++trk;
#endif
        CS_STAMP(0);
        cs_wait_vm(young);   // this wave's input DMAs of this tile have landed
        CS_STAMP(1);
        lds_barrier();
        CS_STAMP(2);

        // P1: conv1 over the halo tile, X -> T1 (zero outside the image)
        if constexpr (!TAIL) {
        cs_phase<T, NC, NI>(
                lds0 + L.w1, XP, dxw, XW,
                [&](int px, int, int) { return CsB{{LX + cs_px<SX>(px) + 16 * hh, 0, 0}}; },
                [&](const CsB& B, int k) { return B.b[0] + 32 * k; },
                [&](int a, int px, int r, int cc, const f32x16& acc) {
                    uint4 o[2];
                    cs_act<T>(acc, lds0 + L.b1 + (32 * a + 16 * hh) * 4, o);
                    if (!((unsigned)r - rlo2 < rn2 && (unsigned)cc - clo2 < cn2)) o[0] = o[1] = make_uint4(0, 0, 0, 0);
                    const unsigned d = LT + cs_px<ST>(px) + (32 * a + 16 * hh) * 2;
                    cs_wr(d, o[0]);
                    cs_wr(d + 16, o[1]);
                });
        CS_STAMP(3);
        lds_barrier();
        CS_STAMP(4);
        if (t + NG < A.ntiles) load_x(nn, nty, ntx);   // X is dead: next tile's input
        }

        // P2: Residual conv1 (3x3, b -> R1) over the 1-pixel halo region
        cs_phase<T, 1, 9 * NC>(
            lds0 + L.w2, MP, dmw, MW,
            [&](int, int r, int cc) {   // rows r, r + 1, r + 2 of T1 at column cc, the b half
                const unsigned b0 = LT + cs_px<ST>(__umul24(r, XW) + cc) + (16 * NC + 8 * hh) * 2;
                const unsigned rs = cs_px<ST>(XW);
                return CsB{{b0, b0 + rs, b0 + 2 * rs}};
            },
            [&](const CsB& B, int k) {
                const int cb = k / 9, tap = k - 9 * (k / 9), kh = tap / 3, kw = tap - 3 * (tap / 3);
                return B.b[kh] + (kw * ST + 16 * cb) * 2;
            },
            [&](int, int px, int r, int cc, const f32x16& acc) {
                const bool in = (unsigned)r - rlo1 < rn1 && (unsigned)cc - clo1 < cn1;
                if constexpr (NH == 1) {   // 16 couts: both lane halves share the epilogue
                    uint4 o = cs_act_half<T>(acc, lds0 + L.b2, hh);
                    if (!in) o = make_uint4(0, 0, 0, 0);
                    cs_wr(LR + cs_px<SR>(px) + 16 * hh, o);
                    return;
                }
                if (16 * hh >= 16 * NH) return;
                uint4 o[2];
                cs_act<T>(acc, lds0 + L.b2 + 16 * hh * 4, o);
                if (!in) o[0] = o[1] = make_uint4(0, 0, 0, 0);
                const unsigned d = LR + cs_px<SR>(px) + 32 * hh;
                cs_wr(d, o[0]);
                cs_wr(d + 16, o[1]);
            });
        CS_STAMP(5);
        lds_barrier();
        CS_STAMP(6);

        // P3: Residual conv2 (3x3, R1 -> C2) + b over the tile
        cs_phase<T, NA3, 9 * NH>(
                lds0 + L.w3, NP, dtw, TW,
                [&](int, int r, int cc) {   // rows r, r + 1, r + 2 of R1 at column cc
                    const unsigned b0 = LR + cs_px<SR>(__umul24(r, MW) + cc) + 16 * hh;
                    const unsigned rs = cs_px<SR>(MW);
                    return CsB{{b0, b0 + rs, b0 + 2 * rs}};
                },
                [&](const CsB& B, int k) {
                    const int cb = k / 9, tap = k - 9 * (k / 9), kh = tap / 3, kw = tap - 3 * (tap / 3);
                    return B.b[kh] + (kw * SR + 16 * cb) * 2;
                },
                [&](int a, int px, int r, int cc, const f32x16& acc) {
                    // the tile pixel's b in T1 (the residual)
                    const unsigned tb = LT + cs_px<ST>(__umul24(r + 2, XW) + cc + 2) + 32 * NC;
                    if constexpr (NC == 1) {   // 16 couts: both lane halves share the epilogue
                        const uint4 o = cs_act_half<T>(acc, lds0 + L.b3, hh);
                        const uint4 rv = cs_rd(tb + 16 * hh);
                        cs_wr(LC + cs_px<SC>(px) + 16 * hh, cs_addres<T>(o, rv));
                        return;
                    }
                    const int co = 32 * a + 16 * hh;
                    if (co >= 16 * NC) return;
                    uint4 o[2];
                    cs_act<T>(acc, lds0 + L.b3 + co * 4, o);
                    const unsigned rs = tb + co * 2;
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        o[hf] = cs_addres<T>(o[hf], cs_rd(rs + 16 * hf));
                    }
                    const unsigned d = LC + cs_px<SC>(px) + co * 2;
                    cs_wr(d, o[0]);
                    cs_wr(d + 16, o[1]);
                });
        CS_STAMP(7);
        lds_barrier();
        CS_STAMP(8);

        // P4: conv2 over cat [a | b | C2] -> block output
        cs_phase<T, NO, 3 * NC>(
                lds0 + L.w4, NP, dtw, TW,
                [&](int px, int r, int cc) {   // [a | b] of the tile pixel in T1, its C2
                    return CsB{{LT + cs_px<ST>(__umul24(r + 2, XW) + cc + 2) + 16 * hh,
                                LC + cs_px<SC>(px) + 16 * hh, 0}};
                },
                [&](const CsB& B, int k) { return k < 2 * NC ? B.b[0] + 32 * k : B.b[1] + 32 * (k - 2 * NC); },
                [&](int a, int, int r, int cc, const f32x16& acc) {
                    uint4 o[2];
                    const int co = 32 * a + 16 * hh;
                    cs_act<T>(acc, lds0 + L.b4 + co * 4, o);
                    if ((unsigned)r < rn0 && (unsigned)cc < cn0) {
                        // 32-bit byte offset from the tile's origin pixel (launch_csp_t checks the range)
                        const unsigned off = (__umul24(__umul24(r, A.W) + cc, A.ldy) + co) * 2u;
                        uint4* d = reinterpret_cast<uint4*>(ybase + off);
                        d[0] = o[0];
                        d[1] = o[1];
                    }
                });
        CS_STAMP(9);
        if constexpr (!TAIL) young = h0 + TH <= A.H && w0 + TW <= A.W ? p4_stores : 0;
        if constexpr (TAIL) {   // T1 is read until here: the next tile's input after a barrier
            lds_barrier();
            if (t + NG < A.ntiles) load_x(nn, nty, ntx);
        }
        n = nn;
        ty = nty;
        tx = ntx;
    }
    vm_wait<0>();
}

// instantiated (ni, nc, no): v11_n p2.1 (2, 1, 2), p3.1 and v11_s p2.1 (4, 2, 4); tail mode
// (ni = 0): v11_n fpn.h2 (0, 2, 2), p3.1 (0, 2, 4)
#define YH_CSP_LIST(X) X(2, 1, 2) X(4, 2, 4) X(0, 2, 2) X(0, 2, 4)

template <typename T>
int launch_csp_t(const CspArgs& a, int grid, hipStream_t s) {
    const int lds = csp_lds(a.TH, a.TW, a.ni, a.nc, a.no);
    if (lds == 0 || grid <= 0 || a.ldx % 8 || a.ldy % 8) return (int)hipErrorInvalidValue;
    // a lane's 32-bit byte offset from its tile's origin pixel (input halo rows, output rows)
    // goes through 24-bit multiplies: pixels of TH + 4 map rows below 2^24, bytes below 2^31
    if (!csp_span_ok(a.TH, a.TW, a.W, a.ldx, a.ldy) || a.nth * a.ntw != a.tiles) return (int)hipErrorInvalidValue;
#define YH_CSP_CASE(NI, NC, NO)                                                                              \
    if (a.ni == NI && a.nc == NC && a.no == NO) {                                                            \
        if (int rc = lds_optin(reinterpret_cast<const void*>(&csp_fused<T, NI, NC, NO>), 160 * 1024)) return rc; \
        hipLaunchKernelGGL((csp_fused<T, NI, NC, NO>), dim3((unsigned)grid), dim3(CSP_THREADS), lds, s, a); \
        return (int)hipGetLastError();                                                                       \
    }
    YH_CSP_LIST(YH_CSP_CASE)
#undef YH_CSP_CASE
    return (int)hipErrorInvalidValue;
}

}  // namespace

int csp_prm_bytes(int ni, int nc, int no) { return cs_layout(ni, nc, no).prm; }

void csp_offsets(int ni, int nc, int no, int (&off)[9]) {
    const CsLayout L = cs_layout(ni, nc, no);
    const int v[9] = {L.w1, L.w2, L.w3, L.w4, L.b1, L.b2, L.b3, L.b4, L.prm};
    for (int i = 0; i < 9; ++i) off[i] = v[i];
}

int csp_lds(int TH, int TW, int ni, int nc, int no) {
    bool inst = false;
#define YH_CSP_HAS(NI, NC, NO) inst = inst || (ni == NI && nc == NC && no == NO);
    YH_CSP_LIST(YH_CSP_HAS)
#undef YH_CSP_HAS
    if (!inst || TH < 1 || TW < 1 || TH > 4096 || TW > 4096) return 0;
    if (!cs_index_ok(TH, TW, ni, nc)) return 0;   // exact row / column quotients, descriptor rounds
    const int b = cs_tile(TH, TW, ni, nc, no).total;
    return b <= 160 * 1024 ? b : 0;
}

#ifdef YH_CSP_TRACE
extern "C" int yh_debug_csp_trace(unsigned long long* dst, int n) {
    if (n > CS_TR_OPS * CS_TR_WG * CS_TR_TILES * CS_TR) n = CS_TR_OPS * CS_TR_WG * CS_TR_TILES * CS_TR;
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(csp_trace_buf), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
}
#endif

int launch_csp(int dtype, const CspArgs& a, int grid, hipStream_t s) {
    switch (dtype) {
        case F16: return launch_csp_t<_Float16>(a, grid, s);
        case BF16: return launch_csp_t<__bf16>(a, grid, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace yh
