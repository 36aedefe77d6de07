// Shared device-side types and launcher declarations for the gfx950 YOLOv11 path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <set>
#include <utility>

#include "yolo_hip.h"   // yh_track_params (launch_track)

struct yh_motion_src;   // csrc/motion_host.h (launch_motion)

namespace yh {

enum DType { F32 = 0, F16 = 1, BF16 = 2 };
inline int dtype_size(int dt) { return dt == F32 ? 4 : 2; }

// Kernel-variant switches of one handle (Options::from_env fills them at yh_create; INTEGRATION.md
// lists the variables). Every variant of a kernel computes the same bits; 0 in a count or a tile
// field leaves the choice to the launcher.
struct Tuning {
    bool attn_full = true;   // whole-K/V attention kernel where it applies (else chunked + pe_add)
    bool attn_lds = true;    // chunked attention: the LDS kernel (else the per-wave one)
    int attn_nw = 0;         // whole-K/V attention: waves per workgroup, 8 or 16
    int attn_qs = 0;         //   and workgroups per (image, head)
    bool sppf_fused = true;  // one SPPF launch (else three maxpool5 launches)
    int sppf_cpw = 0;        // fused SPPF: 8-channel chunks per workgroup
    int sppf_xcd = 1;        //   and an image's workgroups on one XCD (0: hardware order)
    int c3k_bands = 0;       // fused C3k: first band count tried
    int c3k_nb = 0;          //   and an upper bound on its weight ring buffers
    int csp_th = 0, csp_tw = 0;   // fused C3k2: output tile, used where csp_lds admits it
    int boxdfl_tpw = 0;      // box_dfl: 32-pixel tiles per wave, 1, 2 or 4 (0: BOX_DFL_TPW)
    bool pwc_warm = true;    // pw_chain: L2 warm-up of the weights in the prologue
};
// what a launcher needs from its handle beside the kernel arguments
struct LaunchCtx {
    int num_cus;
    Tuning tune;
};

// Opt `kernel` in to `bytes` of dynamic LDS (above the 64 KB default) on the current device. The
// attribute is per device and a process may hold handles on several, driven from several threads:
// the pairs already set are kept under a lock. Returns the hipError_t, 0 once the pair is set.
inline int lds_optin(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return (int)e;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kernel})) return 0;
    if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) return (int)e;
    done.insert({dev, kernel});
    return 0;
}

// the sum of a 64-bit integer over the 64 lanes of a wave, in every lane (reid.hip, track.hip)
__device__ inline long long wave_sum(long long v) {
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)v, m);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), m);
        v += (long long)(((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// ACT_SILU_F64: SiLU of (K sum + bias) evaluated in fp64 and rounded once to fp32; only the fp32
// handle's classifier head conv (conv_gemm's EXACT instances), whose output is held to one ulp
enum Act { ACT_ID = 0, ACT_SILU = 1, ACT_SILU_F64 = 2 };

// floor(n / d) for a run-time divisor without a division: (n * m) >> s with
// m = floor(2^s / d) + 1. Exact for 0 <= n < 2^s / d while n * m < 2^32 (hc_exact is the host
// proof for a numerator range). hc_q24 is the same quotient through the 24-bit multiplier
// (full rate): n and m must be below 2^24 as well, which hc_exact(.., 20) implies for d >= 1.
struct HcDiv {
    unsigned m;
    int s;
};
__host__ __device__ __forceinline__ HcDiv hc_div(int d, int s) { return HcDiv{(1u << s) / (unsigned)d + 1u, s}; }
__host__ __device__ __forceinline__ int hc_q(int n, HcDiv f) { return (int)(((unsigned)n * f.m) >> f.s); }
__device__ __forceinline__ int hc_q24(int n, HcDiv f) { return (int)(__umul24((unsigned)n, f.m) >> f.s); }
// every hc_q / hc_q24 quotient n / d with 0 <= n <= nmax is exact at shift s (s <= 20 for hc_q24)
inline bool hc_exact(long long nmax, long long d, int s) {
    if (d < 1 || nmax < 0 || s > 24) return false;
    const long long m = (1ll << s) / d + 1;
    return nmax * d < (1ll << s) && nmax * m < (1ll << 32) && nmax < (1 << 24) && m < (1 << 24);
}

// Dense conv as an implicit GEMM over NHWC activations.
//   GEMM rows M  = batch * Ho * Wo (output pixels)
//   GEMM cols N  = Cout (physical, multiple of 8)
//   reduction K  = KH * KW * Cin (Cin physical, multiple of 8), packed weights
//                  are [Coutp][Kp] with k = (kh*KW + kw)*Cin + ci, zero padded.
// The input may be the channel-concatenation of two NHWC views ("segments");
// a segment may be read through a nearest x2 upsample (up = 1), which is how
// DarkFPN's up+cat (nets/nn.py:203-209) is fused into the consumer's loader.
struct ConvArgs {
    const void* in0; int ldc0, c0, up0, h0, w0;   // segment 0: channels [0, c0)
    const void* in1; int ldc1, c1, up1, h1, w1;   // segment 1: channels [c0, c0+c1)
    int Hi, Wi, Ho, Wo, stride, pad, KH, KW, Cin, K, Kp, M;
    const void* w;       // packed weights, handle dtype
    const float* bias;   // [Coutp] fp32
    const int* ktab;     // [Kp/8]: (kh<<24)|(kw<<16)|ci, ci=0xffff for padding
    void* out; int ldo;  // output view base (channel offset applied), pixel stride
    const void* res; int ldr;  // optional residual view added after the activation
    int Cout;            // physical output channels written (multiple of 8)
    int act;
    int gm, gn;          // tile grid
    const void* zero;    // >= 16 zero bytes in device memory (source of padded taps)
    int ks;              // > 1: K split over the workgroup's waves (conv_gemm2k), set by
                         //      the engine's shape rule for 16-bit handles
};

// First layer: 3-channel NCHW input (the caller's tensor), 3x3 stride-2 conv.
struct FirstConvArgs {
    const void* const* io;  // io[0] = x (NCHW), read at kernel start (graph-replay friendly)
    int H, W, Ho, Wo, Cout, ldo, M;
    const float* w;      // [Cout][27] fp32 (ci, kh, kw)
    const float* bias;   // [Cout]
    void* out;
    int act;
    int in_u8;           // 1: x is uint8 (the loader's image tensor); the kernel applies
                         //    main.py:265-267's `x.to(dtype) / 255` while staging it
};

// Stem + net.p2.0 fused (nets/nn.py:160-163): the stem output stays in LDS.
struct Stem2Args {
    const void* const* io;   // io[0] = x (NCHW, 3 channels; uint8 when in_u8)
    int H, W, Hs, Ws, Ho, Wo, B;
    const float* b1;         // stem bias [c1 padded] fp32
    int c1, c2;              // stem couts, p2.0 couts
    const void* prm;         // p2.0 fragments (c2/32 tiles x 9*c1/16 steps x 1 KB, MFMA lane order) + fp32 bias
    int prm_bias;            // byte offset of the bias in prm
    int prm_stem;            // byte offset of the stem's own fragments in prm: c1/16 tiles x 1 KB,
                             // lane (fr, g) holds cout 16 i + fr, k = 8 g .. 8 g + 7 (zero for k >= 27)
    void* out; int ldo;      // p2.0 output view
    int in_u8;
    int ntw, nth;            // tiles per row / per column (stem2_tiles)
};
bool stem2_ok(int c1, int c2);
bool stem2_size_ok(int H, int W);   // the staging's 32-bit per-lane offsets cover one H x W image
void stem2_tiles(int Ho, int Wo, int& ntw, int& nth);
int launch_stem2(int dtype, const Stem2Args& a, hipStream_t s);

// Depthwise 3x3 stride-1 conv on an NHWC view.
struct DwArgs {
    const void* in; int ldi;
    int H, W, C, M;
    const float* w;      // [9][C] fp32
    const float* bias;   // [C]
    void* out; int ldo;
    int act;
};

// SPPF: y1 = mp5(x), y2 = mp5(y1), y3 = mp5(y2) (nets/nn.py:90-94) from slice 0
// of a 4-slice concat buffer into slices 1..3.
struct PoolArgs {
    void* buf; int ldc, C, H, W, B;
};

// C2PSA attention (nets/nn.py:111-123) with the positional depthwise conv fused:
// out[:, h*dh + d] = softmax(q^T k * scale) v  +  pe(v)
struct AttnArgs {
    const void* qkv; int ldq;   // per head: [q(dk) | k(dk) | v(dh)]
    int T, Hs, Ws, heads, dk, dh;
    float scale;
    const float* pe_w;   // [9][heads*dh]
    const float* pe_b;   // [heads*dh]
    void* out; int ldo;
};

// Detect-head decode (nets/nn.py:255-270, DFL 222-225, make_anchors util.py:85-96).
struct DecodeArgs {
    const void* lvl[3]; int ldc; int H[3], W[3]; float stride[3];
    int nc, A, B;
    const void* const* io;  // io[1] = y (B, 4+nc, A)
    int a_lo;               // first anchor decoded (anchors [a_lo, A))
    int box;                // 0: class rows only (the box rows come from box_dfl)
};

// NMS (utils/util.py:123-169)
constexpr int NMS_MAX_DET = 1024;    // most rows an image keeps (the kept set lives in LDS)
constexpr int NMS_PAIR_BITS = 26;    // anchors * classes < 2^26 (the pair index in a sort key's low bits)
struct NmsArgs {
    const void* y; int B, A, nc;
    float conf;          // threshold, already rounded to the input dtype
    float iou;           // largest float <= iou threshold (so ovr > iou  <=>  ovr > thr)
    float max_wh;
    int max_det, max_nms;
    // counts, hist, state, gkeys, ents and mask are the workspace (nms_workspace_bytes), filled
    // by nms_workspace_bind: nms.hip owns the layout
    int* counts;               // [B] candidate counts (zeroed by nms_zero)
    unsigned* hist;            // [B][2048] coarse score-bin histogram (zeroed by nms_zero)
    int bin_base;              // (fp32 bits >> 16) of the lowest bin
    float* dets; int* ndet;
    // first-batch scratch of the split greedy (nms.hip): per image a state record, the
    // decoded entries in score order and the lower-triangular IoU bitmask
    unsigned long long* state;  // [B][8]
    unsigned long long* gkeys;  // [B][4096]: the first batch's keys (unordered)
    float* ents;                // [B][3][4096][4]: offset box, plain box, (area, score, class, -)
    unsigned long long* mask;   // [B][64 * 64 * 65 / 2] words
#ifdef YH_ABLATION
    unsigned long long* trace;  // diagnostic builds only: [B][16] phase timestamps (nms.hip TraceSlot)
#endif
};
// bytes of the workspace for a batch of B images; the six workspace pointers of a (a.B set) into base
size_t nms_workspace_bytes(int B);
void nms_workspace_bind(NmsArgs& a, void* base);

// Fused cls branch of the detect head (nets/nn.py:244-252), one launch for all levels:
//   DWConv 3x3 + SiLU -> Conv 1x1 + SiLU -> DWConv 3x3 + SiLU -> Conv 1x1 + SiLU
//   -> Conv2d 1x1 (+ bias)
// per TH x TW output tile, every intermediate in LDS (halo recomputed), bit-identical
// to the five separate launches (same per-channel FMA order, same MFMA K order, one
// rounding to the handle dtype per layer output).
struct HeadClsLevel {
    const void* x; int ldx, C0;      // level input (NHWC view), channels
    int H, W;
    void* y; int ldy;                // output view (the head tensor's cls slice)
    int aoff;                        // direct mode: the level's first anchor
    const float* dw1w; const float* dw1b; int dw1ld;   // [9][dw1ld] fp32, bias
    const void* pw1w; int pw1ld; const float* pw1b;    // [rows][pw1ld] dtype, bias
    const float* dw2w; const float* dw2b; int dw2ld;
    const void* pw2w; int pw2ld; const float* pw2b;
    const void* pw3w; int pw3ld; const float* pw3b;
    int TH, TW, ntw, tiles;          // output tile, tiles per row, tiles per image
    int wg0;                         // first workgroup of the level (one workgroup per tile)
};
struct HeadClsArgs {
    HeadClsLevel lv[3];
    int nlv, B, c3, nc;
    const void* zero;                // >= 16 zero bytes (source of out-of-image / padding chunks)
    // direct mode (io != nullptr): pw3's logits leave as sigmoid scores in rows 4.. of the
    // caller's y = io[1] (B, 4+nc, A) instead of the head tensor (the decode's class part)
    const void* const* io; int A;
};
#ifndef YH_HEAD_CLS_THREADS
#define YH_HEAD_CLS_THREADS 512
#endif
// 8-wave workgroups, two per CU (16 waves); 256 = the round-2 4-wave kernel (fragments
// preloaded a phase ahead), 7 % slower (profiles/r03_ops_hcls_{256,512}.txt)
constexpr int HEAD_CLS_THREADS = YH_HEAD_CLS_THREADS;
#ifndef YH_HEAD_CLS_LDS_KB
#define YH_HEAD_CLS_LDS_KB 80
#endif
constexpr int HEAD_CLS_LDS = YH_HEAD_CLS_LDS_KB * 1024;   // 80: two workgroups (16 waves) per CU, 8x16 tiles at 80x80
// LDS bytes of a tile's buffers; 0 if it does not fit
int head_cls_lds(int TH, int TW, int C0, int c3, int nc);
int launch_head_cls(int dtype, const HeadClsArgs& a, hipStream_t s);

// Fused C3k block (c3k.hip; nets/nn.py:52-63 CSPModule(c, c), c = 2 hh, two Residual(hh,
// e=1.0), hh = 32 or 64): every intermediate of a band of rows (+ the 4-row halo of the four
// 3x3 convs) in one workgroup's LDS. Maps whose bands of >= 4 rows keep <= 512 pixels (v11_n's
// 40x40 hh = 32 and 20x20 hh = 64 blocks at 640 x 640); bit-identical to the seven
// per-layer launches.
struct C3kArgs {
    const void* x; int ldx;          // block input (NHWC view, c channels)
    void* y; int ldy;                // block output view (c channels)
    int B, H, W;
    const void* prm;                 // packed parameters (c3k_offsets)
    int hh;                          // hidden channels (32 or 64)
    int bands;                       // row bands per image (set by launch_c3k: c3k_bands)
    int nbuf;                        // weight ring buffers (set by launch_c3k)
    unsigned long long* trace;       // micro benchmark builds (YH_ABLATION): per-workgroup stamps
};
int c3k_prm_bytes(int hh);
void c3k_offsets(int hh, int (&off)[9]);   // w1, w2, residual convs, w3, b1, b2, residual biases, b3, total
int c3k_lds(int H, int W, int hh);   // 0: no band split fits
// row bands per image (one workgroup each); first > 0: the band count tried first (Tuning::c3k_bands)
int c3k_bands(int B, int H, int W, int hh, int first);
int c3k_region_px(int H, int W, int bands);   // LDS pixels of a band's region (band + 4-row halo)
int launch_c3k(int dtype, const C3kArgs& a, const LaunchCtx& ctx, hipStream_t s);

// Box tail of the detect head, one launch for all levels: the last box conv (Conv2d 1x1
// + bias, nets/nn.py:241) with DFL (nn.py:222-225), make_anchors (utils/util.py:85-96) and
// dist2bbox (nn.py:264-268) in its epilogue, writing rows 0..3 of y = io[1]. Bit-identical
// to the conv launch + head_decode (same MFMA K order, logits rounded to the dtype first).
struct BoxDflLevel {
    const void* x; int ldx;          // box.l.1 output (NHWC), K = 16 * nk channels
    int H, W; float stride; int aoff;
    const void* w; int wld; const float* b;   // [64][wld] dtype weights, fp32 bias
    int wg0;                         // first workgroup of the level
};
struct BoxDflArgs {
    BoxDflLevel lv[3];
    int nlv, B, nk, nc, A;
    const void* const* io;
    int tpw;   // 32-pixel tiles per wave: 1, 2 or 4 (wg0 offsets are computed with it)
};
// Fused C3k2 block with one Residual bottleneck (nets/nn.py:66-80 with n = 1 and
// csp = False; Residual nn.py:42-49): conv1 1x1 (Cin -> 2c) -> split [a | b] ->
// b + conv3x3(conv3x3(b)) (c -> c/2 -> c) -> cat [a | b | r] -> conv2 1x1 (3c -> cout),
// every Conv with SiLU. A persistent workgroup walks TH x TW output tiles; the input tile
// (2-pixel halo) and every intermediate stay in LDS, the packed weights too. Bit-identical
// to the four conv_mx launches (same K order, one rounding per layer output, the residual
// added after the rounding and rounded again).
struct CspArgs {
    const void* x; int ldx;          // block input (NHWC view), Cin = 16 * ni channels
    void* y; int ldy;                // block output view, cout = 32 * no channels
    int H, W, B;
    const void* prm;                 // packed weight fragments + fp32 biases (csp_prm_bytes)
    int ni, nc, no;                  // Cin / 16, c / 16, cout / 32
    int TH, TW, ntw, tiles, ntiles;  // output tile, tiles per row / per image / in total
    int nth;                         // tile rows per image (tiles = ntw * nth)
    const void* zero;                // >= 16 zero bytes
};
#ifndef YH_CSP_THREADS
#define YH_CSP_THREADS 1024
#endif
constexpr int CSP_THREADS = YH_CSP_THREADS;
// bytes of the packed parameter image (weight fragments in MFMA lane order + biases)
int csp_prm_bytes(int ni, int nc, int no);
// byte offsets of the parameter image: w1, w2, w3, w4 (fragments), b1, b2, b3, b4 (fp32), total
void csp_offsets(int ni, int nc, int no, int (&off)[9]);
// LDS bytes for a TH x TW tile, 0 if it does not fit or (ni, nc, no) is not instantiated
int csp_lds(int TH, int TW, int ni, int nc, int no);
int launch_csp(int dtype, const CspArgs& a, int grid, hipStream_t s);
// The kernel addresses the map through a wave-uniform 64-bit base per tile (its origin pixel)
// and a 32-bit byte offset per lane that spans the tile's TH + 4 halo rows of the map. The
// offset is built with 24-bit multiplies: the pixel offset and the pixel strides stay below
// 2^24 and the byte offset below 2^31, whatever the map's height and the batch.
inline bool csp_span_ok(int TH, int TW, int W, int ldx, int ldy) {
    const long long px = (long long)(TH + 4) * W + TW + 4, ld = ldx > ldy ? ldx : ldy;
    return W > 0 && ld > 0 && W < (1 << 24) && ld < (1 << 24) && px < (1 << 24) && (px * ld + ld) * 2 < (1ll << 31);
}

constexpr int BOX_DFL_TPW = 2;       // 32-pixel tiles per wave (4 waves per workgroup; Tuning::boxdfl_tpw: 1 / 2 / 4)
int launch_box_dfl(int dtype, const BoxDflArgs& a, hipStream_t s);

// Pointwise chain (pwchain.hip): consecutive 1x1 convs of one map as one launch. A workgroup
// owns P consecutive pixels (flattened n, h, w) and runs the stages in order; a stage's input
// channels come in runs of whole 128-channel pieces, each from the LDS copy of an earlier
// stage's output or from a global view loaded into LDS in the prologue.
constexpr int PWC_THREADS = 512;
constexpr int PWC_MAX_STAGES = 6, PWC_MAX_RUNS = 4, PWC_MAX_LOADS = 6;
struct PwcRun {
    int lds;   // LDS byte offset of the run's first channel at pixel 0
    int ld;    // pixel stride of that LDS region (elements)
    int nkb;   // 16-channel blocks (a multiple of 8)
};
struct PwcStage {
    int K, N, act, nrun;
    PwcRun run[PWC_MAX_RUNS];
    const void* w; int wld;            // 16-bit weights in A-fragment order: fragment (a, kb) = 1 KB at
                                       // (a * (wld / 16) + kb) KB, lane-major (engine upload "pwfrag")
    const float* bias;                 // >= N floats
    int res_lds, res_ldl;              // residual in LDS (byte offset of channel 0, stride) or -1; a
                                       // residual no stage of the chain writes comes by the prologue
    void* out; int ldo;                // global output view (channel 0) and pixel stride
    int out_lds, out_ldl;              // LDS copy of the output (byte offset, stride) or -1
};
struct PwcLoad {
    const void* g; int ldg;            // global view (channel 0) and pixel stride (elements)
    int lds;                           // LDS byte offset; pixel stride nchunk + 1 16-B chunks
    int nchunk;                        // 16-B chunks (8 channels) per pixel
};
struct PwChainArgs {
    long long M;                       // pixels of the map (B * H * W)
    int P, nst, nload;
    int sink;                          // LDS byte offset of a scratch KB (weight warm-up DMAs)
    PwcStage st[PWC_MAX_STAGES];
    PwcLoad ld[PWC_MAX_LOADS];
    const void* zero;                  // >= 16 zero bytes
};
int launch_pw_chain(int dtype, const PwChainArgs& a, int lds, hipStream_t s);

// Classifier head (cls.hip; nets/nn.py Classify): 1x1 conv to CLS_EMBED channels + SiLU, the
// per-image mean over pixels, the linear layer and the softmax. Summation order of the mean
// (include/yolo_hip.h, "classifier arithmetic"): one fp32 chain per (image, channel) from zero over
// the image's pixels in ascending row-major order, then one multiplication by (float)(1.0 / HW).
constexpr int CLS_EMBED = 1280;
constexpr int CLS_THREADS = 256;                          // cls_head: 4 waves
constexpr int CLS_SCR_BYTES = 4 * 32 * 33 * 4;            // cls_head: per wave a 32 x 32 fp32 tile, rows padded
constexpr int CLS_FC_TB = 8, CLS_FC_TN = 64;              // cls_fc: images x classes per workgroup
// cls_pool: a (B, HW, C) in the handle dtype -> e (B, C) fp32
struct ClsPoolArgs {
    const void* a; int lda;
    int B, HW, C;
    float inv;           // (float)(1.0 / HW)
    float* e;
};
// cls_head: x (B, HW, K) -> e (B, N) without the (B, HW, N) activations in between. A workgroup owns
// G consecutive images (G * HW <= 128 pixels, a function of HW and K only) and all N channels.
struct ClsHeadArgs {
    const void* x; int ldx;
    int B, HW, K, N, G;
    const void* w; int wld;   // 16-bit weights in A-fragment order (engine upload "pwfrag")
    const float* bias;
    int act;
    float inv;
    float* e;
};
// pixels one cls_head workgroup can hold (0: K has no kernel), images per workgroup, LDS bytes
inline int cls_head_pmax(int K) {
    if (K < 128 || K % 128) return 0;
    for (int p : {128, 64, 32})
        if (p * (K + 8) * 2 + CLS_SCR_BYTES <= 160 * 1024) return p;
    return 0;
}
inline int cls_head_group(int K, int HW) {
    const int pm = cls_head_pmax(K);
    return HW > 0 && HW <= pm ? pm / HW : 0;
}
inline int cls_head_lds(int K, int HW) {
    const int g = cls_head_group(K, HW);
    return g ? (g * HW + 31) / 32 * 32 * (K + 8) * 2 + CLS_SCR_BYTES : 0;
}
// cls_fc: z = W e + b (fp32 accumulation, W in the handle dtype), then per row the softmax, the
// count mask and the copies to the caller's probs / logits / embed (io[2..4], count io[5])
struct ClsFcArgs {
    const float* e;
    const void* w; int wld;   // [>= nc rows][wld] handle dtype
    const float* bias;
    int B, nc, K;
    float* z; int ldz;
    const void* const* io;
};
int launch_cls_pool(int dtype, const ClsPoolArgs& a, hipStream_t s);
int launch_cls_head(int dtype, const ClsHeadArgs& a, hipStream_t s);
int launch_cls_fc(int dtype, const ClsFcArgs& a, hipStream_t s);
int launch_set_io_cls(void** io, const void* x, float* probs, float* logits, float* embed, const int* count,
                      hipStream_t s);

// launchers (return hipError_t as int)
int launch_conv(int dtype, int BM, int BN, const ConvArgs& a, hipStream_t s);   // fp32 handle only (conv.hip)
int launch_first_conv(int dtype, const FirstConvArgs& a, int B, hipStream_t s);
int launch_dwconv(int dtype, const DwArgs& a, hipStream_t s);
// silu<T> against silu2<T> over n floats (yh_debug_silu_pairs; the 16-bit dtypes only)
int launch_silu_pairs(int dtype, const float* x, unsigned* ys, unsigned* yp, size_t n, hipStream_t s);
int launch_sppf(int dtype, const PoolArgs& a, const LaunchCtx& ctx, hipStream_t s);
int launch_attention(int dtype, const AttnArgs& a, int B, const LaunchCtx& ctx, hipStream_t s);
int launch_decode(int dtype, const DecodeArgs& a, hipStream_t s);
int launch_set_io(void** io, const void* x, void* y, hipStream_t s);
int launch_nms(int dtype, const NmsArgs& a, hipStream_t s);
// match.hip: detections x labels -> true-positive bytes for a whole batch (yh_match)
int launch_match(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                 const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                 int* counts_out, hipStream_t s);
// merge.hip: tile detections -> source-coordinate detections, duplicates across tiles removed (yh_merge)
int launch_merge(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
                 const int* tile_offsets, const float* image_wh, int images, int max_tiles, double iou_threshold,
                 int max_out, float* out, int* out_counts, hipStream_t s);
// track.hip: one frame of every stream of a batch through its track table (yh_track); p by value;
// optimal: the associations solve an assignment instead of walking greedily (yh_track2)
int launch_track(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                 int streams, int max_tracks, const yh_track_params& p, int max_out, float* out, int* ids,
                 int* det_index, int* out_counts, bool optimal, hipStream_t s);
// the same with the appearance term (yh_track_reid): the state carries the galleries, the
// workspace the rows' features, their flags and the similarities (csrc/track_host.h's layout)
struct TrackReid {
    const int8_t* q;    // (batch, max_det, dim)
    const int* flags;   // (batch, max_det)
    const int* sim;     // (batch, max_tracks, max_det)
    const int* sim_t;   // (batch, max_det, max_tracks): the same numbers, transposed
    const int* gnz;     // (batch, max_tracks): the slot's gallery row is non-zero; NULL without features
    int* code;          // (batch, max_tracks): the gallery's work, for launch_gallery_update
    int dim;
    float cos_min, iou_min;
};
int launch_track_reid(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                      int streams, int max_tracks, const yh_track_params& p, int max_out, float* out, int* ids,
                      int* det_index, int* out_counts, const TrackReid& rd, bool optimal, hipStream_t s);
// track.hip: yh_track_warp, a motion (s, tx, ty) per batch row applied to the stream's live slots
int launch_track_warp(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                      const int* stream_ids, int batch, hipStream_t s);
// motion.hip: yh_motion, a thumbnail launch and a search launch per 32 frames; src from
// csrc/motion_host.h's yh_motion_check
int launch_motion(const ::yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                  int thumb_h, int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, hipStream_t s);
// assign.hip: yh_assign, one wave per problem; the tracker's `optimal` instances above run the same solver
int launch_assign(const int* weights, int problems, int T, int D, const int* t_counts, const int* d_counts,
                  int* row_of_slot, int* slot_of_row, hipStream_t s);
// reid.hip: yh_embed_quantize, the quantise-and-scatter of yh_track_reid, yh_embed_similarity
int launch_embed_quantize(const float* e, int rows, int dim, const int* count, int8_t* q, hipStream_t s);
int launch_embed_scatter(const float* embed, int capacity, int dim, const int* counts, const int* feat_counts,
                         const int* embed_total, int batch, int max_det, int8_t* q, int* flags, hipStream_t s);
int launch_embed_similarity(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                            int batch, int ra, int rb, int dim, int32_t* out, int* a_nonzero, int32_t* out_t,
                            hipStream_t s);
int launch_gallery_update(void* state, size_t stream_bytes, size_t gallery_offset, const int* stream_ids, int batch,
                          int max_tracks, int max_det, int dim, const int8_t* q, const int* flags, const int* code,
                          hipStream_t s);
// gallery.hip: yh_gallery_search (the chunks' k best into the workspace, then their merge) and
// yh_gallery_enrol; the chunking and the workspace layout are csrc/gallery_host.h's
int launch_gallery_search(const int8_t* gallery, const int* labels, const int* size, int capacity, int dim,
                          const int8_t* q, int nq, const int* nq_count, int k, int chunk_rows, int32_t* scores,
                          int32_t* index, void* workspace, hipStream_t s);
int launch_gallery_enrol(int8_t* gallery, int* labels, int* size, int capacity, int dim, const int8_t* q, int nq,
                         const int* nq_count, const int* take, const int* labels_in, int* next_label, int* rows_out,
                         hipStream_t s);

}  // namespace yh
