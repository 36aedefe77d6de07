// Camera-motion estimate (yh_motion): the translation between a stream's previous and current frame,
// from block matching on luma thumbnails. The semantics are stated in include/yolo_hip.h; the host
// twin is csrc/motion_host.cpp, and the state layout and the arithmetic are shared with it through
// csrc/motion_host.h. Everything but the last few fp32 operations is integer arithmetic, so no
// summation order needs fixing. Two launches per YH_MOTION_LAUNCH frames, no atomics:
//
// motion_thumb   grid (thumb_h * chunks, frames): a workgroup of 256 threads makes one row of a
//                frame's thumbnail (one chunk of it for frames wider than MT_COLS). A thread owns 8
//                consecutive source pixels - one 8-byte load of an NV12 row, three of a BGR row, byte
//                loads where the row is not 8-byte aligned or the frame ends - and adds their lumas
//                down the thumbnail row's source rows in registers; the 8 column sums go to LDS, and
//                after a barrier thread j sums the columns of thumbnail pixel j. Every source luma byte
//                is read once. The thumbnail goes to the row's staging slot in the state: the stream's
//                own block still holds the previous thumbnail, which the search needs.
// motion_search  one workgroup of 1024 threads per batch row. Both thumbnails go to LDS with a row
//                pitch of thumb_w + 4, the current one shifted so that column R is dword aligned. A
//                wave takes a work item (dy, c): the four candidates whose previous-frame column
//                offset R - dx is 4 c + 0 .. 3. Its lanes walk the window's dwords: one aligned dword of
//                the current row, two of the previous row, four v_alignbyte_b32 to cut the four shifted
//                dwords out of the pair and four v_sad_u8 (4 bytes each) - 3 LDS reads per 16 byte
//                differences, no byte loads. The lanes' sums are added with lane exchanges into the SAD
//                table in LDS. Then every thread folds its share of the table into the smallest key
//                (SAD, |dy| + |dx|, dy, dx) - a total order, so the spread over lanes and waves cannot
//                matter -, thread 0 refines and writes the row's outputs, and all threads store the
//                current thumbnail and the header into the stream's block.
// Built with -ffp-contract=off: the refinement must round exactly as in the host twin.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "motion_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_PX = 8;          // source pixels per thread and pass
constexpr int MT_COLS = 8192;     // source columns a workgroup keeps sums of
constexpr int MS_THREADS = 1024;
constexpr int MS_WAVES = MS_THREADS / 64;

struct MotionFrame {
    const unsigned char* p0;
    int h, w, stride0, format;
    int aligned;   // p0 and stride0 are multiples of 8: whole groups take the vector loads
};

struct MotionBatch {
    MotionFrame fr[YH_MOTION_LAUNCH];
    const int* stream_ids;   // the launch's first row (or NULL)
    unsigned char* staging;  // YH_MOTION_LAUNCH thumbnails
    int b0, streams, th, tw, chunks, tcw;
};

__device__ inline unsigned byte_of(unsigned v, int k) { return (v >> (8 * k)) & 0xffu; }

__global__ __launch_bounds__(MT_THREADS) void motion_thumb(const MotionBatch mb) {
    __shared__ unsigned colsum[MT_COLS + MT_PX];
    const int k = blockIdx.y;
    const int s = mb.stream_ids ? mb.stream_ids[k] : mb.b0 + k;   // one address for the workgroup: uniform
    if (s < 0 || s >= mb.streams) return;
    const MotionFrame& f = mb.fr[k];
    const int i = blockIdx.x / mb.chunks, ch = blockIdx.x - i * mb.chunks;
    const int j0 = ch * mb.tcw, j1 = j0 + mb.tcw < mb.tw ? j0 + mb.tcw : mb.tw;
    if (j0 >= j1) return;
    const int r0 = yh_motion_edge(i, f.h, mb.th), r1 = yh_motion_edge(i + 1, f.h, mb.th);
    const int cb = yh_motion_edge(j0, f.w, mb.tw), ce = yh_motion_edge(j1, f.w, mb.tw);
    const int cb8 = cb & ~(MT_PX - 1);
    const int groups = (ce - cb8 + MT_PX - 1) / MT_PX;   // <= MT_COLS / MT_PX + 1 (launch_motion's chunking)
    const bool nv12 = f.format == YH_PIX_NV12;
    for (int g = threadIdx.x; g < groups; g += MT_THREADS) {
        const int x0 = cb8 + g * MT_PX;
        unsigned acc[MT_PX];
#pragma unroll
        for (int q = 0; q < MT_PX; ++q) acc[q] = 0u;
        const bool whole = f.aligned && x0 + MT_PX <= f.w;
        for (int y = r0; y < r1; ++y) {
            const unsigned char* row = f.p0 + (size_t)y * f.stride0;
            if (whole && nv12) {
                const uint2 v = *reinterpret_cast<const uint2*>(row + x0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[q] += byte_of(v.x, q);
                    acc[4 + q] += byte_of(v.y, q);
                }
            } else if (whole) {
                const uint2* p = reinterpret_cast<const uint2*>(row + (size_t)x0 * 3);
                const uint2 a = p[0], b = p[1], c = p[2];
                const unsigned w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
                for (int q = 0; q < MT_PX; ++q) {
                    const int o = 3 * q;
                    acc[q] += yh_motion_luma(byte_of(w[o >> 2], o & 3), byte_of(w[(o + 1) >> 2], (o + 1) & 3),
                                             byte_of(w[(o + 2) >> 2], (o + 2) & 3));
                }
            } else {
#pragma unroll
                for (int q = 0; q < MT_PX; ++q) {
                    const int x = x0 + q;
                    if (x >= f.w) continue;
                    if (nv12) {
                        acc[q] += row[x];
                    } else {
                        const unsigned char* p = row + (size_t)x * 3;
                        acc[q] += yh_motion_luma(p[0], p[1], p[2]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MT_PX; ++q) colsum[g * MT_PX + q] = acc[q];
    }
    __syncthreads();
    unsigned char* dst = mb.staging + (size_t)k * mb.th * mb.tw + (size_t)i * mb.tw;
    for (int j = j0 + threadIdx.x; j < j1; j += MT_THREADS) {
        const int c0 = yh_motion_edge(j, f.w, mb.tw), c1 = yh_motion_edge(j + 1, f.w, mb.tw);
        unsigned sum = 0;
        for (int c = c0; c < c1; ++c) sum += colsum[c - cb8];
        dst[j] = (unsigned char)yh_motion_mean(sum, (unsigned)(r1 - r0) * (unsigned)(c1 - c0));
    }
}

// LDS of motion_search: the two thumbnails at pitch thumb_w + 4 (+ 8 bytes of slack each: the shift
// of the current one, the second dword of the last pair), the SAD table, the waves' keys
constexpr size_t ms_plane(int th, int tw) { return ((size_t)th * (tw + 4) + 8 + 15) & ~(size_t)15; }
constexpr size_t ms_lds(int th, int tw, int R) {
    return 2 * ms_plane(th, tw) + (size_t)(2 * R + 1) * (2 * R + 1) * 4 + MS_WAVES * 8;
}
constexpr size_t MS_LDS_MAX = 160 * 1024;

struct MotionSearch {
    int hw[YH_MOTION_LAUNCH][2];   // source height, width of the launch's frames
    const int* stream_ids;
    unsigned char* state;
    const unsigned char* staging;
    float* motion;                 // the launch's first row
    int32_t* sad;
    int b0, streams, th, tw, R, max_mad;
};

__global__ __launch_bounds__(MS_THREADS) void motion_search(const MotionSearch ms) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int th = ms.th, tw = ms.tw, R = ms.R, n = 2 * R + 1;
    float* mo = ms.motion + (size_t)k * 3;
    int32_t* so = ms.sad + (size_t)k * 2;
    const int s = ms.stream_ids ? ms.stream_ids[k] : ms.b0 + k;   // uniform
    if (s < 0 || s >= ms.streams) {
        if (tid == 0) {
            mo[0] = 1.0f; mo[1] = 0.0f; mo[2] = 0.0f;
            so[0] = 0; so[1] = 0;
        }
        return;
    }
    const int pitch = tw + 4;
    const int padc = (4 - (R & 3)) & 3;   // column R of the current thumbnail at a dword
    unsigned char* lc = smem;
    unsigned char* lp = smem + ms_plane(th, tw);
    uint64_t* wkey = reinterpret_cast<uint64_t*>(smem + 2 * ms_plane(th, tw));
    int32_t* table = reinterpret_cast<int32_t*>(wkey + MS_WAVES);
    const size_t pixels = (size_t)th * tw;
    unsigned char* blk = ms.state + (size_t)s * yh_motion_stream_bytes(th, tw);
    const uint32_t* gprev = reinterpret_cast<const uint32_t*>(blk + YH_MOTION_HDR);
    const uint32_t* gcur = reinterpret_cast<const uint32_t*>(ms.staging + (size_t)k * pixels);
    const uint32_t have = *reinterpret_cast<const uint32_t*>(blk);   // uniform
    const int rowdw = tw >> 2, ndw = th * rowdw;
    for (int e = tid; e < ndw; e += MS_THREADS) {
        const int i = e / rowdw, q = e - i * rowdw;
        const uint32_t c = gcur[e];
        unsigned char* d = lc + i * pitch + padc + 4 * q;
        d[0] = (unsigned char)c; d[1] = (unsigned char)(c >> 8); d[2] = (unsigned char)(c >> 16); d[3] = (unsigned char)(c >> 24);
        if (have) *reinterpret_cast<uint32_t*>(lp + i * pitch + 4 * q) = gprev[e];
    }
    // the 4 bytes between the rows and the 8 behind each plane: a pair's second dword reaches into
    // them; what it reads there the mask drops, but the bytes are defined
    for (int i = tid; i < th; i += MS_THREADS) {
        *reinterpret_cast<uint32_t*>(lp + i * pitch + tw) = 0u;
        unsigned char* d = lc + i * pitch + padc + tw;
        for (int q = 0; q < 4 - padc; ++q) d[q] = 0;
        for (int q = 0; q < padc; ++q) lc[i * pitch + q] = 0;
    }
    if (tid < 8) {
        lc[th * pitch + tid] = 0;
        lp[th * pitch + tid] = 0;
    }
    __syncthreads();   // the previous thumbnail is in LDS: its block may now be overwritten
    if (have) {
        const int wh = th - 2 * R, ww = tw - 2 * R;
        const int nq = (ww + 3) >> 2, total = wh * nq;
        const int rem = ww & 3;
        const uint32_t lastmask = rem ? (1u << (8 * rem)) - 1u : 0xffffffffu;
        const int cchunks = ((2 * R) >> 2) + 1;
        const uint32_t* cdw = reinterpret_cast<const uint32_t*>(lc);
        const uint32_t* pdw = reinterpret_cast<const uint32_t*>(lp);
        const int pdwp = pitch >> 2, cofs = (padc + R) >> 2;
        for (int item = wave; item < n * cchunks; item += MS_WAVES) {   // wave-uniform
            const int dyi = item / cchunks, c = item - dyi * cchunks;
            const int dy = dyi - R;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int e = lane; e < total; e += 64) {
                const int wi = e / nq, q = e - wi * nq;
                const int i = R + wi;
                const uint32_t m = q == nq - 1 ? lastmask : 0xffffffffu;
                const uint32_t cv = cdw[i * pdwp + cofs + q] & m;
                const uint32_t* pr = pdw + (i - dy) * pdwp + c + q;
                const uint32_t lo = pr[0], hi = pr[1];
                a0 = __builtin_amdgcn_sad_u8(cv, lo & m, a0);
                a1 = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(hi, lo, 1) & m, a1);
                a2 = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(hi, lo, 2) & m, a2);
                a3 = __builtin_amdgcn_sad_u8(cv, __builtin_amdgcn_alignbyte(hi, lo, 3) & m, a3);
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                a0 += (uint32_t)__shfl_xor((int)a0, d);
                a1 += (uint32_t)__shfl_xor((int)a1, d);
                a2 += (uint32_t)__shfl_xor((int)a2, d);
                a3 += (uint32_t)__shfl_xor((int)a3, d);
            }
            if (lane < 4) {   // previous-frame column offset o = 4 c + lane = R - dx
                const int o = 4 * c + lane;
                const uint32_t v = lane == 0 ? a0 : (lane == 1 ? a1 : (lane == 2 ? a2 : a3));
                if (o <= 2 * R) table[dyi * n + (2 * R - o)] = (int32_t)v;
            }
        }
        __syncthreads();
        uint64_t best = ~(uint64_t)0;
        for (int e = tid; e < n * n; e += MS_THREADS) {
            const int dyi = e / n, dxi = e - dyi * n;
            const uint64_t key = yh_motion_key((uint32_t)table[e], dyi - R, dxi - R);
            if (key < best) best = key;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)best, d);
            const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(best >> 32), d);
            const uint64_t o = ((uint64_t)hi << 32) | lo;
            if (o < best) best = o;
        }
        if (lane == 0) wkey[wave] = best;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < MS_WAVES; ++w)
                if (wkey[w] < best) best = wkey[w];
            float m[3];
            int32_t sv[2];
            yh_motion_result(table, R, yh_motion_key_dy(best), yh_motion_key_dx(best), ms.hw[k][0], ms.hw[k][1], th, tw,
                             ms.max_mad, m, sv);
            mo[0] = m[0]; mo[1] = m[1]; mo[2] = m[2];
            so[0] = sv[0]; so[1] = sv[1];
        }
    } else if (tid == 0) {
        mo[0] = 1.0f; mo[1] = 0.0f; mo[2] = 0.0f;
        so[0] = 0; so[1] = 0;
    }
    // the current thumbnail becomes the stream's
    uint32_t* gout = reinterpret_cast<uint32_t*>(blk + YH_MOTION_HDR);
    for (int e = tid; e < ndw; e += MS_THREADS) gout[e] = gcur[e];
    if (tid < 4) reinterpret_cast<uint32_t*>(blk)[tid] = tid == 0 ? 1u : 0u;
}

}  // namespace

int launch_motion(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams, int thumb_h,
                  int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, hipStream_t s) {
    // arguments were checked by yh_motion (yh_motion_check, and the alignment of state)
    if (batch <= 0) return 0;
    if (ms_lds(thumb_h, thumb_w, radius) > MS_LDS_MAX) return (int)hipErrorInvalidValue;   // cannot happen at the caps
    if (int rc = lds_optin(reinterpret_cast<const void*>(motion_search), (int)MS_LDS_MAX)) return rc;
    unsigned char* base = static_cast<unsigned char*>(state);
    unsigned char* staging = base + yh_motion_staging_offset(streams, thumb_h, thumb_w);
    for (int b0 = 0; b0 < batch; b0 += YH_MOTION_LAUNCH) {
        const int nb = batch - b0 < YH_MOTION_LAUNCH ? batch - b0 : YH_MOTION_LAUNCH;
        MotionBatch mb{};
        MotionSearch ms{};
        int wmax = 1;
        for (int k = 0; k < nb; ++k) {
            const yh_motion_src& f = src[b0 + k];
            mb.fr[k] = MotionFrame{f.p0, f.h, f.w, f.stride0, f.format,
                                   (reinterpret_cast<uintptr_t>(f.p0) | (uintptr_t)f.stride0) % 8 == 0 ? 1 : 0};
            ms.hw[k][0] = f.h;
            ms.hw[k][1] = f.w;
            wmax = f.w > wmax ? f.w : wmax;
        }
        // thumbnail columns per workgroup: their source columns (from the 8-aligned column at or
        // below the first) fit the workgroup's MT_COLS column sums
        int chunks = 1, tcw = thumb_w;
        while (tcw > 1 && ((long long)tcw * wmax + thumb_w - 1) / thumb_w + 1 + MT_PX > MT_COLS) {
            ++chunks;
            tcw = (thumb_w + chunks - 1) / chunks;
        }
        if (((long long)tcw * wmax + thumb_w - 1) / thumb_w + 1 + MT_PX > MT_COLS) return (int)hipErrorInvalidValue;
        chunks = (thumb_w + tcw - 1) / tcw;
        mb.stream_ids = stream_ids ? stream_ids + b0 : nullptr;
        mb.staging = staging;
        mb.b0 = b0; mb.streams = streams; mb.th = thumb_h; mb.tw = thumb_w; mb.chunks = chunks; mb.tcw = tcw;
        hipLaunchKernelGGL(motion_thumb, dim3((unsigned)(thumb_h * chunks), (unsigned)nb), dim3(MT_THREADS), 0, s, mb);
        if (hipError_t e = hipGetLastError()) return (int)e;
        ms.stream_ids = mb.stream_ids;
        ms.state = base;
        ms.staging = staging;
        ms.motion = motion + (size_t)b0 * 3;
        ms.sad = sad + (size_t)b0 * 2;
        ms.b0 = b0; ms.streams = streams; ms.th = thumb_h; ms.tw = thumb_w; ms.R = radius; ms.max_mad = max_mad;
        hipLaunchKernelGGL(motion_search, dim3((unsigned)nb), dim3(MS_THREADS), ms_lds(thumb_h, thumb_w, radius), s, ms);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

}  // namespace yh
