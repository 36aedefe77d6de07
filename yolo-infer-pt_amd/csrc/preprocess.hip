// Eval-mode image preprocessing of the reference's data loader, on the device
// (yh_letterbox_frames, yh_letterbox) and on the host (yh_letterbox_frames_host,
// yh_letterbox_host: same per-pixel functions):
//
//   utils/dataset.py:95-103  load_image: r = input_size / max(h, w); if r != 1
//                            cv2.resize(image, (int(w r), int(h r)), INTER_LINEAR)
//   utils/dataset.py:292-313 resize (augment=False): r <= 1 so no second resize;
//                            zero border (cv2.copyMakeBorder, BORDER_CONSTANT) of
//                            top = round(dh - 0.1), left = round(dw - 0.1) to a
//                            square canvas of input_size
//   utils/dataset.py:86-88   HWC -> CHW and BGR -> RGB
//
// cv2.resize INTER_LINEAR on 8-bit images (OpenCV's published algorithm; cv2 is
// not in this image, so this restatement is parity-unpinned against cv2 itself):
//   scale = 1 / (dst / src) in double; per destination column
//   f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s, with s < 0 -> (0, f 0)
//   and s >= src - 1 -> (src - 1, f 0) on the x axis (rows are clamped instead);
//   11-bit coefficients a0 = rint((1 - f) 2048), a1 = rint(f 2048);
//   horizontal pass in int: H = S[s] a0 + S[s + 1] a1;
//   vertical pass as OpenCV's vector kernel computes it (VResizeLinearVec_32s8u, x86
//   builds with 128-bit universal intrinsics):
//   out = sat_u8((mulhi16(H0 >> 4, b0) + mulhi16(H1 >> 4, b1) + 2) >> 2)
//   over the row's bytes the vector loops cover (16-byte steps while x <= width - 16,
//   then one 8-byte step while x < width - 8, width = 3 nw bytes); the remaining tail
//   bytes take the scalar FixedPtCast: out = sat_u8((H0 b0 + H1 b1 + 2^21) >> 22).
//   Which vector width the cv2 build used is an assumption (parity unpinned vs cv2).
//   Exactly 2x downscales on both axes take INTER_AREA's fast path
//   ((S00 + S01 + S10 + S11 + 2) >> 2), as cv2.resize does.
//
// Beyond the reference (include/yolo_hip.h states the semantics): the canvas may be a
// rectangle (r = min(canvas_h / h, canvas_w / w), the same division for a square one), and
// a frame may be NV12. An NV12 source pixel is converted to B, G, R by lb_tap (integer,
// shift 20, nearest chroma; OpenCV's published COLOR_YUV2BGR_NV12 coefficients, parity
// unpinned against cv2 like the resize) wherever the resize reads a source pixel, so the
// canvas is the BGR letterbox of the converted frame without that frame ever existing.
// yh_crop_rois / yh_crop_rois_host (further down) run the same resize with a box of a frame as
// the source: one fixed-size crop per detection.
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "host_parallel.h"
#include "host_util.h"
#include "yolo_hip.h"

namespace yh {

enum LbMode { LB_COPY = 0, LB_AREA2 = 1, LB_LINEAR = 2 };

struct LbImage {
    const unsigned char* p0;    // BGR: HWC uint8; NV12: the Y plane
    const unsigned char* p1;    // NV12: interleaved U, V rows (h / 2 rows of w bytes)
    double sx, sy;              // LB_LINEAR: source step per resized pixel (lb_finish)
    int h, w, stride0, stride1; // source size, row strides of the planes in bytes
    int nh, nw;                 // resized size
    int top, left;              // border
    int tail;                   // lb_vtail(3 nw)
    int format, matrix;         // YH_PIX_*, YH_YUV_*
    int mode;                   // LbMode
    int ox, oy;                 // origin of the h x w source inside the planes (a crop; 0 for a whole frame)
};

struct LbAxis {
    int s0, s1, a0, a1;
};

// one destination coordinate of the linear resize (see header comment)
__host__ __device__ inline LbAxis lb_axis(int d, int src, double scale, bool clamp_coef) {
#pragma clang fp contract(off)
    const float f0 = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f0);
    float f = f0 - (float)s;
    if (clamp_coef) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
    }
    LbAxis ax;
    ax.a0 = (int)rintf((1.f - f) * 2048.f);
    ax.a1 = (int)rintf(f * 2048.f);
    ax.s0 = s < 0 ? 0 : (s > src - 1 ? src - 1 : s);
    ax.s1 = s + 1 < 0 ? 0 : (s + 1 > src - 1 ? src - 1 : s + 1);
    return ax;
}

__host__ __device__ inline int lb_mulhi(int a, int b) { return (a * b) >> 16; }

// first byte of a resized row (width = 3 nw bytes) that OpenCV's vertical pass computes
// with its scalar loop instead of VResizeLinearVec_32s8u (see the header comment)
__host__ __device__ inline int lb_vtail(int width) {
    int x = width >= 16 ? ((width - 16) / 16 + 1) * 16 : 0;
    if (x < width - 8) x += 8;
    return x;
}

__host__ __device__ inline int lb_sat(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// B, G, R of source pixel (y, x): the bytes of a BGR frame, one conversion of an NV12 frame
// (limited range, shift 20, the chroma pair of (y >> 1, x >> 1); include/yolo_hip.h). The origin
// is added here, so the chroma pair of a crop is that of the absolute pixel (odd origins are legal).
__host__ __device__ inline void lb_tap(const LbImage& im, int y, int x, int bgr[3]) {
    y += im.oy;
    x += im.ox;
    if (im.format == YH_PIX_NV12) {
        const int Y = im.p0[(size_t)y * im.stride0 + x];
        const unsigned char* c = im.p1 + (size_t)(y >> 1) * im.stride1 + ((x >> 1) << 1);
        const int u = c[0] - 128, v = c[1] - 128;
        const bool m709 = im.matrix == YH_YUV_BT709;
        const int cub = m709 ? 2214593 : 2116026, cug = m709 ? -223347 : -409993;
        const int cvg = m709 ? -558891 : -852492, cvr = m709 ? 1880097 : 1673527;
        const int yy = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19);
        bgr[0] = lb_sat((yy + cub * u) >> 20);
        bgr[1] = lb_sat((yy + cvg * v + cug * u) >> 20);
        bgr[2] = lb_sat((yy + cvr * v) >> 20);
        return;
    }
    const unsigned char* p = im.p0 + (size_t)y * im.stride0 + (size_t)x * 3;
    bgr[0] = p[0]; bgr[1] = p[1]; bgr[2] = p[2];
}

// what the pixels of one canvas row share: the resized row and its vertical taps
struct LbRow {
    int dy;        // row of the resized image, -1 for a border row
    LbAxis ay;     // LB_LINEAR only
};

__host__ __device__ inline LbRow lb_row(const LbImage& im, int y) {
    LbRow r;
    r.dy = y - im.top;
    r.ay = LbAxis{0, 0, 0, 0};
    if (r.dy < 0 || r.dy >= im.nh) r.dy = -1;
    else if (im.mode == LB_LINEAR) r.ay = lb_axis(r.dy, im.h, im.sy, false);
    return r;
}

// Pixel x of canvas row `row`, 3 channels in RGB order.
__host__ __device__ inline void lb_pixel_row(const LbImage& im, const LbRow& row, int x, unsigned char rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0;
    const int dy = row.dy, dx = x - im.left;
    if (dy < 0 || dx < 0 || dx >= im.nw) return;
    if (im.mode == LB_COPY) {   // r == 1: no resize (load_image skips it)
        int t[3];
        lb_tap(im, dy, dx, t);
        rgb[0] = (unsigned char)t[2]; rgb[1] = (unsigned char)t[1]; rgb[2] = (unsigned char)t[0];
        return;
    }
    if (im.mode == LB_AREA2) {   // INTER_AREA fast path
        int t00[3], t01[3], t10[3], t11[3];
        lb_tap(im, 2 * dy, 2 * dx, t00);
        lb_tap(im, 2 * dy, 2 * dx + 1, t01);
        lb_tap(im, 2 * dy + 1, 2 * dx, t10);
        lb_tap(im, 2 * dy + 1, 2 * dx + 1, t11);
        for (int c = 0; c < 3; ++c) rgb[2 - c] = (unsigned char)((t00[c] + t01[c] + t10[c] + t11[c] + 2) >> 2);
        return;
    }
    const LbAxis ax = lb_axis(dx, im.w, im.sx, true);
    const LbAxis& ay = row.ay;
    int t00[3], t01[3], t10[3], t11[3];
    lb_tap(im, ay.s0, ax.s0, t00);
    lb_tap(im, ay.s0, ax.s1, t01);
    lb_tap(im, ay.s1, ax.s0, t10);
    lb_tap(im, ay.s1, ax.s1, t11);
    for (int c = 0; c < 3; ++c) {
        const int h0 = t00[c] * ax.a0 + t01[c] * ax.a1;
        const int h1 = t10[c] * ax.a0 + t11[c] * ax.a1;
        const int v = dx * 3 + c < im.tail ? (lb_mulhi(h0 >> 4, ay.a0) + lb_mulhi(h1 >> 4, ay.a1) + 2) >> 2
                                           : (h0 * ay.a0 + h1 * ay.a1 + (1 << 21)) >> 22;
        rgb[2 - c] = (unsigned char)lb_sat(v);
    }
}

// the resize path and its constants from h, w, nh, nw
__host__ __device__ inline void lb_finish(LbImage& im) {
    im.mode = im.nh == im.h && im.nw == im.w ? LB_COPY : (im.h == 2 * im.nh && im.w == 2 * im.nw ? LB_AREA2 : LB_LINEAR);
    im.sx = 1.0 / ((double)im.nw / (double)im.w);
    im.sy = 1.0 / ((double)im.nh / (double)im.h);
    im.tail = lb_vtail(3 * im.nw);
}

// geometry of one image on a canvas_h x canvas_w canvas (dataset.py:95-103, 292-313 for a
// square one), in the reference's double arithmetic; NULL or the reason it is rejected
__host__ __device__ inline const char* lb_geometry(int h, int w, int ch, int cw, LbImage& im) {
    if (h <= 0 || w <= 0 || ch <= 0 || cw <= 0) return "letterbox: image and canvas sides must be positive";
    const double rh = (double)ch / (double)h, rw = (double)cw / (double)w;
    const double r = rh < rw ? rh : rw;
    int nh = h, nw = w;
    if (r != 1.0) { nw = (int)(w * r); nh = (int)(h * r); }
    if (nh < 1 || nw < 1) return "letterbox: a resized side is below 1 pixel";
    if (nh > ch || nw > cw) return "letterbox: the resized image exceeds the canvas";
    const double dw = (cw - nw) / 2.0, dh = (ch - nh) / 2.0;
    im.h = h; im.w = w; im.nh = nh; im.nw = nw;
    im.top = (int)nearbyint(dh - 0.1);
    im.left = (int)nearbyint(dw - 0.1);
    lb_finish(im);
    return nullptr;
}

// descriptor of one frame on a canvas; throws Fail(YH_EINVAL) with the reason
inline LbImage lb_describe(const yh_frame& f, int ch, int cw) {
    LbImage im{};
    require(f.format == YH_PIX_BGR || f.format == YH_PIX_NV12, "letterbox: unknown pixel format " + std::to_string(f.format));
    const bool nv12 = f.format == YH_PIX_NV12;
    if (nv12) {
        require(f.matrix == YH_YUV_BT601 || f.matrix == YH_YUV_BT709, "letterbox: unknown YUV matrix " + std::to_string(f.matrix));
        require(f.height > 0 && f.width > 0 && f.height % 2 == 0 && f.width % 2 == 0,
                "letterbox: an NV12 frame needs even, positive height and width");
    }
    require(f.plane0 != nullptr, "letterbox: plane0 is NULL");
    require(!nv12 || f.plane1 != nullptr, "letterbox: plane1 of an NV12 frame is NULL");
    const char* why = lb_geometry(f.height, f.width, ch, cw, im);
    require(why == nullptr, why ? why : "");
    const int row0 = nv12 ? f.width : 3 * f.width;
    im.stride0 = f.stride0 ? f.stride0 : row0;
    im.stride1 = nv12 ? (f.stride1 ? f.stride1 : f.width) : 0;
    require(im.stride0 >= row0 && (!nv12 || im.stride1 >= f.width), "letterbox: a stride is smaller than the row");
    im.p0 = static_cast<const unsigned char*>(f.plane0);
    im.p1 = nv12 ? static_cast<const unsigned char*>(f.plane1) : nullptr;
    im.format = f.format;
    im.matrix = nv12 ? f.matrix : 0;
    return im;
}

constexpr int LB_MAX = 32;   // frames per launch (kernarg-resident descriptors)
struct LbBatch {
    LbImage im[LB_MAX];
    unsigned char* dst;      // (n, 3, ch, cw) uint8
    int ch, cw, n;
    int dwords;              // every 4-pixel group of dst is an aligned dword (cw % 4 == 0, dst % 4 == 0)
};

// One thread: 4 consecutive canvas pixels of one row, all three planes; consecutive lanes write
// consecutive dwords of a row. The row's vertical taps are computed once (lb_row).
__global__ __launch_bounds__(256) void letterbox_frames_u8(const LbBatch b) {
    const int i = blockIdx.y;
    const int gw = (b.cw + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= gw * b.ch) return;
    const int y = q / gw, x0 = (q - y * gw) * 4;
    const LbImage& im = b.im[i];
    const LbRow row = lb_row(im, y);
    unsigned out[3] = {0u, 0u, 0u};
    if (row.dy >= 0 && x0 + 3 >= im.left && x0 < im.left + im.nw) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned char rgb[3];
            lb_pixel_row(im, row, x0 + k, rgb);
            out[0] |= (unsigned)rgb[0] << (8 * k);
            out[1] |= (unsigned)rgb[1] << (8 * k);
            out[2] |= (unsigned)rgb[2] << (8 * k);
        }
    }
    const size_t plane = (size_t)b.ch * b.cw;
    unsigned char* o = b.dst + (size_t)i * 3 * plane + (size_t)y * b.cw + x0;
    if (b.dwords) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<unsigned*>(o + c * plane) = out[c];
    } else {   // a canvas width or base that is no multiple of 4 (yh_letterbox accepts any size)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 4 && x0 + k < b.cw; ++k) o[c * plane + k] = (unsigned char)(out[c] >> (8 * k));
    }
}

// validates every frame, then one launch per LB_MAX frames; frames[k] may come from `at(k)`
template <typename At>
void lb_launch(At&& at, int batch, int ch, int cw, void* dst, void* stream) {
    require(batch >= 0 && ch > 0 && cw > 0, "letterbox: negative batch or empty canvas");
    require(batch == 0 || dst != nullptr, "letterbox: dst is NULL");
    for (int k = 0; k < batch; ++k) lb_describe(at(k), ch, cw);
    const size_t plane = (size_t)ch * cw;
    for (int b0 = 0; b0 < batch; b0 += LB_MAX) {
        LbBatch lb{};
        lb.n = batch - b0 < LB_MAX ? batch - b0 : LB_MAX;
        lb.ch = ch; lb.cw = cw;
        lb.dst = static_cast<unsigned char*>(dst) + (size_t)b0 * 3 * plane;
        lb.dwords = cw % 4 == 0 && reinterpret_cast<uintptr_t>(lb.dst) % 4 == 0;
        for (int k = 0; k < lb.n; ++k) lb.im[k] = lb_describe(at(b0 + k), ch, cw);
        const long long groups = (long long)((cw + 3) / 4) * ch;
        require(groups < (1ll << 31), "letterbox: canvas too large");
        const dim3 g((unsigned)((groups + 255) / 256), (unsigned)lb.n);
        hipLaunchKernelGGL(letterbox_frames_u8, g, dim3(256), 0, (hipStream_t)stream, lb);
        HIPCHECK(hipGetLastError());
    }
}

void lb_host(const yh_frame& f, int ch, int cw, void* dst, int threads) {
    require(ch > 0 && cw > 0, "letterbox: empty canvas");
    require(dst != nullptr, "letterbox: dst is NULL");
    const LbImage im = lb_describe(f, ch, cw);
    unsigned char* o = static_cast<unsigned char*>(dst);
    const size_t plane = (size_t)ch * cw;
    auto rows = [&](int y0, int y1) {
        for (int y = y0; y < y1; ++y) {
            const LbRow row = lb_row(im, y);
            for (int x = 0; x < cw; ++x) {
                unsigned char rgb[3];
                lb_pixel_row(im, row, x, rgb);
                const size_t q = (size_t)y * cw + x;
                o[q] = rgb[0]; o[plane + q] = rgb[1]; o[2 * plane + q] = rgb[2];
            }
        }
    };
    parallel_blocks(ch, threads > 0 ? threads : 1, rows);   // threads <= 0: the caller's thread alone
}

inline yh_frame lb_bgr_frame(const void* src, int height, int width, int stride) {
    yh_frame f{};
    f.plane0 = src;
    f.height = height; f.width = width;
    f.stride0 = stride;
    f.format = YH_PIX_BGR;
    return f;
}

// ---------------------------------------------------------------- yh_crop_rois
// Fixed-size crops of boxes from BGR / NV12 frames (no reference counterpart; include/yolo_hip.h
// states the semantics, tests/_crop_cases.py restates them). A crop is the letterbox above with
// the rectangle as its source: crop_image turns a frame's descriptor and a box into an LbImage
// whose origin lb_tap adds, on the device and on the host alike.

struct CropRect {
    int x0, y0, w, h;
};

// the exponent is not all ones (a bit test: no floating-point assumption can fold it away)
__host__ __device__ inline bool crop_finite(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u;
}

// (int)min(max(v, 0), hi), clamped in float: v is finite, so the conversion is defined
__host__ __device__ inline int crop_clamp(float v, int hi) {
    const float h = (float)hi;
    v = v < 0.f ? 0.f : v;
    v = v > h ? h : v;
    return (int)v;
}

// The padded box, rounded outwards and clipped to the H x W frame; false for an empty ROI
// (rc is zero then). fp32, one rounding per operation.
__host__ __device__ inline bool crop_rect(const float* box, float pad, int H, int W, CropRect& rc) {
#pragma clang fp contract(off)
    rc = CropRect{0, 0, 0, 0};
    const float x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
    const float bw = x2 - x1, bh = y2 - y1;
    const float px = bw * pad, py = bh * pad;
    const float X1 = x1 - px, Y1 = y1 - py, X2 = x2 + px, Y2 = y2 + py;
    if (!(crop_finite(X1) && crop_finite(Y1) && crop_finite(X2) && crop_finite(Y2))) return false;
    const int ix0 = crop_clamp(floorf(X1), W), ix1 = crop_clamp(ceilf(X2), W);
    const int iy0 = crop_clamp(floorf(Y1), H), iy1 = crop_clamp(ceilf(Y2), H);
    const int w = ix1 - ix0, h = iy1 - iy0;
    if (w < 1 || h < 1) return false;
    rc = CropRect{ix0, iy0, w, h};
    return true;
}

// LbImage of one ROI on an oh x ow crop from `fr`, its frame described on the frame's own size;
// false for an empty ROI (rc is zero then)
__host__ __device__ inline bool crop_image(const LbImage& fr, const float* box, float pad, int oh, int ow,
                                           int keep_aspect, LbImage& im, CropRect& rc) {
    im = fr;
    if (!crop_rect(box, pad, fr.h, fr.w, rc)) return false;
    if (keep_aspect) {
        if (lb_geometry(rc.h, rc.w, oh, ow, im) != nullptr) {   // a resized side below 1 pixel
            rc = CropRect{0, 0, 0, 0};
            return false;
        }
    } else {
        im.h = rc.h; im.w = rc.w; im.nh = oh; im.nw = ow;
        im.top = im.left = 0;
        lb_finish(im);
    }
    im.ox = rc.x0; im.oy = rc.y0;
    return true;
}

__host__ __device__ inline int crop_count(int n, int max_rois) { return n < 0 ? 0 : (n > max_rois ? max_rois : n); }

struct CropBatch {
    LbImage fr[LB_MAX];      // frames b0 .. b0 + LB_MAX - 1, each on its own size
    const float* boxes;      // (batch, max_rois, box_stride)
    const int* counts;       // (batch)
    unsigned char* crops;    // (capacity, 3, oh, ow) uint8, 4-byte aligned, ow % 4 == 0
    int* rois;               // (capacity, 6)
    int* total;              // (1)
    int batch, b0, max_rois, box_stride, oh, ow, keep_aspect, capacity, chunks;
    float pad;
};

enum CropState { CROP_SKIP = 0, CROP_ZERO = 1, CROP_LIVE = 2 };
// 4-pixel groups per workgroup, one per thread. 1024 (a loop of four per thread) was measured too:
// the walk and the geometry are then paid a quarter as often, which helps few small crops, but the
// loop costs 24 VGPRs (84: 5 waves per SIMD instead of 8) and many large crops get slower
// (DESIGN.md section 14).
constexpr int CROP_CHUNK = 256;

// One workgroup: CROP_CHUNK 4-pixel groups (a chunk) of one slot. Wave 0 finds the slot's
// (frame, row) by a prefix walk over all clamped counts and makes the ROI's LbImage once; then one
// thread is 4 consecutive pixels of a crop row, all three planes, as in letterbox_frames_u8. A slot
// whose frame another launch holds is left to that launch; the launch of frame 0 zero-fills the
// slots beyond total and writes total.
__global__ __launch_bounds__(256) void crop_rois_u8(const CropBatch b) {
    __shared__ LbImage s_im;
    __shared__ int s_state;
    const int slot = blockIdx.x / b.chunks, chunk = blockIdx.x - slot * b.chunks;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const bool first = b.b0 == 0;
        const bool need_total = first && blockIdx.x == 0;
        int base = 0, f = -1, r = 0;
        for (int k0 = 0; k0 < b.batch && (f < 0 || need_total); k0 += 64) {
            const int k = k0 + lane;
            const int n = k < b.batch ? crop_count(b.counts[k], b.max_rois) : 0;
            int inc = n;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(inc, d);
                if (lane >= d) inc += t;
            }
            const int excl = base + inc - n;
            const unsigned long long hit = __ballot(slot >= excl && slot < excl + n);
            if (hit != 0 && f < 0) {
                const int src = __ffsll((long long)hit) - 1;
                f = k0 + src;
                r = slot - __shfl(excl, src);
            }
            base += __shfl(inc, 63);
        }
        // f, r and base are the same in every lane
        int state = f < 0 ? (first ? CROP_ZERO : CROP_SKIP) : CROP_SKIP;
        LbImage im;
        CropRect rc{0, 0, 0, 0};
        if (f >= b.b0 && f < b.b0 + LB_MAX) {
            const int fl = __builtin_amdgcn_readfirstlane(f - b.b0);
            const float* box = b.boxes + ((size_t)f * b.max_rois + r) * b.box_stride;
            state = crop_image(b.fr[fl], box, b.pad, b.oh, b.ow, b.keep_aspect, im, rc) ? CROP_LIVE : CROP_ZERO;
        }
        if (lane == 0) {
            s_state = state;
            if (state == CROP_LIVE) s_im = im;
            if (chunk == 0 && state != CROP_SKIP) {
                int* o = b.rois + (size_t)slot * 6;
                o[0] = f < 0 ? 0 : f; o[1] = f < 0 ? 0 : r;
                o[2] = rc.x0; o[3] = rc.y0; o[4] = rc.w; o[5] = rc.h;
            }
            if (need_total) *b.total = base < b.capacity ? base : b.capacity;
        }
    }
    __syncthreads();
    const int state = s_state;
    if (state == CROP_SKIP) return;
    const int gw = b.ow >> 2;
    const int q = chunk * CROP_CHUNK + threadIdx.x;
    if (q >= gw * b.oh) return;
    const int y = q / gw, x0 = (q - y * gw) * 4;
    unsigned out[3] = {0u, 0u, 0u};
    if (state == CROP_LIVE) {
        const LbImage& im = s_im;
        const LbRow row = lb_row(im, y);
        if (row.dy >= 0 && x0 + 3 >= im.left && x0 < im.left + im.nw) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned char rgb[3];
                lb_pixel_row(im, row, x0 + k, rgb);
                out[0] |= (unsigned)rgb[0] << (8 * k);
                out[1] |= (unsigned)rgb[1] << (8 * k);
                out[2] |= (unsigned)rgb[2] << (8 * k);
            }
        }
    }
    const size_t plane = (size_t)b.oh * b.ow;
    unsigned char* o = b.crops + (size_t)slot * 3 * plane + (size_t)y * b.ow + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<unsigned*>(o + c * plane) = out[c];
}

struct CropArgs {
    const yh_frame* frames;
    int batch;
    const float* boxes;
    int box_stride;
    const int* counts;
    int max_rois, oh, ow, keep_aspect;
    float pad;
    int capacity;
    void* crops;
    int* rois;
    int* total;
};

// every YH_EINVAL of yh_crop_rois / yh_crop_rois_host; returns the frames on their own sizes
std::vector<LbImage> crop_check(const CropArgs& a) {
    require(a.batch >= 0 && a.max_rois >= 0 && a.capacity >= 0, "crop_rois: negative batch, max_rois or capacity");
    require(a.oh >= 1, "crop_rois: out_h must be at least 1");
    require(a.ow >= 4 && a.ow % 4 == 0, "crop_rois: out_w must be a positive multiple of 4");
    require(a.box_stride >= 4, "crop_rois: box_stride must be at least 4");
    require(crop_finite(a.pad) && a.pad >= 0.f, "crop_rois: pad must be finite and not negative");
    require(a.keep_aspect == 0 || a.keep_aspect == 1, "crop_rois: keep_aspect must be 0 or 1");
    require(a.total != nullptr, "crop_rois: total is NULL");
    require(a.batch == 0 || (a.frames != nullptr && a.counts != nullptr), "crop_rois: frames or counts is NULL");
    require(a.batch == 0 || a.max_rois == 0 || a.boxes != nullptr, "crop_rois: boxes is NULL");
    require(a.capacity == 0 || (a.crops != nullptr && a.rois != nullptr), "crop_rois: crops or rois is NULL");
    require((long long)a.batch * a.max_rois < (1ll << 31), "crop_rois: batch * max_rois too large");
    std::vector<LbImage> fr((size_t)a.batch);
    for (int k = 0; k < a.batch; ++k) fr[k] = lb_describe(a.frames[k], a.frames[k].height, a.frames[k].width);
    return fr;
}

void crop_launch(const CropArgs& a, void* stream) {
    const std::vector<LbImage> fr = crop_check(a);
    require(reinterpret_cast<uintptr_t>(a.crops) % 4 == 0, "crop_rois: crops must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (a.capacity == 0) {
        HIPCHECK(hipMemsetAsync(a.total, 0, sizeof(int), st));
        return;
    }
    const long long groups = (long long)(a.ow / 4) * a.oh;
    const long long chunks = (groups + CROP_CHUNK - 1) / CROP_CHUNK;
    require(groups < (1ll << 30) && chunks * a.capacity < (1ll << 31), "crop_rois: capacity x crop size too large");
    CropBatch cb{};
    cb.boxes = a.boxes; cb.counts = a.counts;
    cb.crops = static_cast<unsigned char*>(a.crops); cb.rois = a.rois; cb.total = a.total;
    cb.batch = a.batch; cb.max_rois = a.max_rois; cb.box_stride = a.box_stride;
    cb.oh = a.oh; cb.ow = a.ow; cb.keep_aspect = a.keep_aspect; cb.capacity = a.capacity;
    cb.chunks = (int)chunks; cb.pad = a.pad;
    for (int b0 = 0; b0 == 0 || b0 < a.batch; b0 += LB_MAX) {   // batch 0: one launch zero-fills
        cb.b0 = b0;
        for (int k = 0; k < LB_MAX; ++k) cb.fr[k] = b0 + k < a.batch ? fr[b0 + k] : LbImage{};
        hipLaunchKernelGGL(crop_rois_u8, dim3((unsigned)(chunks * a.capacity)), dim3(256), 0, st, cb);
        HIPCHECK(hipGetLastError());
    }
}

void crop_host(const CropArgs& a, int threads) {
    const std::vector<LbImage> fr = crop_check(a);
    std::vector<long long> start((size_t)a.batch + 1, 0);
    for (int k = 0; k < a.batch; ++k) start[k + 1] = start[k] + crop_count(a.counts[k], a.max_rois);
    const int total = (int)(start[a.batch] < a.capacity ? start[a.batch] : a.capacity);
    *a.total = total;
    const size_t plane = (size_t)a.oh * a.ow;
    unsigned char* crops = static_cast<unsigned char*>(a.crops);
    auto slots = [&](int s0, int s1) {
        int f = 0;
        for (int s = s0; s < s1; ++s) {
            unsigned char* o = crops + (size_t)s * 3 * plane;
            int* ro = a.rois + (size_t)s * 6;
            LbImage im;
            CropRect rc{0, 0, 0, 0};
            bool live = false;
            ro[0] = ro[1] = 0;
            if (s < total) {
                while (start[f + 1] <= s) ++f;
                const int r = (int)(s - start[f]);
                ro[0] = f; ro[1] = r;
                live = crop_image(fr[f], a.boxes + ((size_t)f * a.max_rois + r) * a.box_stride, a.pad, a.oh, a.ow,
                                  a.keep_aspect, im, rc);
            }
            ro[2] = rc.x0; ro[3] = rc.y0; ro[4] = rc.w; ro[5] = rc.h;
            if (!live) {
                std::memset(o, 0, 3 * plane);
                continue;
            }
            for (int y = 0; y < a.oh; ++y) {
                const LbRow row = lb_row(im, y);
                for (int x = 0; x < a.ow; ++x) {
                    unsigned char rgb[3];
                    lb_pixel_row(im, row, x, rgb);
                    const size_t q = (size_t)y * a.ow + x;
                    o[q] = rgb[0]; o[plane + q] = rgb[1]; o[2 * plane + q] = rgb[2];
                }
            }
        }
    };
    parallel_blocks(a.capacity, threads, slots);
}

}  // namespace yh

using namespace yh;

extern "C" int yh_letterbox_geometry2(int height, int width, int canvas_h, int canvas_w, int* new_h, int* new_w,
                                      int* top, int* left) {
    return guarded([&] {
        LbImage im{};
        const char* why = lb_geometry(height, width, canvas_h, canvas_w, im);
        require(why == nullptr, why ? why : "");
        if (new_h) *new_h = im.nh;
        if (new_w) *new_w = im.nw;
        if (top) *top = im.top;
        if (left) *left = im.left;
    });
}

extern "C" int yh_letterbox_geometry(int height, int width, int size, int* new_h, int* new_w, int* top,
                                     int* left) {
    return yh_letterbox_geometry2(height, width, size, size, new_h, new_w, top, left);
}

extern "C" int yh_letterbox_frames(const yh_frame* frames, int batch, int canvas_h, int canvas_w, void* dst,
                                   void* stream) {
    return guarded([&] {
        require(batch <= 0 || frames != nullptr, "letterbox_frames: frames is NULL");
        require(canvas_w % 4 == 0, "letterbox_frames: canvas_w must be a multiple of 4");
        lb_launch([&](int k) -> const yh_frame& { return frames[k]; }, batch, canvas_h, canvas_w, dst, stream);
    });
}

extern "C" int yh_letterbox_frames_host(const yh_frame* frame, int canvas_h, int canvas_w, void* dst, int threads) {
    return guarded([&] {
        require(frame != nullptr, "letterbox_frames_host: frame is NULL");
        lb_host(*frame, canvas_h, canvas_w, dst, threads);
    });
}

extern "C" int yh_nv12_to_bgr_host(const yh_frame* frame, void* dst_bgr) {
    return guarded([&] {
        require(frame != nullptr && dst_bgr != nullptr, "nv12_to_bgr_host: NULL argument");
        require(frame->format == YH_PIX_NV12, "nv12_to_bgr_host: the frame is not NV12");
        // the frame's own size as the canvas: validates planes, strides and the matrix
        const LbImage im = lb_describe(*frame, frame->height, frame->width);
        unsigned char* o = static_cast<unsigned char*>(dst_bgr);
        for (int y = 0; y < im.h; ++y)
            for (int x = 0; x < im.w; ++x) {
                int t[3];
                lb_tap(im, y, x, t);
                unsigned char* p = o + ((size_t)y * im.w + x) * 3;
                p[0] = (unsigned char)t[0]; p[1] = (unsigned char)t[1]; p[2] = (unsigned char)t[2];
            }
    });
}

extern "C" int yh_crop_rois(const yh_frame* frames, int batch, const float* boxes, int box_stride, const int* counts,
                            int max_rois, int out_h, int out_w, int keep_aspect, float pad, int capacity, void* crops,
                            int* rois, int* total, void* stream) {
    return guarded([&] {
        crop_launch(CropArgs{frames, batch, boxes, box_stride, counts, max_rois, out_h, out_w, keep_aspect, pad,
                             capacity, crops, rois, total}, stream);
    });
}

extern "C" int yh_crop_rois_host(const yh_frame* frames, int batch, const float* boxes, int box_stride,
                                 const int* counts, int max_rois, int out_h, int out_w, int keep_aspect, float pad,
                                 int capacity, void* crops, int* rois, int* total, int threads) {
    return guarded([&] {
        crop_host(CropArgs{frames, batch, boxes, box_stride, counts, max_rois, out_h, out_w, keep_aspect, pad,
                           capacity, crops, rois, total}, threads);
    });
}

extern "C" int yh_letterbox(const void* const* srcs, const int* heights, const int* widths, const int* strides,
                            int batch, int size, void* dst, void* stream) {
    return guarded([&] {
        require(batch <= 0 || (srcs && heights && widths), "letterbox: NULL argument");
        lb_launch([&](int k) { return lb_bgr_frame(srcs[k], heights[k], widths[k], strides ? strides[k] : 0); },
                  batch, size, size, dst, stream);
    });
}

extern "C" int yh_letterbox_host(const void* src, int height, int width, int stride, int size, void* dst,
                                 int threads) {
    return guarded([&] { lb_host(lb_bgr_frame(src, height, width, stride > 0 ? stride : 0), size, size, dst, threads); });
}

extern "C" int yh_resize_linear_host(const void* src, int height, int width, int stride, int new_h, int new_w,
                                     void* dst) {
    if (!src || !dst || height <= 0 || width <= 0 || new_h <= 0 || new_w <= 0) return YH_EINVAL;
    LbImage im{};
    im.p0 = static_cast<const unsigned char*>(src);
    im.h = height; im.w = width; im.nh = new_h; im.nw = new_w;
    im.stride0 = stride > 0 ? stride : 3 * width;
    if (im.stride0 < 3 * width) return YH_EINVAL;
    im.format = YH_PIX_BGR;
    lb_finish(im);
    unsigned char* o = static_cast<unsigned char*>(dst);
    for (int y = 0; y < new_h; ++y) {
        const LbRow row = lb_row(im, y);
        for (int x = 0; x < new_w; ++x) {
            unsigned char rgb[3];
            lb_pixel_row(im, row, x, rgb);
            unsigned char* p = o + ((size_t)y * new_w + x) * 3;
            p[0] = rgb[2]; p[1] = rgb[1]; p[2] = rgb[0];
        }
    }
    return YH_OK;
}
