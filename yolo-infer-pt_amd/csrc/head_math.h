// Value arithmetic of the detect head's decode (nets/nn.py:255-270, DFL 222-225, make_anchors
// utils/util.py:85-96), written once for decode.hip (head_decode, head_decode_lds) and head.hip
// (box_dfl, head_cls's direct mode): the fused and the per-layer paths agree bit for bit by calling these.
#pragma once
#include "common.h"
#include "dtypes.h"

namespace yh {

template <typename T> __device__ __forceinline__ float ex(float x) { return __expf(x); }
template <> __device__ __forceinline__ float ex<float>(float x) { return expf(x); }
// a / b: correctly rounded on the f32 (parity) path, hardware reciprocal on the
// 16-bit paths, whose outputs are rounded to 8 / 11 mantissa bits anyway (same
// policy as silu, dtypes.h)
template <typename T> __device__ __forceinline__ float dv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
template <> __device__ __forceinline__ float dv<float>(float a, float b) { return a / b; }
template <typename T> __device__ __forceinline__ float sigmoid(float x) { return dv<T>(1.0f, 1.0f + ex<T>(-x)); }
// sigmoid<T> of two adjacent values of a 16-bit path on one register pair (as silu2, dtypes.h): the
// multiply by -log2e that ex<T>(-x) expands to and the add packed, exp and rcp per element
template <typename T> __device__ __forceinline__ f32x2 sigmoid2(f32x2 x) {
    static_assert(sizeof(T) == 2, "sigmoid2: the 16-bit handles only");
    const f32x2 t = 0x1.715476p+0f * -x;
    const f32x2 d = 1.0f + f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    return f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
}

// DFL: softmax over the 16 bins of one box side, expectation with weights 0..15 (v is overwritten)
template <typename T>
__device__ __forceinline__ float dfl16(float (&v)[16]) {
    float mx = v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, v[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = ex<T>(v[i] - mx); sum += v[i]; }
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) d = fmaf((float)i, dv<T>(v[i], sum), d);
    return d;
}

// anchor a of the three levels' concatenated pixels (l0, l1 = the pixels of levels 0 and 1):
// its level l and its pixel loc within that level
struct LevelLoc { int l, loc; };
__device__ __forceinline__ LevelLoc anchor_level(int l0, int l1, int a) {
    int l = 0, loc = a;
    if (loc >= l0) { loc -= l0; l = 1; if (loc >= l1) { loc -= l1; l = 2; } }
    return LevelLoc{l, loc};
}

// dist2bbox at pixel (gx, gy) of a level, in two steps (box_dfl's lane halves each take two of
// the four outputs). The anchor point is the pixel centre, d = the (left, top, right, bottom)
// distances: the box's edges e = (x1, y1, x2, y2) in grid units,
__device__ __forceinline__ void box_edges(int gx, int gy, const float (&d)[4], float (&e)[4]) {
    const float ax = (float)gx + 0.5f, ay = (float)gy + 0.5f;
    e[0] = ax - d[0]; e[1] = ay - d[1];
    e[2] = ax + d[2]; e[3] = ay + d[3];
}
// then per axis the centre and the extent in input pixels: o = (cx, cy, w, h)
__device__ __forceinline__ float box_centre(float lo, float hi, float stride) { return (lo + hi) / 2.0f * stride; }
__device__ __forceinline__ float box_extent(float lo, float hi, float stride) { return (hi - lo) * stride; }
__device__ __forceinline__ void dist2bbox(int gx, int gy, float stride, const float (&d)[4], float (&o)[4]) {
    float e[4];
    box_edges(gx, gy, d, e);
    o[0] = box_centre(e[0], e[2], stride);
    o[1] = box_centre(e[1], e[3], stride);
    o[2] = box_extent(e[0], e[2], stride);
    o[3] = box_extent(e[1], e[3], stride);
}

}  // namespace yh
