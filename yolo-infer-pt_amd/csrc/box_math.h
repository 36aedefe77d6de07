// Box arithmetic of the stages after the forward (match, merge, track), HIP-free. A kernel and its
// host twin must agree bit for bit, so every formula they share is written once, here or in the
// stage's *_host.h, and compiled for both sides (build both with -ffp-contract=off).
#ifndef YH_BOX_MATH_H
#define YH_BOX_MATH_H

#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define YH_HD __host__ __device__ inline
#else
#define YH_HD inline
#endif

#define YH_STR_(x) #x
#define YH_STR(x) YH_STR_(x)

namespace yh {

// min / max / max(v, 0) as a compare and a select. They agree with torch (whose min / max
// propagate NaN) for finite inputs, as NMS output and labels are.
YH_HD float lesser(float a, float b) { return b < a ? b : a; }
YH_HD float greater(float a, float b) { return a < b ? b : a; }
YH_HD float clamp0(float v) { return v < 0.0f ? 0.0f : v; }

// area of the intersection of the boxes a and b, each side clamped at 0
YH_HD float intersection(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
    const float w = clamp0(lesser(ax2, bx2) - greater(ax1, bx1));
    const float h = clamp0(lesser(ay2, by2) - greater(ay1, by1));
    return w * h;
}

// An unsigned that orders like the float (negative floats included); Descending: its complement,
// which orders the other way round. (The complement is taken here, not by the caller: the
// compiler then folds it into the map, and merge's kernel depends on that instruction.)
template <bool Descending = false>
YH_HD uint32_t float_order(float v) {
    uint32_t u;
#ifdef __HIP_DEVICE_COMPILE__
    u = __float_as_uint(v);
#else
    std::memcpy(&u, &v, 4);
#endif
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return Descending ? ~u : u;
}

}  // namespace yh

#endif
