// Error plumbing and dtype casts shared by the host translation units behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "yolo_hip.h"

namespace yh {

inline thread_local std::string g_err;   // yh_last_error

struct Fail : std::runtime_error {
    int code;
    Fail(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHECK(expr)                                                                     \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess)                                                             \
            throw yh::Fail(YH_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

inline void require(bool ok, const std::string& msg, int code = YH_EINVAL) {
    if (!ok) throw Fail(code, msg);
}

// body of an extern "C" entry point: exceptions become a status code and yh_last_error's text
template <typename F>
int guarded(F&& f) {
    try {
        f();
        g_err.clear();
        return YH_OK;
    } catch (const Fail& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_err = e.what();
        return YH_EINVAL;
    } catch (...) {
        g_err = "unknown error";
        return YH_EINVAL;
    }
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------- dtype casts
inline uint16_t f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t f2h(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (ax > 0x7f800000u ? 0x200u : 0u));
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to inf
    if (ax < 0x38800000u) {  // subnormal / zero in half
        float af;
        std::memcpy(&af, &ax, 4);
        const float scaled = af * 16777216.0f;  // 2^24: half subnormal unit = 2^-24
        const uint32_t m = (uint32_t)std::nearbyint(scaled);
        return (uint16_t)(sign | m);
    }
    uint32_t e = ((ax >> 23) - 112u) << 10;
    uint32_t m = (ax >> 13) & 0x3ffu;
    uint32_t h = e | m;
    const uint32_t rem = ax & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
}
inline float bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline float h2f(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
    uint32_t u;
    if (e == 0) {
        if (m == 0) {
            u = s;
        } else {  // subnormal
            int ee = -1;
            uint32_t mm = m;
            do { ++ee; mm <<= 1; } while (!(mm & 0x400));
            u = s | ((uint32_t)(127 - 15 - ee) << 23) | ((mm & 0x3ff) << 13);
        }
    } else if (e == 31) {
        u = s | 0x7f800000u | (m << 13);
    } else {
        u = s | ((e + 127 - 15) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// f rounded to the dtype (YH_F32 / YH_F16 / YH_BF16) and back: round to nearest even, as torch's
// casts. The device and the host NMS round the confidence threshold with this.
inline float round_to_dtype(int dtype, float f) {
    return dtype == YH_F16 ? h2f(f2h(f)) : (dtype == YH_BF16 ? bf2f(f2bf(f)) : f);
}

}  // namespace yh
