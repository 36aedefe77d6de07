// Stand-alone driver of the camera-motion host twins (csrc/motion_host.cpp, and yh_track_warp's in
// csrc/track_host.cpp), for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/motion_host_check.cpp yolo-infer-pt_amd/csrc/motion_host.cpp \
//       yolo-infer-pt_amd/csrc/track_host.cpp yolo-infer-pt_amd/csrc/assign_host.cpp -lpthread -o build/motion_host_check
//   build/motion_host_check
// Every frame, state and output lives in an exactly sized heap buffer, so a read or write one byte
// beyond a plane's last row, the state or the outputs is a report: frames of the minimum legal sizes
// (the thumbnail's own size, and the smallest thumbnail a radius admits), strided rows whose last row
// ends with the frame, box edges where H % thumb_h != 0 and W % thumb_w != 0, BGR and NV12, radius 1
// and YH_MOTION_MAX_RADIUS, batches beyond one staging round, permuted and invalid ids, threads 1
// and 3; the argument check; both layouts of the warp with valid, invalid and out-of-range rows.
// Known shifts are checked to come out. Exit status 0 and no sanitizer report is the result.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "motion_host.h"
#include "track_host.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what.c_str());
        ++fails;
    }
}

// a world of pixel noise (no two windows alike), sampled at an offset
unsigned char world_at(int y, int x, int c) {
    uint32_t h = (uint32_t)(y * 7919 + x * 104729 + c * 31) * 2654435761u;
    h ^= h >> 15;
    h *= 2246822519u;
    return (unsigned char)(h >> 24);
}

struct Frame {
    std::unique_ptr<unsigned char[]> p0, p1;   // exactly sized: (h - 1) * stride + row bytes
    yh_frame f;
};

Frame make_frame(int h, int w, int format, int pad, int oy, int ox) {
    Frame fr;
    const bool nv12 = format == YH_PIX_NV12;
    const int row0 = nv12 ? w : 3 * w, stride0 = row0 + pad;
    const size_t n0 = (size_t)(h - 1) * stride0 + row0;
    fr.p0.reset(new unsigned char[n0]);
    std::memset(fr.p0.get(), 0xEE, n0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            if (nv12) {
                fr.p0[(size_t)y * stride0 + x] = world_at(y + oy, x + ox, 1);
            } else {
                for (int c = 0; c < 3; ++c) fr.p0[(size_t)y * stride0 + 3 * x + c] = world_at(y + oy, x + ox, c);
            }
        }
    fr.f = yh_frame{fr.p0.get(), nullptr, h, w, pad ? stride0 : 0, 0, format, YH_YUV_BT601};
    if (nv12) {
        const int stride1 = w + pad;
        const size_t n1 = (size_t)(h / 2 - 1) * stride1 + w;
        fr.p1.reset(new unsigned char[n1]);
        std::memset(fr.p1.get(), 0x80, n1);
        fr.f.plane1 = fr.p1.get();
        fr.f.stride1 = pad ? stride1 : 0;
    }
    return fr;
}

size_t state_bytes(int streams, int th, int tw) {
    return yh_motion_staging_offset(streams, th, tw) + (size_t)YH_MOTION_LAUNCH * th * tw;
}

// `steps` frames of `batch` rows; the camera moves by (cy, cx) source pixels per step
void run_motion(int h, int w, int th, int tw, int R, int batch, int streams, int steps, int cy, int cx, int threads,
                bool check_shift) {
    const std::string what = std::to_string(h) + "x" + std::to_string(w) + " thumb " + std::to_string(th) + "x" +
                             std::to_string(tw) + " R " + std::to_string(R) + " batch " + std::to_string(batch);
    const size_t sb = state_bytes(streams, th, tw);
    std::unique_ptr<unsigned char[]> state(new unsigned char[sb]);
    std::memset(state.get(), 0, sb);
    std::unique_ptr<float[]> motion(new float[(size_t)batch * 3]);
    std::unique_ptr<int32_t[]> sad(new int32_t[(size_t)batch * 2]);
    std::unique_ptr<int[]> ids(new int[batch]);
    for (int b = 0; b < batch; ++b) ids[b] = (b * 7 + 3) % batch < streams ? (b * 7 + 3) % batch : -1 - b;
    if (batch % 7 == 0)
        for (int b = 0; b < batch; ++b) ids[b] = b < streams ? streams - 1 - b : streams + b;
    for (int step = 0; step < steps; ++step) {
        std::vector<Frame> frames;
        std::vector<yh_frame> desc;
        for (int b = 0; b < batch; ++b) {
            const bool nv12 = b % 2 == 1 && h % 2 == 0 && w % 2 == 0;
            frames.push_back(make_frame(h, w, nv12 ? YH_PIX_NV12 : YH_PIX_BGR, (b % 3) * 5, 64 + step * cy, 64 + step * cx));
            desc.push_back(frames.back().f);
        }
        std::vector<yh_motion_src> src(batch);
        const char* bad = yh_motion_check(desc.data(), batch, state.get(), streams, th, tw, R, motion.get(), sad.get(), src.data());
        expect(bad == nullptr, what + ": check: " + (bad ? bad : ""));
        if (bad) return;
        yh_motion_host_run(src.data(), batch, ids.get(), state.get(), streams, th, tw, R, -1, motion.get(), sad.get(), threads);
        for (int b = 0; b < batch; ++b) {
            const float* m = motion.get() + 3 * b;
            const bool valid = ids[b] >= 0 && ids[b] < streams;
            expect(m[0] == 1.0f && std::isfinite(m[1]) && std::isfinite(m[2]), what + ": motion row");
            if (!valid || step == 0) expect(m[1] == 0.0f && m[2] == 0.0f && sad[2 * b] == 0, what + ": identity row");
            if (valid && step > 0 && check_shift) {
                // content moves against the camera; whole thumbnail pixels match exactly
                expect(sad[2 * b] == 0, what + ": an exact shift has SAD 0");
                expect(std::fabs(m[1] + (float)cx) <= (float)w / tw && std::fabs(m[2] + (float)cy) <= (float)h / th,
                       what + ": shift (" + std::to_string(m[1]) + ", " + std::to_string(m[2]) + ")");
            }
        }
    }
}

void check_args() {
    Frame fr = make_frame(12, 16, YH_PIX_BGR, 0, 0, 0);
    float m[3];
    int32_t s[2];
    unsigned char st[16];
    yh_motion_src src;
    auto bad = [&](const yh_frame& f, int batch, int th, int tw, int R) {
        return yh_motion_check(&f, batch, st, 1, th, tw, R, m, s, &src) != nullptr;
    };
    expect(!bad(fr.f, 1, 12, 16, 2), "args: the minimum frame is legal");
    expect(bad(fr.f, 1, 12, 18, 2), "args: thumb_w % 4");
    expect(bad(fr.f, 1, 12, 16, 0) && bad(fr.f, 1, 12, 16, YH_MOTION_MAX_RADIUS + 1), "args: radius");
    expect(bad(fr.f, 1, 12, 16, 5), "args: window below 4");
    expect(bad(fr.f, 1, 13, 16, 2) && bad(fr.f, 1, 12, 20, 2), "args: frame below the thumbnail");
    expect(bad(fr.f, 1, 256, 256, 2), "args: MAX_THUMB");
    expect(bad(fr.f, -1, 12, 16, 2), "args: batch");
    yh_frame f = fr.f;
    f.stride0 = 47;
    expect(bad(f, 1, 12, 16, 2), "args: stride");
    f = fr.f;
    f.format = 5;
    expect(bad(f, 1, 12, 16, 2), "args: format");
    f = fr.f;
    f.format = YH_PIX_NV12;
    expect(bad(f, 1, 12, 16, 2), "args: NV12 without plane1");
    f = fr.f;
    f.plane0 = nullptr;
    expect(bad(f, 1, 12, 16, 2), "args: plane0");
}

void run_warp(int T, int reid_dim, int streams) {
    const std::string what = "warp T " + std::to_string(T) + " dim " + std::to_string(reid_dim);
    const size_t stride = yh_track_warp_stride(T, reid_dim), bytes = stride * streams;
    std::unique_ptr<char[]> state(new char[bytes]), before(new char[bytes]);
    for (size_t i = 0; i < bytes; ++i) state[i] = (char)(rnd() >> 8);
    for (int s = 0; s < streams; ++s) {
        uint32_t* w = reinterpret_cast<uint32_t*>(state.get() + s * stride);
        for (int t = 0; t < T; ++t) {
            w[YH_TRACK_HDR + t] = (uint32_t)((t + s) % 4);
            for (int f = YH_TRK_X; f < YH_TRACK_FIELDS; ++f) {
                const float v = (float)(rnd() % 2000) * 0.25f;
                std::memcpy(w + YH_TRACK_HDR + (size_t)f * T + t, &v, 4);
            }
        }
    }
    std::memcpy(before.get(), state.get(), bytes);
    const int batch = streams + 1;
    std::unique_ptr<float[]> motion(new float[(size_t)batch * 3]);
    std::unique_ptr<int[]> ids(new int[batch]);
    for (int b = 0; b < batch; ++b) {
        ids[b] = b < streams ? streams - 1 - b : streams + 2;
        motion[3 * b] = b % 3 == 2 ? NAN : (b % 3 == 1 ? 0.5f : 1.0f);
        motion[3 * b + 1] = 3.5f;
        motion[3 * b + 2] = -2.0f;
    }
    expect(yh_track_warp_check(state.get(), streams, T, reid_dim, motion.get(), batch) == nullptr, what + ": check");
    for (int threads : {1, 3}) {
        std::memcpy(state.get(), before.get(), bytes);
        yh_track_warp_host_run(state.get(), streams, T, reid_dim, motion.get(), ids.get(), batch, threads);
        for (int b = 0; b < streams; ++b) {
            const int s = ids[b];
            const char* a = state.get() + s * stride;
            const char* o = before.get() + s * stride;
            const size_t words = yh_track_stream_words(T) * 4;
            expect(std::memcmp(a, o, YH_TRACK_HDR * 4 + 4 * (size_t)T * YH_TRK_X) == 0, what + ": header / status / id / last / class");
            expect(std::memcmp(a + words, o + words, stride - words) == 0, what + ": gallery");
            if (b % 3 == 2) expect(std::memcmp(a, o, stride) == 0, what + ": a NaN motion changes nothing");
            for (int t = 0; t < T; ++t) {
                float x0, y0;
                std::memcpy(&x0, a + 4 * (YH_TRACK_HDR + (size_t)YH_TRK_X * T + t), 4);
                std::memcpy(&y0, o + 4 * (YH_TRACK_HDR + (size_t)YH_TRK_X * T + t), 4);
                const bool live = (t + s) % 4 != 0;
                const float sc = motion[3 * b];
                if (b % 3 != 2) expect(live ? x0 == sc * y0 + 3.5f : x0 == y0, what + ": cx");
            }
        }
    }
    expect(yh_track_warp_check(state.get(), streams, 0, reid_dim, motion.get(), batch) != nullptr, what + ": max_tracks 0");
    expect(yh_track_warp_check(state.get(), streams, T, 60, motion.get(), batch) != nullptr, what + ": bad dim");
}

}  // namespace

int main() {
    // the minimum legal sizes: the frame is the thumbnail, the window is 4 x 4
    run_motion(6, 8, 6, 8, 1, 1, 1, 3, 1, -1, 1, true);
    run_motion(12, 16, 12, 16, 2, 3, 3, 3, 2, 2, 1, true);
    // the smallest thumbnail of the largest radius
    run_motion(70, 70, 68, 68, YH_MOTION_MAX_RADIUS, 2, 2, 2, 0, 0, 3, false);
    run_motion(136, 204, 68, 68, YH_MOTION_MAX_RADIUS, 2, 2, 3, 8, -12, 3, true);     // 2 x 3 px boxes, 4 thumbnail pixels
    // box edges: H % thumb_h != 0, W % thumb_w != 0, odd sizes (BGR only), strided rows
    run_motion(33, 101, 12, 16, 2, 5, 4, 3, 1, 3, 3, false);
    run_motion(37, 50, 24, 40, 4, 4, 6, 3, -1, 2, 1, false);
    // more rows than staging slots, invalid ids among them
    run_motion(24, 32, 12, 16, 2, 35, 30, 2, 2, 2, 3, true);
    run_motion(48, 64, 12, 16, 2, 70, 70, 3, -4, 4, 3, true);
    check_args();
    run_warp(1, 0, 1);
    run_warp(7, 0, 3);
    run_warp(16, 64, 4);
    run_warp(5, 128, 2);
    if (fails == 0) std::printf("motion_host_check: ok\n");
    return fails == 0 ? 0 : 1;
}
