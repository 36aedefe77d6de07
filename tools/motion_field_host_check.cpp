// Stand-alone driver of yh_motion_field's host twin (csrc/motion_host.cpp), for a sanitizer build on
// the CPU (make motion_field_host_check builds and runs it):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/motion_field_host_check.cpp yolo-infer-pt_amd/csrc/motion_host.cpp \
//       -lpthread -o build/motion_field_host_check
// Frames, state, outputs and the field live in exactly sized heap buffers, so a byte read or written
// beyond a block's last column, the previous thumbnail's first or last row, the state or an output
// is a report: the smallest legal blocks (4 x 4) and thumbnails, grids whose edges fall off every
// alignment, 1 x 1, the block cap, radius 1 and YH_MOTION_MAX_RADIUS, BGR and NV12, batches beyond one
// staging round with permuted and invalid ids, threads 1 and 3, yh_motion and yh_motion_field
// alternating on one state; the argument check. A known shift is checked to come out of the fit, a
// 1 x 1 grid to equal yh_motion. Exit status 0 and no sanitizer report is the result.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "motion_host.h"

namespace {

int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what.c_str());
        ++fails;
    }
}

// blocky texture (8 x 8 source pixels per cell) so that thumbnails keep contrast
unsigned char world_at(int y, int x, int c) {
    uint32_t h = (uint32_t)((y >> 3) * 7919 + (x >> 3) * 104729 + c * 31) * 2654435761u;
    h ^= h >> 15;
    h *= 2246822519u;
    return (unsigned char)(h >> 24);
}

struct Frame {
    std::unique_ptr<unsigned char[]> p0, p1;   // exactly sized
    yh_frame f;
};

Frame make_frame(int h, int w, bool nv12, int pad, int oy, int ox) {
    Frame fr;
    const int row0 = nv12 ? w : 3 * w, stride0 = row0 + pad;
    const size_t n0 = (size_t)(h - 1) * stride0 + row0;
    fr.p0.reset(new unsigned char[n0]);
    std::memset(fr.p0.get(), 0xEE, n0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < (nv12 ? 1 : 3); ++c)
                fr.p0[(size_t)y * stride0 + (nv12 ? x : 3 * x + c)] = world_at(y + oy, x + ox, nv12 ? 1 : c);
    fr.f = yh_frame{fr.p0.get(), nullptr, h, w, pad ? stride0 : 0, 0, nv12 ? YH_PIX_NV12 : YH_PIX_BGR, YH_YUV_BT601};
    if (nv12) {
        const size_t n1 = (size_t)(h / 2 - 1) * (w + pad) + w;
        fr.p1.reset(new unsigned char[n1]);
        std::memset(fr.p1.get(), 0x80, n1);
        fr.f.plane1 = fr.p1.get();
        fr.f.stride1 = pad ? w + pad : 0;
    }
    return fr;
}

// `steps` calls of `batch` rows on one state, the camera moving by (cy, cx) source pixels per step;
// every `plain_every`-th step advances the state with yh_motion instead
void run(int h, int w, int th, int tw, int R, int gh, int gw, int batch, int streams, int steps, int cy, int cx,
         int threads, int plain_every, bool check_shift) {
    const std::string what = std::to_string(h) + "x" + std::to_string(w) + " thumb " + std::to_string(th) + "x" +
                             std::to_string(tw) + " R " + std::to_string(R) + " grid " + std::to_string(gh) + "x" +
                             std::to_string(gw) + " batch " + std::to_string(batch);
    const yh_motion_field_params p{gh, gw, R, -1, 1, 0, 2, 0};   // tol 0: the inliers share one model exactly
    const int NB = gh * gw;
    const size_t sb = yh_motion_staging_offset(streams, th, tw) + (size_t)YH_MOTION_LAUNCH * th * tw;
    std::unique_ptr<unsigned char[]> state(new unsigned char[sb]), twin(new unsigned char[sb]);
    std::memset(state.get(), 0, sb);
    std::unique_ptr<float[]> motion(new float[(size_t)batch * 3]), pm(new float[(size_t)batch * 3]);
    std::unique_ptr<int32_t[]> sad(new int32_t[(size_t)batch * 2]), ps(new int32_t[(size_t)batch * 2]);
    std::unique_ptr<int32_t[]> field(new int32_t[(size_t)batch * NB * 4]);
    std::unique_ptr<int[]> ids(new int[batch]);
    for (int b = 0; b < batch; ++b) ids[b] = (b * 7 + 3) % batch < streams ? (b * 7 + 3) % batch : -1 - b;
    if (batch % 7 == 0)   // 7 b is no permutation then
        for (int b = 0; b < batch; ++b) ids[b] = b < streams ? streams - 1 - b : streams + b;
    for (int step = 0; step < steps; ++step) {
        std::vector<Frame> frames;
        std::vector<yh_frame> desc;
        for (int b = 0; b < batch; ++b) {
            frames.push_back(make_frame(h, w, b % 2 == 1 && h % 2 == 0 && w % 2 == 0, (b % 3) * 5, 64 + step * cy, 64 + step * cx));
            desc.push_back(frames.back().f);
        }
        std::vector<yh_motion_src> src(batch);
        const char* bad = yh_motion_check(desc.data(), batch, state.get(), streams, th, tw, R, motion.get(), sad.get(), src.data());
        if (!bad) bad = yh_motion_field_check(&p, th, tw);
        expect(bad == nullptr, what + ": check: " + (bad ? bad : ""));
        if (bad) return;
        // yh_motion on a copy of the state: the sad columns always agree, a 1 x 1 grid in every byte
        std::memcpy(twin.get(), state.get(), sb);
        yh_motion_host_run(src.data(), batch, ids.get(), twin.get(), streams, th, tw, R, -1, pm.get(), ps.get(), threads);
        if (plain_every && step % plain_every == plain_every - 1) {
            std::memcpy(state.get(), twin.get(), sb);
            continue;
        }
        std::memset(field.get(), 0x55, (size_t)batch * NB * 16);
        yh_motion_field_host_run(src.data(), batch, ids.get(), state.get(), streams, th, tw, &p, motion.get(), sad.get(),
                                 step % 2 ? field.get() : nullptr, threads);
        expect(std::memcmp(state.get(), twin.get(), sb) == 0, what + ": the state advances as under yh_motion");
        expect(std::memcmp(sad.get(), ps.get(), (size_t)batch * 8) == 0, what + ": sad is the global table's");
        if (NB == 1) expect(std::memcmp(motion.get(), pm.get(), (size_t)batch * 12) == 0, what + ": 1 x 1 equals yh_motion");
        for (int b = 0; b < batch; ++b) {
            const float* m = motion.get() + 3 * b;
            const bool valid = ids[b] >= 0 && ids[b] < streams;
            expect(m[0] >= 0.8f && m[0] <= 1.25f && std::isfinite(m[1]) && std::isfinite(m[2]), what + ": motion row");
            if (!valid || step == 0) expect(m[0] == 1.0f && m[1] == 0.0f && m[2] == 0.0f, what + ": identity row");
            if (step % 2)
                for (int k = 0; k < NB; ++k) {
                    const int32_t* f = field.get() + ((size_t)b * NB + k) * 4;
                    expect(f[0] >= -R && f[0] <= R && f[1] >= -R && f[1] <= R && f[2] >= 0 && (f[3] & ~3) == 0, what + ": field row");
                }
            if (valid && step > 0 && check_shift)   // whole thumbnail pixels: every block finds the shift, s = 1 exactly
                expect(m[0] == 1.0f && std::fabs(m[1] + (float)cx) <= 0.01f && std::fabs(m[2] + (float)cy) <= 0.01f,
                       what + ": shift (" + std::to_string(m[0]) + ", " + std::to_string(m[1]) + ", " + std::to_string(m[2]) + ")");
        }
    }
}

void check_args() {
    auto bad = [](yh_motion_field_params p, int th, int tw) { return yh_motion_field_check(&p, th, tw) != nullptr; };
    const yh_motion_field_params ok{2, 3, 2, 24, 4, 1, 2, 0};
    expect(!bad(ok, 12, 16), "args: 4 x 4 blocks are legal");
    expect(yh_motion_field_check(nullptr, 12, 16) != nullptr, "args: null params");
    yh_motion_field_params p = ok;
    p.grid_h = 3;
    expect(bad(p, 12, 16), "args: a block below 4 rows");
    p = ok; p.grid_w = 4;
    expect(bad(p, 12, 16), "args: a block below 4 columns");
    p = ok; p.grid_h = 0;
    expect(bad(p, 12, 16), "args: grid_h 0");
    p = ok; p.grid_h = 17; p.grid_w = 16;
    expect(bad(p, 128, 128), "args: more than YH_MOTION_FIELD_MAX_BLOCKS");
    p = ok; p.min_blocks = 1;
    expect(bad(p, 12, 16), "args: min_blocks");
    p = ok; p.tol = -1;
    expect(bad(p, 12, 16), "args: tol");
    p = ok; p.min_contrast = -1;
    expect(bad(p, 12, 16), "args: min_contrast");
    p = yh_motion_field_params{1, 10, YH_MOTION_MAX_RADIUS, 24, 4, 1, 2, 0};
    expect(bad(p, 128, 256), "args: the LDS cap");
}

}  // namespace

int main() {
    run(12, 16, 12, 16, 2, 2, 3, 1, 1, 3, 1, -1, 1, 0, false);          // the frame is the thumbnail, blocks 4 x 4
    run(48, 64, 12, 16, 2, 2, 3, 3, 3, 3, 4, -4, 3, 0, true);            // 4 x 4 source pixels per thumbnail pixel
    run(120, 156, 40, 52, 3, 3, 4, 4, 4, 4, 3, -3, 3, 0, true);          // ragged block edges, R % 4 != 0
    run(120, 156, 40, 52, 3, 1, 1, 2, 2, 3, 3, 3, 1, 0, false);          // 1 x 1
    run(74, 104, 37, 52, 1, 8, 11, 2, 2, 2, 2, 2, 3, 0, true);           // radius 1, 88 blocks of 4 x 4
    run(140, 144, 70, 72, YH_MOTION_MAX_RADIUS, 1, 2, 2, 2, 2, 2, -2, 3, 0, false);   // the largest radius
    run(33, 101, 16, 24, 2, 3, 4, 5, 4, 3, 1, 3, 3, 0, false);           // odd frame sizes, uneven boxes
    run(96, 128, 24, 32, 2, 2, 2, 35, 30, 4, 4, 4, 3, 2, true);          // two staging rounds, invalid ids, yh_motion in between
    check_args();
    if (fails == 0) std::printf("motion_field_host_check: ok\n");
    return fails == 0 ? 0 : 1;
}
