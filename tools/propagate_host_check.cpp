// Stand-alone driver of yh_propagate's host twin (csrc/propagate_host.cpp), for a sanitizer build on
// the CPU (make propagate_host_check builds and runs it):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/propagate_host_check.cpp yolo-infer-pt_amd/csrc/propagate_host.cpp \
//       yolo-infer-pt_amd/csrc/motion_host.cpp -lpthread -o build/propagate_host_check
// Frames, state and outputs live in exactly sized heap buffers, so a byte read beyond a frame's last
// row or column - the clamping of boxes that hang over every edge, or lie outside the frame - or
// written beyond an entry, the state or an output is a report: BGR and NV12, strided rows, cells of
// 1 x 1 up to the cap, radius 1 and YH_PROPAGATE_MAX_RADIUS, counts of 0 and beyond max_tracks,
// max_out below the survivors, permuted and invalid ids, non-finite boxes, threads 1 and 3, a
// remember - propagate - propagate - remember sequence. A planted shift is checked to come out with
// SAD 0. Exit status 0 and no sanitizer report is the result.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "propagate_host.h"

namespace {

int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what.c_str());
        ++fails;
    }
}

unsigned char world_at(int y, int x, int c) {
    uint32_t h = (uint32_t)(y * 7919 + x * 104729 + c * 31) * 2654435761u;
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

// boxes of a batch row: one inside (the planted shift is checked on it), then boxes over and beyond
// every edge, a huge one, a degenerate one and non-finite ones
std::vector<float> boxes_of(int h, int w, int side) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const float x = (float)(w / 2 - side / 2), y = (float)(h / 2 - side / 2), s = (float)side;
    const float b[][4] = {{x, y, x + s, y + s}, {-20, 5, 12, 40}, {(float)w - 9, 3, (float)w + 30, 50}, {8, -30, 50, 6},
                          {4, (float)h - 5, 70, (float)h + 90}, {-5000, -5000, 5000, 5000}, {-300, -300, -250, -260},
                          {7, 7, 7, 7}, {nan, 3, 40, 50}, {3, -inf, 40, inf}, {(float)w + 400, 2, (float)w + 500, 90}};
    std::vector<float> rows;
    for (const auto& q : b) {
        rows.insert(rows.end(), q, q + 4);
        rows.push_back(0.5f);
        rows.push_back(1.0f);
    }
    return rows;
}

void run(int h, int w, int R, int T, int max_out, int batch, int streams, int side, int sx, int sy, int threads) {
    const std::string what = std::to_string(h) + "x" + std::to_string(w) + " R " + std::to_string(R) + " T " +
                             std::to_string(T) + " batch " + std::to_string(batch);
    const std::vector<float> one = boxes_of(h, w, side);
    const int md = (int)one.size() / 6;
    std::unique_ptr<float[]> dets(new float[(size_t)batch * md * 6]), out(new float[(size_t)batch * max_out * 6 + 1]);
    std::unique_ptr<int32_t[]> ids(new int32_t[(size_t)batch * md]), oid(new int32_t[(size_t)batch * max_out + 1]),
        osad(new int32_t[(size_t)batch * max_out + 1]);
    std::unique_ptr<int[]> counts(new int[batch]), ocount(new int[batch]), sid(new int[batch]);
    for (int b = 0; b < batch; ++b) {
        std::memcpy(dets.get() + (size_t)b * md * 6, one.data(), one.size() * 4);
        for (int r = 0; r < md; ++r) ids[(size_t)b * md + r] = 10 * b + r + 1;
        counts[b] = b % 3 == 2 ? 0 : (b % 3 == 1 ? md + 5 : md);        // beyond max_det and max_tracks alike
        sid[b] = (b + 1) % batch < streams ? (b + 1) % batch : -1 - b;
    }
    const size_t sb = (size_t)streams * yh_prop_stream_bytes(T);
    std::unique_ptr<unsigned char[]> state(new unsigned char[sb]);
    std::memset(state.get(), 0, sb);
    int cell, origin;
    yh_prop_axis(one[0], one[2], &cell, &origin);
    for (int step = 0; step < 4; ++step) {               // remember, propagate, propagate, remember
        std::vector<Frame> frames;
        std::vector<yh_frame> desc;
        const int moved = step == 0 || step == 3 ? 0 : step;   // the content moves by `moved` shifts of whole cells
        for (int b = 0; b < batch; ++b) {
            frames.push_back(make_frame(h, w, b % 2 == 1 && h % 2 == 0 && w % 2 == 0, (b % 3) * 5, 64 - moved * sy * cell, 64 - moved * sx * cell));
            desc.push_back(frames.back().f);
        }
        std::vector<yh_motion_src> src(batch);
        if (step == 0 || step == 3) {
            const char* bad = yh_propagate_remember_check(desc.data(), batch, dets.get(), ids.get(), counts.get(), md, state.get(), streams, T, src.data());
            expect(!bad, what + ": remember check: " + (bad ? bad : ""));
            if (bad) return;
            yh_propagate_remember_host_run(src.data(), batch, sid.get(), dets.get(), ids.get(), counts.get(), md, state.get(), streams, T, threads);
            continue;
        }
        const char* bad = yh_propagate_check(desc.data(), batch, state.get(), streams, T, R, max_out, out.get(), oid.get(), osad.get(), ocount.get(), src.data());
        expect(!bad, what + ": check: " + (bad ? bad : ""));
        if (bad) return;
        yh_propagate_host_run(src.data(), batch, sid.get(), state.get(), streams, T, R, -1, max_out, out.get(), oid.get(), osad.get(), ocount.get(), threads);
        for (int b = 0; b < batch; ++b) {
            const bool valid = sid[b] >= 0 && sid[b] < streams;
            expect(ocount[b] >= 0 && ocount[b] <= max_out && (valid || ocount[b] == 0), what + ": count");
            if (!valid || counts[b] == 0 || max_out == 0) continue;
            // the first entry is the box inside the frame: it survives, and the planted shift comes out exactly
            const float* d = out.get() + (size_t)b * max_out * 6;
            expect(oid[(size_t)b * max_out] == 10 * b + 1 && osad[(size_t)b * max_out] == 0, what + ": the planted shift matches with SAD 0");
            expect(std::fabs(d[0] - (one[0] + (float)(step * sx * cell))) <= 0.5f * cell && std::fabs(d[1] - (one[1] + (float)(step * sy * cell))) <= 0.5f * cell,
                   what + ": shift, step " + std::to_string(step) + " (" + std::to_string(d[0]) + ", " + std::to_string(d[1]) + ")");
        }
    }
}

// a state from elsewhere: cells and origins far outside what the library writes must not take the
// twin out of the frame or overflow a coordinate sum
void foreign_state() {
    Frame fr = make_frame(40, 64, false, 0, 0, 0);
    std::unique_ptr<unsigned char[]> st(new unsigned char[yh_prop_stream_bytes(2)]);
    std::memset(st.get(), 0x7F, yh_prop_stream_bytes(2));          // every field 0x7F7F7F7F
    const uint32_t n = 2;
    std::memcpy(st.get(), &n, 4);
    const yh_prop_entry e{1, {0, 0, 8, 8}, 0.5f, 0, -3, 1 << 30, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, {0, 0, 0}};
    std::memcpy(st.get() + YH_PROP_HDR, &e, sizeof e);
    float d[12];
    int32_t id[2], sad[2];
    int count[1];
    yh_motion_src src;
    expect(!yh_propagate_check(&fr.f, 1, st.get(), 1, 2, 16, 2, d, id, sad, count, &src), "foreign state: check");
    yh_propagate_host_run(&src, 1, nullptr, st.get(), 1, 2, 16, -1, 2, d, id, sad, count, 1);
    expect(count[0] >= 0 && count[0] <= 2, "foreign state: count");
}

}  // namespace

int main() {
    run(97, 131, 2, 16, 16, 1, 1, 32, 1, -2, 1);      // odd BGR frame, cells 1 x 1
    run(96, 128, 3, 4, 2, 5, 4, 60, -3, 1, 3);        // NV12 among the rows, cells 2 x 2, the table and max_out below the rows
    run(40, 64, 1, 16, 16, 3, 3, 8, 1, 1, 3);         // radius 1, a box smaller than the template
    run(300, 420, YH_PROPAGATE_MAX_RADIUS, 3, 3, 2, 2, 100, 16, -16, 1);   // the largest radius, shifts of +-R
    run(64, 64, 2, 1, 0, 2, 1, 32, 0, 0, 1);          // max_tracks 1, no output rows
    foreign_state();
    if (fails == 0) std::printf("propagate_host_check: ok\n");
    return fails == 0 ? 0 : 1;
}
