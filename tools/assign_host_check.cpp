// Stand-alone driver of the assignment's host twins (csrc/assign_host.cpp, and the tracker's
// optimal mode in csrc/track_host.cpp), for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/assign_host_check.cpp yolo-infer-pt_amd/csrc/assign_host.cpp \
//       yolo-infer-pt_amd/csrc/track_host.cpp -lpthread -o build/assign_host_check
//   build/assign_host_check
// Every problem runs on exactly sized heap buffers, so a read or write one element beyond the
// live corner, the matrix or the outputs is a report: small shapes (1 x 1, rectangular both
// ways, the wave edges 63 / 64 / 65, a band that forces long paths, tie-heavy, sparse), counts
// above the sizes and below 0, weights outside [0, MAX_WEIGHT], threads 1 and 3; the argument
// check with sizes above the caps and below 0; then a crowded tracker sequence in optimal mode,
// plain and with features. Each matching is checked to be a valid one whose total is not below
// the greedy walk's. Exit status 0 and no sanitizer report is the result.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "assign_host.h"
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

long long greedy_total(const std::vector<int>& w, int nt, int nd, int D) {
    struct P { int w, t, d; };
    std::vector<P> pairs;
    for (int t = 0; t < nt; ++t)
        for (int d = 0; d < nd; ++d)
            if (yh_assign_clamp(w[(size_t)t * D + d]) > 0) pairs.push_back({yh_assign_clamp(w[(size_t)t * D + d]), t, d});
    std::sort(pairs.begin(), pairs.end(), [](const P& a, const P& b) {
        if (a.w != b.w) return a.w > b.w;
        if (a.t != b.t) return a.t < b.t;
        return a.d < b.d;
    });
    std::vector<char> ut(nt, 0), ud(nd, 0);
    long long total = 0;
    for (const P& p : pairs)
        if (!ut[p.t] && !ud[p.d]) {
            ut[p.t] = ud[p.d] = 1;
            total += p.w;
        }
    return total;
}

// kind: 0 random dense, 1 tie-heavy, 2 sparse, 3 band, 4 out-of-range weights
void solver_case(int problems, int T, int D, int kind, bool counts, const std::string& name) {
    std::vector<int> w((size_t)problems * T * D), tc(problems), dc(problems);
    for (int p = 0; p < problems; ++p) {
        tc[p] = counts ? (int)(rnd() % (T + 9)) - 4 : T;      // below 0 and above T included
        dc[p] = counts ? (int)(rnd() % (D + 9)) - 4 : D;
        for (int t = 0; t < T; ++t)
            for (int d = 0; d < D; ++d) {
                int v = 0;
                if (kind == 0) v = 1 + (int)(rnd() % YH_ASSIGN_MAX_WEIGHT);
                if (kind == 1) v = (int)(rnd() % 4) * 10;
                if (kind == 2) v = std::abs(t * D / std::max(T, 1) - d) <= 2 && rnd() % 3 ? 1 + (int)(rnd() % 1000) : 0;
                if (kind == 3) v = d == t ? 1000 : (d == t + 1 ? 1001 : 0);
                if (kind == 4) v = (int)(rnd() % 7 - 3) * (YH_ASSIGN_MAX_WEIGHT / 2);
                w[((size_t)p * T + t) * D + d] = v;
            }
    }
    std::vector<int> first_r, first_s;
    for (int threads : {1, 3}) {
        std::vector<int> ros((size_t)problems * T, -9), sor((size_t)problems * D, -9);
        const char* bad = yh_assign_check(w.data(), problems, T, D, ros.data(), sor.data());
        expect(!bad, name + ": " + (bad ? bad : ""));
        yh_assign_host_run(w.data(), problems, T, D, counts ? tc.data() : nullptr, counts ? dc.data() : nullptr,
                           ros.data(), sor.data(), threads);
        for (int p = 0; p < problems; ++p) {
            const int nt = std::min(std::max(tc[p], 0), T), nd = std::min(std::max(dc[p], 0), D);
            const std::vector<int> wp(w.begin() + (size_t)p * T * D, w.begin() + (size_t)(p + 1) * T * D);
            long long total = 0;
            for (int t = 0; t < T; ++t) {
                const int d = ros[(size_t)p * T + t];
                expect(d >= -1 && d < nd && (t < nt || d == -1), name + ": row_of_slot range");
                if (d < 0 || d >= nd) continue;
                expect(sor[(size_t)p * D + d] == t, name + ": not inverse");
                expect(yh_assign_clamp(wp[(size_t)t * D + d]) > 0, name + ": forbidden pair");
                total += yh_assign_clamp(wp[(size_t)t * D + d]);
            }
            for (int d = 0; d < D; ++d) {
                const int t = sor[(size_t)p * D + d];
                expect(t >= -1 && t < nt && (t < 0 || ros[(size_t)p * T + t] == d), name + ": slot_of_row");
            }
            const long long g = greedy_total(wp, nt, nd, D);
            expect(total >= g && (kind != 3 || nt != T || nd != D || T < 2 || total > g), name + ": below the greedy walk");
        }
        if (threads == 1) {
            first_r = ros;
            first_s = sor;
        } else {
            expect(ros == first_r && sor == first_s, name + ": threads differ");
        }
    }
}

void tracker_case(int dim, const std::string& name) {
    const int B = 2, D = 40, T = 24, frames = 6, objects = 28;
    yh_track_params p{0.25f, 0.1f, 0.25f, 0.2f, 0.5f, 0.3f, 3, 1};
    const size_t stream_bytes = dim ? yh_track_reid_stream_bytes(T, dim) : yh_track_stream_words(T) * 4;
    std::vector<std::vector<char>> states(2, std::vector<char>(B * stream_bytes, 0));
    std::vector<float> pos((size_t)B * objects * 2);
    for (float& v : pos) v = 40.0f + (float)(rnd() % 200);
    for (int f = 0; f < frames; ++f) {
        std::vector<float> dets((size_t)B * D * 6);
        std::vector<int> counts(B);
        for (int b = 0; b < B; ++b) {
            counts[b] = f == 3 ? D + 5 : objects;               // once above max_det: clamped
            for (int r = 0; r < D; ++r) {
                float* d = &dets[((size_t)b * D + r) * 6];
                const int o = r % objects;
                const float cx = pos[((size_t)b * objects + o) * 2] + 3.0f * f, cy = pos[((size_t)b * objects + o) * 2 + 1];
                d[0] = cx - 30; d[1] = cy - 40; d[2] = cx + 30; d[3] = cy + 40;
                d[4] = 0.15f + 0.01f * (float)(rnd() % 80);
                d[5] = (float)(o % 2);
            }
        }
        std::vector<float> embed;
        if (dim) {
            embed.resize((size_t)B * D * dim);
            for (float& v : embed) v = (float)(rnd() % 2001) / 1000.0f - 1.0f;
        }
        std::vector<std::vector<int>> ids_of(2);
        for (int run = 0; run < 2; ++run) {                      // threads 1 and 3: the same bytes
            std::vector<float> out((size_t)B * D * 6);
            std::vector<int> ids((size_t)B * D), idx((size_t)B * D), oc(B);
            const char* bad = yh_track_check(dets.data(), counts.data(), B, D, states[run].data(), B, T, &p, D, out.data(),
                                             ids.data(), idx.data(), oc.data());
            expect(!bad, name + ": " + (bad ? bad : ""));
            std::vector<char> ws(dim ? yh_reid_ws_bytes(B, D, T, dim) : 0);
            yh_track_reid_args ra{embed.data(), B * D, dim, nullptr, nullptr, yh_reid_params{0.5f, 0.5f}, ws.data()};
            yh_track_host_run(dets.data(), counts.data(), B, D, nullptr, states[run].data(), B, T, &p, D, out.data(),
                              ids.data(), idx.data(), oc.data(), run ? 3 : 1, dim ? &ra : nullptr, YH_ASSIGN_OPTIMAL);
            ids_of[run] = ids;
        }
        expect(ids_of[0] == ids_of[1] && states[0] == states[1], name + ": threads differ");
    }
}

}  // namespace

int main() {
    int cases = 0;
    const int shapes[][2] = {{1, 1}, {2, 3}, {3, 2}, {0, 5}, {5, 0}, {17, 63}, {40, 64}, {33, 65}, {65, 33}, {70, 70}};
    for (const auto& s : shapes)
        for (int kind : {0, 1, 2, 4})
            for (bool counts : {false, true}) {
                solver_case(3, s[0], s[1], kind, counts,
                            "solver " + std::to_string(s[0]) + "x" + std::to_string(s[1]) + " kind " + std::to_string(kind));
                ++cases;
            }
    solver_case(1, 64, 64, 3, false, "band 64");
    solver_case(2, 128, 128, 1, true, "ties 128");
    solver_case(1, 256, 300, 2, false, "sparse 256x300");
    cases += 3;
    // the argument check: sizes above the caps and below 0, NULL pointers
    int one = 1;
    expect(yh_assign_check(&one, 1, YH_ASSIGN_MAX_SIZE + 1, 1, &one, &one) != nullptr, "T above the cap");
    expect(yh_assign_check(&one, 1, 1, YH_ASSIGN_MAX_SIZE + 1, &one, &one) != nullptr, "D above the cap");
    expect(yh_assign_check(&one, -1, 1, 1, &one, &one) != nullptr, "problems below 0");
    expect(yh_assign_check(&one, 1, -1, 1, &one, &one) != nullptr, "T below 0");
    expect(yh_assign_check(&one, 1, 1, -1, &one, &one) != nullptr, "D below 0");
    expect(yh_assign_check(nullptr, 1, 1, 1, &one, &one) != nullptr, "null weights");
    expect(yh_assign_check(&one, 1, 1, 1, nullptr, &one) != nullptr, "null row_of_slot");
    expect(yh_assign_check(&one, 1, 1, 1, &one, nullptr) != nullptr, "null slot_of_row");
    expect(yh_assign_check(nullptr, 0, 1, 1, nullptr, nullptr) == nullptr, "nothing to do");
    yh_assign_params ap{2, {0, 0, 0}};
    expect(yh_assign_params_check(&ap) != nullptr && yh_assign_params_check(nullptr) != nullptr, "bad mode");
    tracker_case(0, "tracker");
    tracker_case(64, "tracker reid");
    cases += 2;
    std::printf("assignment host twins: %d cases ran, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
