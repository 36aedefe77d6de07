// Stand-alone driver of the appearance stage's host twins (csrc/track_host.cpp), for a sanitizer
// build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/reid_host_check.cpp yolo-infer-pt_amd/csrc/track_host.cpp \
//       -lpthread -o build/reid_host_check && build/reid_host_check
// It runs the shapes of the tests' case list on random data - quantise with the special rows and
// every count, the similarity at ra, rb in {1, 31, 32, 33, 70} with strided blocks and an index
// out of range, and 12-frame yh_track_reid sequences at (1, 1), (33, 31), (256, 70) and (256, 300)
// with features cut off by feat_counts, capacity and embed_total - each with 1, 3 and 100 threads,
// in exactly sized heap buffers, and compares the bytes of the thread counts. Exit status 0 and
// no sanitizer report is the result.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "track_host.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xFFFFFF) / 16777216.0f; }

int fails = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

void quantize_cases(int dim) {
    const int rows = 24;
    std::vector<float> e((size_t)rows * dim);
    for (float& v : e) v = uni(-1.0f, 1.0f);
    auto row = [&](int r) { return e.data() + (size_t)r * dim; };
    std::fill(row(1), row(1) + dim, 0.0f);
    std::fill(row(2), row(2) + dim, 0.0f);
    row(2)[5] = -3.5f;
    row(3)[7] = std::numeric_limits<float>::infinity();
    row(4)[0] = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < dim; ++i) row(6)[i] *= 1e-42f;
    std::fill(row(7), row(7) + dim, 0.0f);
    row(7)[3] = std::numeric_limits<float>::denorm_min();
    std::fill(row(9), row(9) + dim, 3e38f);
    const int counts[] = {0, 9, 24, 99, -3};
    std::vector<int8_t> first;
    for (int threads : {1, 3, 100}) {
        std::vector<int8_t> all;
        for (int ci = -1; ci < 5; ++ci) {
            std::vector<int8_t> q((size_t)rows * dim, 55);
            yh_embed_quantize_host_run(e.data(), rows, dim, ci < 0 ? nullptr : &counts[ci], q.data(), threads);
            all.insert(all.end(), q.begin(), q.end());
        }
        if (first.empty()) first = all;
        expect(first == all, "quantize: thread counts differ");
    }
    expect(first[(size_t)2 * dim + 5] == -127 && first[(size_t)7 * dim + 3] == 127, "quantize: single elements");
}

void similarity_cases(int dim) {
    const int sizes[] = {1, 31, 32, 33, 70};
    for (int ra : sizes)
        for (int rb : sizes) {
            const size_t stride = (size_t)(ra + 3) * dim;
            std::vector<int8_t> a(4 * stride + (size_t)ra * dim), b((size_t)3 * rb * dim);   // 5 blocks, the last one short
            for (int8_t& v : a) v = (int8_t)(rnd() & 0xFF);
            for (int8_t& v : b) v = (int8_t)(rnd() & 0xFF);
            std::fill(a.begin() + stride, a.begin() + stride + dim, (int8_t)-128);
            std::fill(b.begin(), b.begin() + dim, (int8_t)-128);
            const int index[3] = {4, 7, 1};
            std::vector<int32_t> first;
            for (int threads : {1, 3, 100}) {
                std::vector<int32_t> out((size_t)3 * ra * rb, -9);
                yh_embed_similarity_host_run(a.data(), stride, 5, index, b.data(), 3, ra, rb, dim, out.data(), threads);
                if (first.empty()) first = out;
                expect(first == out, "similarity: thread counts differ");
            }
            bool zero = true;
            for (int i = 0; i < ra * rb; ++i) zero = zero && first[(size_t)ra * rb + i] == 0;
            expect(zero, "similarity: the block out of range is not zero");
        }
}

void track_cases(int max_tracks, int max_det, int dim, int frames) {
    const int B = 3, streams = 3, objects = std::min(max_det, 40);
    yh_track_params p{0.25f, 0.1f, 0.25f, 0.2f, 0.5f, 0.3f, 3, 1};
    const yh_reid_params rp{0.3f, 0.0f};
    std::vector<float> proto((size_t)B * objects * dim);
    for (float& v : proto) v = uni(-1.0f, 1.0f);
    std::vector<float> px((size_t)B * objects), py((size_t)B * objects);
    for (size_t i = 0; i < px.size(); ++i) px[i] = uni(40, 360), py[i] = uni(40, 360);
    // the frames, made once
    struct Fr {
        std::vector<float> dets, embed;
        std::vector<int> counts, fc;
        int total;
        bool use_total;
    };
    std::vector<Fr> seq(frames);
    for (int f = 0; f < frames; ++f) {
        Fr& fr = seq[f];
        fr.dets.assign((size_t)B * max_det * 6, std::numeric_limits<float>::quiet_NaN());
        fr.counts.resize(B);
        fr.fc.resize(B);
        int nfeat = 0;
        for (int b = 0; b < B; ++b) {
            const int n = (int)(rnd() % (objects + 1));
            fr.counts[b] = f == 2 ? n + 5 : n;                       // above max_det sometimes: clamped
            const int c = std::min(fr.counts[b], max_det);
            for (int r = 0; r < c; ++r) {
                const int o = r % objects;
                const float cx = px[(size_t)b * objects + o] + 3.0f * f + uni(-2, 2), cy = py[(size_t)b * objects + o] + uni(-2, 2);
                float* d = &fr.dets[((size_t)b * max_det + r) * 6];
                d[0] = cx - 30; d[1] = cy - 40; d[2] = cx + 30; d[3] = cy + 40;
                d[4] = uni(0.05f, 0.95f);
                d[5] = (float)(o % 3);
            }
            fr.fc[b] = f % 3 == 1 ? (int)(rnd() % (c + 1)) : c + (f % 3 == 2 ? 4 : 0);
            const int nf = std::min(fr.fc[b], c);
            for (int r = 0; r < nf; ++r) {
                const float* pr = &proto[((size_t)b * objects + r % objects) * dim];
                for (int i = 0; i < dim; ++i) fr.embed.push_back(pr[i] + uni(-0.3f, 0.3f));
                if (rnd() % 16 == 0) fr.embed[fr.embed.size() - 1] = std::numeric_limits<float>::infinity();
            }
            nfeat += nf;
        }
        fr.use_total = f % 4 == 1;
        fr.total = std::max(nfeat - 2, 0);
        if (f % 4 == 2 && nfeat > 3) fr.embed.resize((size_t)(nfeat - 3) * dim);     // a short capacity
    }
    const size_t state_bytes = (size_t)streams * yh_track_reid_stream_bytes(max_tracks, dim);
    const size_t ws_bytes = yh_reid_ws_bytes(B, max_det, max_tracks, dim);
    std::vector<char> first_state;
    std::vector<float> first_out;
    for (int threads : {1, 3, 100}) {
        std::vector<char> state(state_bytes, 0), ws(ws_bytes, 0x5A);
        std::vector<float> outs;
        for (int f = 0; f < frames; ++f) {
            Fr& fr = seq[f];
            const int max_out = max_det;
            std::vector<float> out((size_t)B * max_out * 6, -7.0f);
            std::vector<int> ids((size_t)B * max_out, -7), di((size_t)B * max_out, -7), oc(B, -7);
            const int sid[3] = {f % 2 ? 2 : 1, f % 2 ? 7 : 0, f % 2 ? 0 : 2};       // 7: no such stream
            const int capacity = (int)(fr.embed.size() / dim);
            const yh_track_reid_args ra{f == 5 ? nullptr : fr.embed.data(), capacity, dim, fr.fc.data(),
                                        fr.use_total ? &fr.total : nullptr, rp, ws.data()};
            const char* bad = yh_track_check(fr.dets.data(), fr.counts.data(), B, max_det, state.data(), streams, max_tracks,
                                             &p, max_out, out.data(), ids.data(), di.data(), oc.data());
            expect(!bad, bad ? bad : "");
            bad = yh_track_reid_check(B, max_det, max_tracks, capacity, dim, &rp, ws.data(), ws_bytes);
            expect(!bad, bad ? bad : "");
            yh_track_host_run(fr.dets.data(), fr.counts.data(), B, max_det, sid, state.data(), streams, max_tracks, &p,
                              max_out, out.data(), ids.data(), di.data(), oc.data(), threads, &ra);
            outs.insert(outs.end(), out.begin(), out.end());
            for (int v : ids) outs.push_back((float)v);
            for (int v : oc) outs.push_back((float)v);
        }
        if (first_state.empty()) first_state = state, first_out = outs;
        expect(first_state == state, "track_reid: states of the thread counts differ");
        expect(std::memcmp(first_out.data(), outs.data(), outs.size() * 4) == 0, "track_reid: outputs differ");
    }
    bool any = false;
    for (size_t i = yh_track_stream_words(max_tracks) * 4; i < yh_track_reid_stream_bytes(max_tracks, dim); ++i)
        any = any || first_state[i] != 0;
    expect(any || max_tracks == 1, "track_reid: no gallery was written");
}

}  // namespace

int main() {
    for (int dim : {64, 1280}) quantize_cases(dim);
    for (int dim : {64, 128, 1280}) similarity_cases(dim);
    track_cases(1, 1, 64, 12);
    track_cases(33, 31, 64, 12);
    track_cases(256, 70, 1280, 12);
    track_cases(256, 300, 64, 6);
    std::printf(fails ? "%d failures\n" : "reid host twins: all cases ran, %d failures\n", fails);
    return fails ? 1 : 0;
}
