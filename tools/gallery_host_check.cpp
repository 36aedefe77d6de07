// Stand-alone driver of the identity search's host twins (csrc/gallery_host.cpp), for a sanitizer
// build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/gallery_host_check.cpp yolo-infer-pt_amd/csrc/gallery_host.cpp \
//       yolo-infer-pt_amd/csrc/track_host.cpp -lpthread -o build/gallery_host_check
//   build/gallery_host_check tools/gallery_host_cases.txt
// The case list has one case per line, '#' starts a comment:
//   search <dim> <nq> <n> <k>                 the sizes of tests/_gallery_cases.py's SEARCH_CASES
//   enrol <dim> <capacity> <size> <nq>
// Each case runs on random full-range data in exactly sized heap buffers - rows of 127s beyond the
// size, hidden labels, a zero query, a count that cuts queries off; masks and zero rows for the
// enrolment - with 1, 3 and 100 threads and the three chunkings, against a sort of all scores
// written here. Exit status 0 and no sanitizer report is the result.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gallery_host.h"

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

void search_case(int dim, int nq, int n, int k, const std::string& name) {
    const int capacity = n + 7;
    std::vector<int8_t> gallery((size_t)capacity * dim), q((size_t)nq * dim);
    for (int8_t& v : gallery) v = (int8_t)(rnd() & 0xFF);
    for (int g = n / 2; g < n; ++g) std::memcpy(&gallery[(size_t)g * dim], &gallery[(size_t)(g - n / 2) * dim], dim);
    std::fill(gallery.begin() + (size_t)n * dim, gallery.end(), (int8_t)127);
    for (int8_t& v : q) v = (int8_t)(rnd() & 0xFF);
    if (nq) std::fill(q.begin(), q.begin() + dim, (int8_t)127);
    if (nq > 2) std::fill(q.begin() + 2 * (size_t)dim, q.begin() + 3 * (size_t)dim, (int8_t)0);
    std::vector<int32_t> labels(capacity);
    for (int32_t& v : labels) v = rnd() % 5 ? (int32_t)(rnd() % 1000) : -1 - (int32_t)(rnd() % 1000);
    const int32_t size = n, count = nq > 5 ? nq - 3 : nq + 2;
    // the reference: every score, sorted
    std::vector<int32_t> want_s((size_t)nq * k, INT32_MIN), want_i((size_t)nq * k, -1);
    for (int i = 0; i < std::min(nq, count); ++i) {
        if (i == 2) continue;
        std::vector<std::pair<int64_t, int>> all;
        for (int g = 0; g < n; ++g) {
            if (labels[g] < 0) continue;
            int32_t acc = 0;
            for (int e = 0; e < dim; ++e) acc += (int32_t)q[(size_t)i * dim + e] * gallery[(size_t)g * dim + e];
            all.push_back({-(int64_t)acc, g});
        }
        std::sort(all.begin(), all.end());
        for (int j = 0; j < k && j < (int)all.size(); ++j) {
            want_s[(size_t)i * k + j] = (int32_t)-all[j].first;
            want_i[(size_t)i * k + j] = all[j].second;
        }
    }
    for (int chunk_rows : {0, 64, 128})
        for (int threads : {1, 3, 100}) {
            const size_t ws_bytes = yh_gal_ws_bytes(capacity, nq, k, chunk_rows);
            std::vector<char> ws(ws_bytes);
            std::vector<int32_t> scores((size_t)nq * k, -9), index((size_t)nq * k, -9);
            const char* bad = yh_gallery_search_check(gallery.data(), capacity, dim, q.data(), nq, k, chunk_rows,
                                                      scores.data(), index.data(), ws.data(), ws_bytes);
            expect(!bad, name + ": " + (bad ? bad : ""));
            yh_gallery_search_host_run(gallery.data(), labels.data(), &size, capacity, dim, q.data(), nq, &count, k,
                                       scores.data(), index.data(), threads);
            expect(scores == want_s && index == want_i, name + ": differs from the sort");
        }
}

void enrol_case(int dim, int capacity, int size0, int nq, const std::string& name) {
    std::vector<int8_t> gallery((size_t)capacity * dim, 1), q((size_t)nq * dim);
    for (int8_t& v : q) v = (int8_t)(rnd() & 0xFF);
    for (int i = 1; i < nq; i += 7) std::fill(q.begin() + (size_t)i * dim, q.begin() + (size_t)(i + 1) * dim, (int8_t)0);
    std::vector<int32_t> labels(capacity, -7), take(nq), rows(nq, -9);
    for (int32_t& v : take) v = (int32_t)(rnd() % 3) - 1;
    int32_t size = size0, next = 100;
    const int32_t count = nq > 3 ? nq - 2 : nq;
    const char* bad = yh_gallery_enrol_check(gallery.data(), labels.data(), &size, capacity, dim, q.data(), nq, nullptr,
                                             &next, rows.data());
    expect(!bad, name + ": " + (bad ? bad : ""));
    yh_gallery_enrol_host_run(gallery.data(), labels.data(), &size, capacity, dim, q.data(), nq, &count, take.data(),
                              nullptr, &next, rows.data());
    int n = std::min(std::max(size0, 0), capacity), label = 100;
    for (int i = 0; i < nq; ++i) {
        const bool zero = i % 7 == 1;
        const bool in = i < count && take[i] != 0 && !zero && n < capacity;
        expect(rows[i] == (in ? n : -1), name + ": rows_out");
        if (!in) continue;
        expect(std::memcmp(&gallery[(size_t)n * dim], &q[(size_t)i * dim], dim) == 0 && labels[n] == label, name + ": row");
        ++n;
        ++label;
    }
    expect(size == n && next == label, name + ": size / next_label");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: %s <case list>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    int cases = 0;
    for (std::string line; std::getline(in, line);) {
        std::istringstream ls(line.substr(0, line.find('#')));
        std::string kind;
        int a = 0, b = 0, c = 0, d = 0;
        if (!(ls >> kind)) continue;
        if (!(ls >> a >> b >> c >> d) || (kind != "search" && kind != "enrol")) {
            std::printf("bad line: %s\n", line.c_str());
            return 2;
        }
        if (kind == "search") search_case(a, b, c, d, line);
        else enrol_case(a, b, c, d, line);
        ++cases;
    }
    std::printf("gallery host twins: %d cases ran, %d failures\n", cases, fails);
    return fails || !cases ? 1 : 0;
}
