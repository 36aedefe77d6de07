// Stand-alone driver of the HOTA evaluation's host twin (csrc/hota_host.cpp), for a sanitizer build
// on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -Iinclude -Iyolo-infer-pt_amd/csrc tools/hota_host_check.cpp yolo-infer-pt_amd/csrc/hota_host.cpp \
//       -lpthread -o build/hota_host_check       (make hota_host_check)
//   build/hota_host_check
// Every case runs on exactly sized heap buffers, so a read or write one element beyond a frame's
// counts, the inputs or the outputs is a report: row counts 0, 1, 63, 64, 65 and 256 mixed within a
// sequence, counts above the sizes and below 0, ids outside the range, no identities at all,
// `frames` shorter than F and NULL, 1, 19 and 32 thresholds in a shuffled order, class_aware 0 and 1,
// threads 1 and 3 (the same bytes); then the identities every result obeys, the quotient that is
// taken apart, and the argument check. Exit status 0 and no sanitizer report is the result.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "hota_host.h"

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

void run_case(int S, int F, int max_gt, int max_out, int num_thr, int n_gt_ids, int n_tr_ids, int class_aware,
              bool with_frames, const std::string& name) {
    const int rows[] = {0, 1, 63, 64, 65, 256};
    std::vector<float> gt((size_t)S * F * max_gt * 5), tr((size_t)S * F * max_out * 6), thr(num_thr);
    std::vector<int32_t> gi((size_t)S * F * max_gt), ti((size_t)S * F * max_out), gc((size_t)S * F), tc((size_t)S * F), frames(S);
    for (int a = 0; a < num_thr; ++a) thr[a] = 0.05f + 0.9f * (float)((a * 7) % num_thr) / (float)std::max(num_thr - 1, 1);
    for (int s = 0; s < S; ++s) {
        frames[s] = s % 2 ? F : (int)(rnd() % (F + 3)) - 1;       // below 0 and above F included
        for (int f = 0; f < F; ++f) {
            const size_t sf = (size_t)s * F + f;
            gc[sf] = std::min(rows[rnd() % 6], max_gt) + (rnd() % 8 == 0 ? (int)(rnd() % 7) - 3 : 0);
            tc[sf] = std::min(rows[rnd() % 6], max_out) + (rnd() % 8 == 0 ? (int)(rnd() % 7) - 3 : 0);
            for (int r = 0; r < max_gt; ++r) {                    // object r sits in cell r of a grid, drifting
                float* g = &gt[(sf * max_gt + r) * 5];
                g[0] = 40.0f * (float)(r % 16) + 3.0f * (float)f;
                g[1] = 60.0f * (float)(r / 16);
                g[2] = g[0] + 50.0f;
                g[3] = g[1] + 50.0f;
                g[4] = (float)(r % 2);
                gi[sf * max_gt + r] = rnd() % 20 == 0 ? (rnd() % 2 ? -1 : n_gt_ids + (int)(rnd() % 5)) : (n_gt_ids ? (r + s) % n_gt_ids : 0);
            }
            for (int c = 0; c < max_out; ++c) {                   // hypothesis c follows object c (a trade late on)
                const int o = f >= F / 2 && c < 2 ? 1 - c : c;
                float* t = &tr[(sf * max_out + c) * 6];
                const bool exact = rnd() % 4 == 0;                // a quarter lies exactly on its object: s = 65536
                t[0] = 40.0f * (float)(o % 16) + 3.0f * (float)f + (exact ? 0.0f : (float)(rnd() % 13) - 6.0f);
                t[1] = 60.0f * (float)(o / 16) + (exact ? 0.0f : (float)(rnd() % 13) - 6.0f);
                t[2] = t[0] + 50.0f;
                t[3] = t[1] + 50.0f;
                t[4] = 0.5f;
                t[5] = (float)((o + (rnd() % 10 == 0)) % 2);
                ti[sf * max_out + c] = rnd() % 20 == 0 ? (rnd() % 2 ? -1 : n_tr_ids + (int)(rnd() % 5)) : (n_tr_ids ? (c * 7 + 3) % n_tr_ids : 0);
            }
        }
    }
    const char* bad = yh_hota_check(tr.data(), ti.data(), tc.data(), max_out, gt.data(), gi.data(), gc.data(), max_gt, S, F,
                                    thr.data(), num_thr, n_gt_ids, n_tr_ids, class_aware, thr.data(), thr.data(), thr.data());
    expect(!bad, name + ": " + (bad ? bad : ""));
    std::vector<int64_t> first, first_rows;
    std::vector<int32_t> first_ign;
    for (int threads : {1, 3}) {
        std::vector<int64_t> out((size_t)S * num_thr * YH_HOTA_OUT, -9), nrows((size_t)S * 2, -9);
        std::vector<int32_t> ign((size_t)S * 2, -9);
        yh_hota_eval_host_run(tr.data(), ti.data(), tc.data(), max_out, gt.data(), gi.data(), gc.data(), max_gt, S, F,
                              with_frames ? frames.data() : nullptr, thr.data(), num_thr, n_gt_ids, n_tr_ids, class_aware,
                              out.data(), nrows.data(), ign.data(), threads);
        for (int s = 0; s < S; ++s)
            for (int a = 0; a < num_thr; ++a) {
                const int64_t* o = &out[((size_t)s * num_thr + a) * YH_HOTA_OUT];
                const int64_t tp = o[YH_HOTA_TP], one = (int64_t)1 << YH_HOTA_ASS_SHIFT;
                expect(tp >= 0 && tp + o[YH_HOTA_FN] == nrows[2 * s] && tp + o[YH_HOTA_FP] == nrows[2 * s + 1],
                       name + ": TP + FN = GT, TP + FP = HYP");
                expect(o[YH_HOTA_LOC] >= 0 && o[YH_HOTA_LOC] <= YH_HOTA_ONE * tp, name + ": LOC");
                expect(o[YH_HOTA_PAIRS] >= 0 && o[YH_HOTA_PAIRS] <= tp, name + ": PAIRS");
                // sum m^2 / (n_g + n_t - m) <= sum m = TP, and the union is the largest of the three denominators
                expect(o[YH_HOTA_ASSA] >= 0 && o[YH_HOTA_ASSA] <= o[YH_HOTA_ASSRE] && o[YH_HOTA_ASSA] <= o[YH_HOTA_ASSPR], name + ": ASSA");
                expect(o[YH_HOTA_ASSRE] <= one * tp && o[YH_HOTA_ASSPR] <= one * tp, name + ": ASSRE, ASSPR");
                // a threshold that is not below another one is met by no more pairs
                for (int b = 0; b < num_thr; ++b)
                    if (thr[b] >= thr[a]) expect(out[((size_t)s * num_thr + b) * YH_HOTA_OUT] <= tp, name + ": TP falls with the threshold");
            }
        for (int32_t v : ign) expect(v >= 0, name + ": ignored");
        if (threads == 1) {
            first = out;
            first_rows = nrows;
            first_ign = ign;
        } else {
            expect(out == first && nrows == first_rows && ign == first_ign, name + ": threads differ");
        }
    }
}

}  // namespace

int main() {
    int cases = 0;
    for (int class_aware : {0, 1})
        for (bool with_frames : {false, true}) {
            run_case(2, 1, 64, 65, 1, 70, 80, class_aware, with_frames, "one frame");
            run_case(3, 7, 256, 256, 19, 300, 320, class_aware, with_frames, "mixed rows");
            run_case(2, 7, 5, 3, 32, 6, 8, class_aware, with_frames, "small");
            run_case(1, 4, 8, 8, 2, 0, 0, class_aware, with_frames, "no identities");
            run_case(1, 3, 0, 4, 1, 4, 4, class_aware, with_frames, "no ground truth rows");
            run_case(0, 3, 4, 4, 1, 4, 4, class_aware, with_frames, "no sequences");
            run_case(2, 3, 0, 0, 2, 4, 4, class_aware, with_frames, "no rows on either side");
            cases += 7;
        }
    // the quotient whose numerator may be 2^32
    for (uint32_t den : {65536u, 65537u, 98304u, 131071u, 131072u, 1u << 24, (1u << 25) - 1u})
        for (uint32_t num : {1u, 65535u, 65536u})
            expect(yh_hota_div16(num, den) == (uint32_t)(((uint64_t)num << 16) / den), "div16");
    float one = 0.5f;
    auto check = [&](int max_out, int max_gt, int S, int F, int num_thr, int ng, int nt, int ca, const void* p) {
        return yh_hota_check(p, p, p, max_out, p, p, p, max_gt, S, F, p, num_thr, ng, nt, ca, p, p, p);
    };
    expect(check(4, 4, 1, 1, 1, 4, 4, 1, &one) == nullptr, "acceptable arguments");
    expect(check(YH_MOT_MAX_ROWS + 1, 4, 1, 1, 1, 4, 4, 1, &one) != nullptr, "max_out above the cap");
    expect(check(4, YH_MOT_MAX_ROWS + 1, 1, 1, 1, 4, 4, 1, &one) != nullptr, "max_gt above the cap");
    expect(check(4, 4, 1, YH_HOTA_MAX_FRAMES + 1, 1, 4, 4, 1, &one) != nullptr, "F above the cap");
    expect(check(4, 4, 1, 1, 0, 4, 4, 1, &one) != nullptr && check(4, 4, 1, 1, YH_HOTA_MAX_THR + 1, 4, 4, 1, &one) != nullptr, "num_thr");
    expect(check(4, 4, 1, 1, 1, YH_MOT_MAX_IDS + 1, 4, 1, &one) != nullptr, "n_gt_ids above the cap");
    expect(check(4, 4, 1, 1, 1, 4, YH_MOT_MAX_IDS + 1, 1, &one) != nullptr, "n_tr_ids above the cap");
    expect(check(4, 4, -1, 1, 1, 4, 4, 1, &one) != nullptr && check(4, -1, 1, 1, 1, 4, 4, 1, &one) != nullptr, "negative sizes");
    expect(check(4, 4, 1, 1, 1, 4, 4, 2, &one) != nullptr, "class_aware");
    expect(check(4, 4, 1, 1, 1, 4, 4, 1, nullptr) != nullptr, "null pointers");
    std::printf("HOTA evaluation host twin: %d cases ran, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
