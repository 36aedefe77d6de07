// Host (CPU) twin of the HOTA evaluation (csrc/hota.hip), and the argument check both entry points
// share. HIP-free on purpose: this file compiles alone with any C++17 compiler. The rules - stated
// at yh_hota_eval in include/yolo_hip.h - run here one sequence at a time, two walks over its frames;
// the arithmetic is csrc/hota_host.h's, the assignment is csrc/assign_host.h's yh_assign_solve. Where
// the kernels keep the matched pairs of every level in a dense workspace, the twin lists them and
// sorts the list: every sum is an integer, so the order is free.
#include "hota_host.h"

#include <algorithm>
#include <vector>

#include "host_parallel.h"

const char* yh_hota_check(const void* tr, const void* tr_ids, const void* tr_counts, int max_out, const void* gt,
                          const void* gt_ids, const void* gt_counts, int max_gt, int sequences, int frame_cap,
                          const void* thr, int num_thr, int n_gt_ids, int n_tr_ids, int class_aware, const void* out,
                          const void* rows, const void* ignored) {
    if (sequences < 0 || frame_cap < 0 || max_out < 0 || max_gt < 0 || n_gt_ids < 0 || n_tr_ids < 0)
        return "hota_eval: sizes must be >= 0";
    if (max_out > YH_MOT_MAX_ROWS || max_gt > YH_MOT_MAX_ROWS)
        return "hota_eval: max_out or max_gt exceeds YH_MOT_MAX_ROWS (" YH_STR(YH_MOT_MAX_ROWS) ")";
    if (n_gt_ids > YH_MOT_MAX_IDS || n_tr_ids > YH_MOT_MAX_IDS)
        return "hota_eval: n_gt_ids or n_tr_ids exceeds YH_MOT_MAX_IDS (" YH_STR(YH_MOT_MAX_IDS) ")";
    if (frame_cap > YH_HOTA_MAX_FRAMES) return "hota_eval: more than YH_HOTA_MAX_FRAMES (" YH_STR(YH_HOTA_MAX_FRAMES) ") frames";
    if (num_thr < 1 || num_thr > YH_HOTA_MAX_THR) return "hota_eval: num_thr must be in [1, " YH_STR(YH_HOTA_MAX_THR) "]";
    if (class_aware != 0 && class_aware != 1) return "hota_eval: class_aware must be 0 or 1";
    if (!thr) return "hota_eval: null thr";
    if (sequences > 0 && (!out || !rows || !ignored)) return "hota_eval: null output";
    if (sequences > 0 && frame_cap > 0) {
        if (!tr_counts || !gt_counts) return "hota_eval: null counts";
        if (max_out > 0 && (!tr || !tr_ids)) return "hota_eval: null hypotheses";
        if (max_gt > 0 && (!gt || !gt_ids)) return "hota_eval: null ground truth";
    }
    return nullptr;
}

namespace {

// one sequence -> its (num_thr, 8) numbers, its two row counts and its two ignored counts
void eval_one(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out, const float* gt,
              const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int nf, const float* thr, int num_thr,
              int n_gt_ids, int n_tr_ids, int class_aware, int64_t* out, int64_t* rows, int32_t* ignored) {
    const size_t nti = (size_t)n_tr_ids;
    std::vector<uint32_t> P((size_t)n_gt_ids * nti, 0), cnt_g(n_gt_ids, 0), cnt_t(n_tr_ids, 0);
    std::vector<int> sim((size_t)max_gt * max_out), R(max_gt), C(max_out), ros(max_gt), sor(max_out);
    std::vector<uint16_t> w((size_t)max_gt * max_out);
    std::vector<uint64_t> matched;                       // (g * n_tr_ids + t) << 8 | level, one per matched pair
    std::vector<int64_t> ctr((size_t)num_thr * YH_HOTA_CTR, 0);
    int64_t n_gt = 0, n_hyp = 0, ign_g = 0, ign_h = 0;

    // the similarities of frame f into sim (0 where an id is out of range) -> its counts
    int ng = 0, nh = 0;
    const float *G = nullptr, *T = nullptr;
    const int32_t *gi = nullptr, *ti = nullptr;
    auto frame = [&](int f) {
        ng = yh_hota_clampi(gt_counts[f], max_gt);
        nh = yh_hota_clampi(tr_counts[f], max_out);
        G = gt + (size_t)f * max_gt * 5;
        T = tr + (size_t)f * max_out * 6;
        gi = gt_ids + (size_t)f * max_gt;
        ti = tr_ids + (size_t)f * max_out;
        for (int r = 0; r < ng; ++r)
            for (int c = 0; c < nh; ++c)
                sim[(size_t)r * nh + c] = yh_hota_id_ok(gi[r], n_gt_ids) && yh_hota_id_ok(ti[c], n_tr_ids)
                                              ? yh_hota_pair_sim(G + 5 * r, T + 6 * c, class_aware)
                                              : 0;
    };

    // pass A: the alignment sums
    for (int f = 0; f < nf; ++f) {
        frame(f);
        for (int c = 0; c < nh; ++c) {
            C[c] = 0;
            const bool ok = yh_hota_id_ok(ti[c], n_tr_ids);
            n_hyp += ok;
            ign_h += !ok;
            if (ok) ++cnt_t[ti[c]];
        }
        for (int r = 0; r < ng; ++r) {
            const bool ok = yh_hota_id_ok(gi[r], n_gt_ids);
            n_gt += ok;
            ign_g += !ok;
            if (ok) ++cnt_g[gi[r]];
            R[r] = 0;
            for (int c = 0; c < nh; ++c) {
                R[r] += sim[(size_t)r * nh + c];
                C[c] += sim[(size_t)r * nh + c];
            }
        }
        for (int r = 0; r < ng; ++r)
            for (int c = 0; c < nh; ++c) {
                const int s = sim[(size_t)r * nh + c];
                if (s > 0) P[(size_t)gi[r] * nti + ti[c]] += yh_hota_jaccard(s, R[r], C[c]);
            }
    }

    // pass B: the matching of every frame on the aligned weights
    for (int f = 0; f < nf; ++f) {
        frame(f);
        if (ng == 0 || nh == 0) continue;
        for (int r = 0; r < ng; ++r)
            for (int c = 0; c < nh; ++c) {
                const int s = sim[(size_t)r * nh + c];
                int v = 0;
                if (s > 0) {
                    const int g = gi[r], t = ti[c];
                    v = yh_hota_weight(yh_hota_align(P[(size_t)g * nti + t], cnt_g[g], cnt_t[t]), s);
                }
                w[(size_t)r * nh + c] = (uint16_t)v;
            }
        const int n = nh;
        yh_assign_solve(ng, nh, [&](int r, int c) { return (int)w[(size_t)r * n + c]; }, ros.data(), sor.data());
        for (int r = 0; r < ng; ++r) {
            const int c = ros[r];
            if (c < 0) continue;
            const int level = yh_hota_reached(yh_hota_iou(G + 5 * r, T + 6 * c), thr, num_thr) - 1;
            if (level < 0) continue;
            ctr[(size_t)level * YH_HOTA_CTR + YH_HOTA_C_TP] += 1;
            ctr[(size_t)level * YH_HOTA_CTR + YH_HOTA_C_LOC] += sim[(size_t)r * nh + c];
            matched.push_back((uint64_t)((size_t)gi[r] * nti + ti[c]) << 8 | (uint64_t)level);
        }
    }

    // closing: per identity pair the matches of every level, summed from the top level down
    std::sort(matched.begin(), matched.end());
    for (size_t i = 0; i < matched.size();) {
        const uint64_t pair = matched[i] >> 8;
        uint32_t h[YH_HOTA_MAX_THR] = {};
        for (; i < matched.size() && (matched[i] >> 8) == pair; ++i) ++h[matched[i] & 255];
        const uint32_t cg = cnt_g[pair / nti], ct = cnt_t[pair % nti];
        uint32_t m = 0;
        for (int b = num_thr - 1; b >= 0; --b) {
            m += h[b];
            if (m == 0) continue;
            uint64_t a, re, pr;
            yh_hota_terms(m, cg, ct, &a, &re, &pr);
            int64_t* k = &ctr[(size_t)b * YH_HOTA_CTR];
            k[YH_HOTA_C_ASSA] += (int64_t)a;
            k[YH_HOTA_C_ASSRE] += (int64_t)re;
            k[YH_HOTA_C_ASSPR] += (int64_t)pr;
            k[YH_HOTA_C_PAIRS] += 1;
        }
    }

    for (int a = 0; a < num_thr; ++a) {
        const int rank = yh_hota_rank(thr, num_thr, a);
        int64_t* o = out + (size_t)a * YH_HOTA_OUT;
        int64_t tp = 0, loc = 0;
        for (int b = rank; b < num_thr; ++b) {
            tp += ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_TP];
            loc += ctr[(size_t)b * YH_HOTA_CTR + YH_HOTA_C_LOC];
        }
        const int64_t* k = rank < num_thr ? &ctr[(size_t)rank * YH_HOTA_CTR] : nullptr;
        o[YH_HOTA_TP] = tp;
        o[YH_HOTA_FP] = n_hyp - tp;
        o[YH_HOTA_FN] = n_gt - tp;
        o[YH_HOTA_LOC] = loc;
        o[YH_HOTA_ASSA] = k ? k[YH_HOTA_C_ASSA] : 0;
        o[YH_HOTA_ASSRE] = k ? k[YH_HOTA_C_ASSRE] : 0;
        o[YH_HOTA_ASSPR] = k ? k[YH_HOTA_C_ASSPR] : 0;
        o[YH_HOTA_PAIRS] = k ? k[YH_HOTA_C_PAIRS] : 0;
    }
    rows[0] = n_gt;
    rows[1] = n_hyp;
    ignored[0] = (int32_t)ign_g;
    ignored[1] = (int32_t)ign_h;
}

}  // namespace

void yh_hota_eval_host_run(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out,
                           const float* gt, const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int sequences,
                           int frame_cap, const int32_t* frames, const float* thr, int num_thr, int n_gt_ids,
                           int n_tr_ids, int class_aware, int64_t* out, int64_t* rows, int32_t* ignored, int threads) {
    const int F = frame_cap;
    yh::parallel_strided(sequences, threads, [&](int s) {
        const int nf = frames ? yh_hota_clampi(frames[s], F) : F;
        eval_one(tr + (size_t)s * F * max_out * 6, tr_ids + (size_t)s * F * max_out, tr_counts + (size_t)s * F, max_out,
                 gt + (size_t)s * F * max_gt * 5, gt_ids + (size_t)s * F * max_gt, gt_counts + (size_t)s * F, max_gt, nf,
                 thr, num_thr, n_gt_ids, n_tr_ids, class_aware, out + (size_t)s * num_thr * YH_HOTA_OUT, rows + 2 * s,
                 ignored + 2 * s);
    });
}
