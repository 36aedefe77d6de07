// Host (CPU) twin of the tracking evaluation (csrc/mot.hip), and the argument check both entry
// points share. HIP-free on purpose: this file compiles alone with any C++17 compiler. The rules -
// stated at yh_mot_eval in include/yolo_hip.h - run here one sequence and one threshold at a time;
// the pair arithmetic is csrc/mot_host.h's, the assignments are csrc/assign_host.h's yh_assign_solve.
#include "mot_host.h"

#include <algorithm>
#include <vector>

#include "host_parallel.h"

const char* yh_mot_check(const void* tr, const void* tr_ids, const void* tr_counts, int max_out, const void* gt,
                         const void* gt_ids, const void* gt_counts, int max_gt, int sequences, int frame_cap,
                         const void* thr, int num_thr, int n_gt_ids, int n_tr_ids, int class_aware, const void* out,
                         const void* ignored) {
    if (sequences < 0 || frame_cap < 0 || max_out < 0 || max_gt < 0 || n_gt_ids < 0 || n_tr_ids < 0)
        return "mot_eval: sizes must be >= 0";
    if (max_out > YH_MOT_MAX_ROWS || max_gt > YH_MOT_MAX_ROWS)
        return "mot_eval: max_out or max_gt exceeds YH_MOT_MAX_ROWS (" YH_STR(YH_MOT_MAX_ROWS) ")";
    if (n_gt_ids > YH_MOT_MAX_IDS || n_tr_ids > YH_MOT_MAX_IDS)
        return "mot_eval: n_gt_ids or n_tr_ids exceeds YH_MOT_MAX_IDS (" YH_STR(YH_MOT_MAX_IDS) ")";
    if (frame_cap > YH_MOT_MAX_FRAMES) return "mot_eval: more than YH_MOT_MAX_FRAMES (" YH_STR(YH_MOT_MAX_FRAMES) ") frames";
    if (num_thr < 1 || num_thr > YH_MOT_MAX_THR) return "mot_eval: num_thr must be in [1, " YH_STR(YH_MOT_MAX_THR) "]";
    if (class_aware != 0 && class_aware != 1) return "mot_eval: class_aware must be 0 or 1";
    if (!thr) return "mot_eval: null thr";
    if (sequences > 0 && (!out || !ignored)) return "mot_eval: null output";
    if (sequences > 0 && frame_cap > 0) {
        if (!tr_counts || !gt_counts) return "mot_eval: null counts";
        if (max_out > 0 && (!tr || !tr_ids)) return "mot_eval: null hypotheses";
        if (max_gt > 0 && (!gt || !gt_ids)) return "mot_eval: null ground truth";
    }
    return nullptr;
}

namespace {

// one sequence at one threshold -> its YH_MOT_OUT numbers
void eval_one(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out, const float* gt,
              const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int nf, float a, int n_gt_ids, int n_tr_ids,
              int class_aware, int64_t* o) {
    std::vector<int> prev(n_gt_ids, -1), now(n_gt_ids, -1), last(n_gt_ids, -1), row_of_id(n_tr_ids, -1);
    std::vector<uint16_t> C((size_t)n_gt_ids * n_tr_ids, 0);
    std::vector<int> grow, hrow, mate(max_gt), ros(max_gt), sor(max_out);
    std::vector<char> taken(max_out);
    int64_t tp = 0, idsw = 0, siou = 0, ngt = 0, nhyp = 0;
    for (int f = 0; f < nf; ++f) {
        const int ng = yh_mot_clampi(gt_counts[f], max_gt), nh = yh_mot_clampi(tr_counts[f], max_out);
        const float* G = gt + (size_t)f * max_gt * 5;
        const float* T = tr + (size_t)f * max_out * 6;
        const int32_t* gi = gt_ids + (size_t)f * max_gt;
        const int32_t* ti = tr_ids + (size_t)f * max_out;
        auto weight = [&](int r, int c) { return yh_mot_weight(G + 5 * r, T + 6 * c, class_aware, a); };
        for (int c = 0; c < nh; ++c) {
            taken[c] = 0;
            if (yh_mot_id_ok(ti[c], n_tr_ids)) {
                row_of_id[ti[c]] = c;
                ++nhyp;
            }
        }
        // the overlap counts, and the carry: last frame's pair stays when it is still allowed
        for (int r = 0; r < ng; ++r) {
            mate[r] = -1;
            if (!yh_mot_id_ok(gi[r], n_gt_ids)) continue;
            ++ngt;
            for (int c = 0; c < nh; ++c)
                if (yh_mot_id_ok(ti[c], n_tr_ids) && weight(r, c) > 0) ++C[(size_t)gi[r] * n_tr_ids + ti[c]];
            const int h = prev[gi[r]];
            const int c = h >= 0 ? row_of_id[h] : -1;
            if (c >= 0 && weight(r, c) > 0) {
                mate[r] = c;
                taken[c] = 1;
            }
        }
        // the assignment of the rest
        grow.clear();
        hrow.clear();
        for (int r = 0; r < ng; ++r)
            if (yh_mot_id_ok(gi[r], n_gt_ids) && mate[r] < 0) grow.push_back(r);
        for (int c = 0; c < nh; ++c)
            if (yh_mot_id_ok(ti[c], n_tr_ids) && !taken[c]) hrow.push_back(c);
        if (!grow.empty() && !hrow.empty()) {
            yh_assign_solve((int)grow.size(), (int)hrow.size(), [&](int s, int c) { return weight(grow[s], hrow[c]); },
                            ros.data(), sor.data());
            for (size_t s = 0; s < grow.size(); ++s)
                if (ros[s] >= 0) mate[grow[s]] = hrow[ros[s]];
        }
        // the counts
        for (int r = 0; r < ng; ++r) {
            if (mate[r] < 0) continue;
            const int g = gi[r], h = ti[mate[r]];
            ++tp;
            siou += weight(r, mate[r]) - 1;
            if (last[g] >= 0 && last[g] != h) ++idsw;
            last[g] = h;
            now[g] = h;
        }
        prev.swap(now);
        std::fill(now.begin(), now.end(), -1);
        for (int c = 0; c < nh; ++c)
            if (yh_mot_id_ok(ti[c], n_tr_ids)) row_of_id[ti[c]] = -1;
    }
    int64_t idtp = 0;
    if (n_gt_ids > 0 && n_tr_ids > 0) {
        std::vector<int> idr(n_gt_ids), ids(n_tr_ids);
        auto cw = [&](int g, int t) { return yh_assign_clamp((int)C[(size_t)g * n_tr_ids + t]); };
        yh_assign_solve(n_gt_ids, n_tr_ids, cw, idr.data(), ids.data());
        for (int g = 0; g < n_gt_ids; ++g)
            if (idr[g] >= 0) idtp += C[(size_t)g * n_tr_ids + idr[g]];
    }
    o[YH_MOT_TP] = tp;
    o[YH_MOT_FP] = nhyp - tp;
    o[YH_MOT_FN] = ngt - tp;
    o[YH_MOT_IDSW] = idsw;
    o[YH_MOT_SIOU] = siou;
    o[YH_MOT_IDTP] = idtp;
    o[YH_MOT_GT] = ngt;
    o[YH_MOT_HYP] = nhyp;
}

}  // namespace

void yh_mot_eval_host_run(const float* tr, const int32_t* tr_ids, const int32_t* tr_counts, int max_out,
                          const float* gt, const int32_t* gt_ids, const int32_t* gt_counts, int max_gt, int sequences,
                          int frame_cap, const int32_t* frames, const float* thr, int num_thr, int n_gt_ids,
                          int n_tr_ids, int class_aware, int64_t* out, int32_t* ignored, int threads) {
    const int F = frame_cap;
    yh::parallel_strided(sequences * num_thr, threads, [&](int job) {
        const int s = job / num_thr, a = job % num_thr;
        const int nf = frames ? yh_mot_clampi(frames[s], F) : F;
        const float* T = tr + (size_t)s * F * max_out * 6;
        const float* G = gt + (size_t)s * F * max_gt * 5;
        const int32_t* ti = tr_ids + (size_t)s * F * max_out;
        const int32_t* gi = gt_ids + (size_t)s * F * max_gt;
        const int32_t* tc = tr_counts + (size_t)s * F;
        const int32_t* gc = gt_counts + (size_t)s * F;
        eval_one(T, ti, tc, max_out, G, gi, gc, max_gt, nf, thr[a], n_gt_ids, n_tr_ids, class_aware,
                 out + ((size_t)s * num_thr + a) * YH_MOT_OUT);
        if (a != 0) return;
        int ig = 0, ih = 0;
        for (int f = 0; f < nf; ++f) {
            const int ng = yh_mot_clampi(gc[f], max_gt), nh = yh_mot_clampi(tc[f], max_out);
            for (int r = 0; r < ng; ++r) ig += !yh_mot_id_ok(gi[(size_t)f * max_gt + r], n_gt_ids);
            for (int c = 0; c < nh; ++c) ih += !yh_mot_id_ok(ti[(size_t)f * max_out + c], n_tr_ids);
        }
        ignored[2 * s] = ig;
        ignored[2 * s + 1] = ih;
    });
}
