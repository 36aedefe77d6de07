// Host (CPU) twin of the weighted boxes fusion (csrc/fuse.hip), and the argument check both entry
// points share. HIP-free: this file compiles alone with any C++17 compiler (build it with
// -ffp-contract=off, as the device file is). The arithmetic of a candidate and of a cluster is in
// csrc/fuse_host.h, shared with the kernel; the semantics are stated in include/yolo_hip.h.
//
// Per image: the candidates are sorted by yh_fuse_cand_key (class, s descending, position), each
// class segment is walked in that order - a candidate joins the cluster whose fused box has the
// largest IoU with it (ties: the oldest) if that IoU exceeds the threshold, else it opens one - and
// the clusters of all classes are written by yh_fuse_out_key (score descending, class, creation).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "fuse_host.h"
#include "host_parallel.h"

namespace {

struct Cand {
    uint64_t key;
    yh_fuse_box b;
    float s;
};

struct Cluster {
    yh_fuse_sums sums;
    yh_fuse_box f;
    float area;
};

void fuse_image(const float* dets, const int* counts, int max_det, const float* group_xf, const float* group_weight,
                int lo, int hi, float W, float H, double iou, float skip, int max_out, float* out, int* out_count) {
    std::fill(out, out + (size_t)max_out * 6, 0.0f);
    float wtot = 0.0f;
    std::vector<Cand> c;
    for (int g = lo; g < hi; ++g) {
        wtot = wtot + group_weight[g];
        const int cnt = std::min(std::max(counts[g], 0), max_det);
        for (int r = 0; r < cnt; ++r) {
            Cand k;
            uint32_t cls;
            if (!yh_fuse_map_row(dets + ((size_t)g * max_det + r) * 6, group_xf + 6 * (size_t)g, W, H, group_weight[g],
                                 skip, k.b, k.s, cls))
                continue;
            k.key = yh_fuse_cand_key(cls, k.s, (uint32_t)(g - lo) * (uint32_t)max_det + (uint32_t)r);
            c.push_back(k);
        }
    }
    std::sort(c.begin(), c.end(), [](const Cand& p, const Cand& q) { return p.key < q.key; });   // keys are unique
    const int n = (int)c.size();
    std::vector<Cluster> cl;            // the clusters of the class being walked
    std::vector<uint64_t> okey;         // output keys of all clusters; the slot indexes `done`
    std::vector<Cluster> done(n);       // slot = segment start + creation index, as on the device
    for (int a = 0; a < n;) {
        const uint32_t cls = yh_fuse_key_class(c[a].key);
        int b = a;
        cl.clear();
        for (; b < n && yh_fuse_key_class(c[b].key) == cls; ++b) {
            const Cand& k = c[b];
            const float ba = yh_fuse_area(k.b);
            float best = -1.0f;                     // every IoU is >= 0 (or NaN, which never wins)
            int at = -1;
            for (int q = 0; q < (int)cl.size(); ++q) {
                const float v = yh_fuse_iou(cl[q].f, cl[q].area, k.b, ba);
                if (v > best) {
                    best = v;
                    at = q;
                }
            }
            if (at >= 0 && (double)best > iou) {
                yh_fuse_add(cl[at].sums, k.s, k.b);
            } else {
                at = (int)cl.size();
                cl.push_back(Cluster{yh_fuse_open(k.s, k.b), {}, 0.0f});
            }
            cl[at].f = yh_fuse_box_of(cl[at].sums);
            cl[at].area = yh_fuse_area(cl[at].f);
        }
        for (int q = 0; q < (int)cl.size(); ++q) {
            done[a + q] = cl[q];
            okey.push_back(yh_fuse_out_key(yh_fuse_score(cl[q].sums, wtot), cls, (uint32_t)(a + q)));
        }
        a = b;
    }
    std::sort(okey.begin(), okey.end());
    const int kept = std::min((int)okey.size(), max_out);
    for (int i = 0; i < kept; ++i) {
        const Cluster& k = done[yh_fuse_key_low(okey[i])];
        float* o = out + 6 * (size_t)i;
        o[0] = k.f.x1; o[1] = k.f.y1; o[2] = k.f.x2; o[3] = k.f.y2;
        o[4] = yh_fuse_score(k.sums, wtot);
        o[5] = (float)yh_fuse_out_key_class(okey[i]);
    }
    *out_count = kept;
}

}  // namespace

const char* yh_fuse_check(const void* dets, const void* counts, int groups, int max_det, const void* group_xf,
                          const void* group_weight, const void* group_offsets, const void* image_wh, int images,
                          int max_groups, int max_out, const void* out, const void* out_counts) {
    if (groups < 0) return "fuse: groups must be >= 0";
    if (max_det < 0) return "fuse: max_det must be >= 0";
    if (images < 0) return "fuse: images must be >= 0";
    if (max_out < 0) return "fuse: max_out must be >= 0";
    if (max_groups < 1) return "fuse: max_groups must be >= 1";
    if ((long long)max_groups * (long long)max_det > (long long)YH_FUSE_MAX_CAND)
        return "fuse: max_groups * max_det exceeds YH_FUSE_MAX_CAND (" YH_STR(YH_FUSE_MAX_CAND) ")";
    if (images > 0 && (!group_offsets || !image_wh || !out_counts)) return "fuse: null group_offsets / image_wh / out_counts";
    if (images > 0 && max_out > 0 && !out) return "fuse: null out";
    if (groups > 0 && (!counts || !group_xf || !group_weight)) return "fuse: null counts / group_xf / group_weight";
    if (groups > 0 && max_det > 0 && !dets) return "fuse: null dets";
    return nullptr;
}

const char* yh_fuse_check_weights(const float* group_weight, const int* group_offsets, int images, int groups,
                                  int max_groups) {
    for (int i = 0; i < images; ++i) {
        const int lo = std::min(std::max(group_offsets[i], 0), groups);
        const int hi = std::min(std::min(std::max(group_offsets[i + 1], lo), groups), lo + max_groups);
        for (int g = lo; g < hi; ++g)
            if (!(group_weight[g] > 0.0f)) return "fuse: every group_weight must be > 0";
    }
    return nullptr;
}

int yh_fuse_host_run(const float* dets, const int* counts, int groups, int max_det, const float* group_xf,
                     const float* group_weight, const int* group_offsets, const float* image_wh, int images,
                     int max_groups, double iou_threshold, float skip_score, int max_out, float* out,
                     int* out_counts, int threads) {
    auto run = [&](int i) {
        // the same clamps as the kernel: the range stays inside the group axis and within max_groups
        const int lo = std::min(std::max(group_offsets[i], 0), groups);
        int hi = std::min(std::max(group_offsets[i + 1], lo), groups);
        if (hi - lo > max_groups) hi = lo + max_groups;
        fuse_image(dets, counts, max_det, group_xf, group_weight, lo, hi, image_wh[2 * (size_t)i],
                   image_wh[2 * (size_t)i + 1], iou_threshold, skip_score, max_out, out + (size_t)i * max_out * 6,
                   out_counts + i);
    };
    yh::parallel_strided(images, threads, run);
    return 0;
}
