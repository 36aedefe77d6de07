// Host (CPU) twin of the cross-tile detection merge (csrc/merge.hip), and the argument check
// both entry points share. HIP-free on purpose: this file compiles alone with any C++17
// compiler (build it with -ffp-contract=off, as the device file is). The arithmetic of a row is
// in csrc/merge_host.h, shared with the kernel.
//
// Semantics, per image i (tiles tile_offsets[i] .. tile_offsets[i + 1], the range clamped to
// [0, tiles] and to max_tiles tiles):
//   1. every row r < counts[t] (clamped to [0, max_det]) of every tile t is a candidate at
//      position (t - first tile) * max_det + r;
//   2. its box is mapped to the source image in fp32, one rounding per step and no FMA:
//      t = x - px; t = t * sx; X = t + ox (y with sy, py, oy), then clipped to [0, W] / [0, H];
//      a row whose clipped box has x2 <= x1 or y2 <= y1 is dropped;
//   3. an image of exactly one tile writes its surviving rows in input order, up to max_out;
//   4. an image of two or more tiles orders its candidates by score descending (ties: the lower
//      position; the order is that of yh_merge_sort_key's 64-bit key) and walks them greedily:
//      a live candidate is kept and kills every later one of equal class (f32 ==) whose
//      inter / (area_i + area_j - inter) in fp32 is, as a double, > iou_threshold
//      (torchvision.ops.nms, as csrc/nms_host.cpp states it, without the class offset); it stops
//      at max_out kept;
//   5. every float of out (images, max_out, 6) and every out_counts[i] is written; rows beyond
//      the count are 0.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_parallel.h"
#include "merge_host.h"

namespace {

struct Cand {
    yh_merge_box b;
    float score, cls, area;
    uint64_t key;
};

void merge_image(const float* dets, const int* counts, int max_det, const float* tile_xf, int lo, int hi, float W,
                 float H, double iou, int max_out, float* out, int* out_count) {
    std::fill(out, out + (size_t)max_out * 6, 0.0f);
    std::vector<Cand> c;
    for (int t = lo; t < hi; ++t) {
        const int cnt = std::min(std::max(counts[t], 0), max_det);
        for (int r = 0; r < cnt; ++r) {
            const float* d = dets + ((size_t)t * max_det + r) * 6;
            yh_merge_box b;
            if (!yh_merge_map_row(d, tile_xf + 6 * (size_t)t, W, H, b)) continue;
            const uint32_t pos = (uint32_t)(t - lo) * (uint32_t)max_det + (uint32_t)r;
            c.push_back({b, d[4], d[5], (b.x2 - b.x1) * (b.y2 - b.y1), yh_merge_sort_key(d[4], pos)});
        }
    }
    const int n = (int)c.size();
    int kept = 0;
    auto emit = [&](const Cand& k) {
        float* o = out + 6 * (size_t)kept++;
        o[0] = k.b.x1; o[1] = k.b.y1; o[2] = k.b.x2; o[3] = k.b.y2; o[4] = k.score; o[5] = k.cls;
    };
    if (hi - lo == 1) {
        for (int i = 0; i < n && kept < max_out; ++i) emit(c[i]);
        *out_count = kept;
        return;
    }
    std::sort(c.begin(), c.end(), [](const Cand& p, const Cand& q) { return p.key < q.key; });   // keys are unique
    std::vector<char> dead(n, 0);
    for (int i = 0; i < n && kept < max_out; ++i) {
        if (dead[i]) continue;
        emit(c[i]);
        const Cand& k = c[i];
        for (int j = i + 1; j < n; ++j) {
            if (dead[j] || !(c[j].cls == k.cls)) continue;
            if (yh_merge_kills(k.b.x1, k.b.y1, k.b.x2, k.b.y2, k.area, c[j].b, c[j].area, iou)) dead[j] = 1;
        }
    }
    *out_count = kept;
}

}  // namespace

const char* yh_merge_check(const void* dets, const void* counts, int tiles, int max_det, const void* tile_xf,
                           const void* tile_offsets, const void* image_wh, int images, int max_tiles, int max_out,
                           const void* out, const void* out_counts) {
    if (tiles < 0) return "tiles must be >= 0";
    if (max_det < 0) return "max_det must be >= 0";
    if (images < 0) return "images must be >= 0";
    if (max_out < 0) return "max_out must be >= 0";
    if (max_tiles < 1) return "max_tiles must be >= 1";
    if ((long long)max_tiles * (long long)max_det > (long long)YH_MERGE_MAX_CAND)
        return "max_tiles * max_det exceeds YH_MERGE_MAX_CAND (" YH_STR(YH_MERGE_MAX_CAND) ")";
    if (images > 0 && (!tile_offsets || !image_wh || !out_counts)) return "null tile_offsets / image_wh / out_counts";
    if (images > 0 && max_out > 0 && !out) return "null out";
    if (tiles > 0 && (!counts || !tile_xf)) return "null counts / tile_xf";
    if (tiles > 0 && max_det > 0 && !dets) return "null dets";
    return nullptr;
}

int yh_merge_host_run(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
                      const int* tile_offsets, const float* image_wh, int images, int max_tiles,
                      double iou_threshold, int max_out, float* out, int* out_counts, int threads) {
    auto run = [&](int i) {
        // the same clamps as the kernel: the range stays inside the tile axis and within max_tiles
        const int lo = std::min(std::max(tile_offsets[i], 0), tiles);
        int hi = std::min(std::max(tile_offsets[i + 1], lo), tiles);
        if (hi - lo > max_tiles) hi = lo + max_tiles;
        merge_image(dets, counts, max_det, tile_xf, lo, hi, image_wh[2 * (size_t)i], image_wh[2 * (size_t)i + 1],
                    iou_threshold, max_out, out + (size_t)i * max_out * 6, out_counts + i);
    };
    yh::parallel_strided(images, threads, run);
    return 0;
}
