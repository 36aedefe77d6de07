// Host (CPU) twin of the track propagation (csrc/propagate.hip), and the argument checks both entry
// points share. HIP-free on purpose: this file compiles with any C++17 compiler beside
// motion_host.cpp (build both with -ffp-contract=off, as the device file is). The state layout, the
// geometry and the result arithmetic are in csrc/propagate_host.h, shared with the kernels.
//
// Semantics: the rules stated at yh_propagate in include/yolo_hip.h. Where the kernels spread the
// source bytes and the candidates over lanes and waves, this file does what the text says: a box
// sum per cell, a SAD per candidate, the smallest key, an ordered compaction. Every sum is an
// integer sum, so the orders need not agree.
#include "propagate_host.h"

#include <cstring>
#include <vector>

#include "host_parallel.h"

namespace {

unsigned luma(const yh_motion_src& f, int y, int x) {
    const unsigned char* row = f.p0 + (size_t)y * f.stride0;
    if (f.format == YH_PIX_NV12) return row[x];
    const unsigned char* p = row + (size_t)x * 3;
    return yh_motion_luma(p[0], p[1], p[2]);
}

// rule 2: cell (i, j) relative to the origin (oy, ox), pixel coordinates clamped into the frame
unsigned char cell(const yh_motion_src& f, int oy, int ox, int ch, int cw, int i, int j) {
    unsigned sum = 0;
    for (int t = 0; t < ch; ++t) {
        const int y = yh_prop_clamp(oy + i * ch + t, f.h);
        for (int u = 0; u < cw; ++u) sum += luma(f, y, yh_prop_clamp(ox + j * cw + u, f.w));
    }
    return (unsigned char)yh_motion_mean(sum, (unsigned)(cw * ch));
}

const char* common_check(const yh_frame* frames, int batch, const void* state, int streams, int max_tracks,
                         yh_motion_src* src) {
    if (batch < 0) return "propagate: batch must be >= 0";
    if (streams < 0) return "propagate: streams must be >= 0";
    if (max_tracks < 1 || max_tracks > YH_PROPAGATE_MAX_TRACKS)
        return "propagate: max_tracks must be in [1, " YH_STR(YH_PROPAGATE_MAX_TRACKS) "]";
    if (batch > 0 && (!frames || !state)) return "propagate: null frames / state";
    for (int k = 0; k < batch; ++k) {
        yh_motion_src s{};
        if (const char* bad = yh_motion_describe(frames[k], s)) return bad;
        if (s.h > (1 << 20) || s.w > (1 << 20)) return "propagate: a frame side exceeds 2^20";
        if (src) src[k] = s;
    }
    return nullptr;
}

}  // namespace

const char* yh_propagate_remember_check(const yh_frame* frames, int batch, const float* dets, const int32_t* ids,
                                        const int* counts, int max_det, const void* state, int streams, int max_tracks,
                                        yh_motion_src* src) {
    if (max_det < 0) return "propagate: max_det must be >= 0";
    if (batch > 0 && (!counts || (max_det > 0 && (!dets || !ids)))) return "propagate: null dets / ids / counts";
    return common_check(frames, batch, state, streams, max_tracks, src);
}

const char* yh_propagate_check(const yh_frame* frames, int batch, const void* state, int streams, int max_tracks,
                               int radius, int max_out, const float* dets, const int32_t* ids, const int32_t* sad,
                               const int* counts, yh_motion_src* src) {
    if (radius < 1 || radius > YH_PROPAGATE_MAX_RADIUS)
        return "propagate: radius must be in [1, " YH_STR(YH_PROPAGATE_MAX_RADIUS) "]";
    if (max_out < 0) return "propagate: max_out must be >= 0";
    if (batch > 0 && (!counts || (max_out > 0 && (!dets || !ids || !sad)))) return "propagate: null dets / ids / sad / counts";
    return common_check(frames, batch, state, streams, max_tracks, src);
}

int yh_propagate_remember_host_run(const yh_motion_src* src, int batch, const int* stream_ids, const float* dets,
                                   const int32_t* ids, const int* counts, int max_det, void* state, int streams,
                                   int max_tracks, int threads) {
    unsigned char* base = static_cast<unsigned char*>(state);
    yh::parallel_strided(batch, threads, [&](int b) {
        const int s = stream_ids ? stream_ids[b] : b;
        if (s < 0 || s >= streams) return;
        unsigned char* blk = base + (size_t)s * yh_prop_stream_bytes(max_tracks);
        const int n = yh_prop_rows(counts[b], max_det, max_tracks);
        const uint32_t hdr[4] = {(uint32_t)n, 0u, 0u, 0u};
        std::memcpy(blk, hdr, YH_PROP_HDR);
        for (int r = 0; r < n; ++r) {
            const float* d = dets + ((size_t)b * max_det + r) * 6;
            yh_prop_entry e{};
            e.id = ids[(size_t)b * max_det + r];
            for (int q = 0; q < 4; ++q) e.box0[q] = d[q];
            e.score = d[4];
            e.cls = d[5];
            yh_prop_axis(d[0], d[2], &e.cw, &e.ox0);
            yh_prop_axis(d[1], d[3], &e.ch, &e.oy0);
            e.ox = e.ox0;
            e.oy = e.oy0;
            unsigned char* slot = blk + YH_PROP_HDR + (size_t)r * YH_PROP_ENTRY;
            std::memcpy(slot, &e, sizeof e);
            unsigned char* T = slot + YH_PROP_ENTRY_HDR;
            for (int i = 0; i < YH_PROP_P; ++i)
                for (int j = 0; j < YH_PROP_P; ++j) T[i * YH_PROP_P + j] = cell(src[b], e.oy, e.ox, e.ch, e.cw, i, j);
        }
    });
    return 0;
}

int yh_propagate_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                          int max_tracks, int radius, int max_mad, int max_out, float* dets, int32_t* ids, int32_t* sad,
                          int* counts, int threads) {
    constexpr int P = YH_PROP_P;
    const int R = radius, n1 = 2 * R + 1, S = P + 2 * R;
    unsigned char* base = static_cast<unsigned char*>(state);
    yh::parallel_strided(batch, threads, [&](int b) {
        if (max_out > 0) {
            std::memset(dets + (size_t)b * max_out * 6, 0, (size_t)max_out * 24);
            std::memset(ids + (size_t)b * max_out, 0, (size_t)max_out * 4);
            std::memset(sad + (size_t)b * max_out, 0, (size_t)max_out * 4);
        }
        counts[b] = 0;
        const int s = stream_ids ? stream_ids[b] : b;
        if (s < 0 || s >= streams) return;
        unsigned char* blk = base + (size_t)s * yh_prop_stream_bytes(max_tracks);
        uint32_t stored;
        std::memcpy(&stored, blk, 4);
        const int n = stored > (uint32_t)max_tracks ? max_tracks : (int)stored;
        std::vector<unsigned char> win((size_t)S * S);
        std::vector<int32_t> table((size_t)n1 * n1);
        int kept = 0;
        for (int k = 0; k < n; ++k) {
            unsigned char* slot = blk + YH_PROP_HDR + (size_t)k * YH_PROP_ENTRY;
            yh_prop_entry e;
            std::memcpy(&e, slot, sizeof e);
            yh_prop_sanitize(&e);
            const unsigned char* T = slot + YH_PROP_ENTRY_HDR;
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < S; ++j) win[(size_t)i * S + j] = cell(src[b], e.oy, e.ox, e.ch, e.cw, i - R, j - R);
            uint64_t best = ~(uint64_t)0;
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    uint32_t acc = 0;
                    for (int i = 0; i < P; ++i) {
                        const unsigned char* w = win.data() + (size_t)(i + dy + R) * S + (dx + R);
                        for (int j = 0; j < P; ++j) {
                            const int a = w[j], q = T[i * P + j];
                            acc += (uint32_t)(a > q ? a - q : q - a);
                        }
                    }
                    table[(size_t)(dy + R) * n1 + (dx + R)] = (int32_t)acc;
                    const uint64_t key = yh_motion_key(acc, dy, dx);
                    if (key < best) best = key;
                }
            yh_prop_rec r;
            yh_prop_result(table.data(), R, best, e, src[b].h, src[b].w, max_mad, &r);
            if (!r.ok) continue;
            if (kept < max_out) {
                float* d = dets + ((size_t)b * max_out + kept) * 6;
                for (int q = 0; q < 4; ++q) d[q] = r.box[q];
                d[4] = e.score;
                d[5] = e.cls;
                ids[(size_t)b * max_out + kept] = e.id;
                sad[(size_t)b * max_out + kept] = r.s0;
            }
            unsigned char* dst = blk + YH_PROP_HDR + (size_t)kept * YH_PROP_ENTRY;
            if (dst != slot) std::memmove(dst, slot, YH_PROP_ENTRY);
            std::memcpy(dst + offsetof(yh_prop_entry, ox), &r.ox, 4);
            std::memcpy(dst + offsetof(yh_prop_entry, oy), &r.oy, 4);
            ++kept;
        }
        if (kept < n) std::memset(blk + YH_PROP_HDR + (size_t)kept * YH_PROP_ENTRY, 0, (size_t)(n - kept) * YH_PROP_ENTRY);
        const uint32_t hdr[4] = {(uint32_t)kept, 0u, 0u, 0u};
        std::memcpy(blk, hdr, YH_PROP_HDR);
        counts[b] = kept < max_out ? kept : max_out;
    });
    return 0;
}
