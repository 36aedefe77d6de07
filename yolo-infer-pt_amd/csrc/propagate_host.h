// Internal interface of csrc/propagate_host.cpp (HIP-free): the argument check of yh_propagate and
// yh_propagate_remember, the host twin, and - because the kernels (csrc/propagate.hip) and the twin
// must agree bit for bit - the state layout, the geometry of a box and the arithmetic of a result,
// written once for both. The C ABI wrappers live in post_abi.cpp. The semantics are stated at
// yh_propagate in include/yolo_hip.h; tests/_propagate_cases.py restates them in numpy. Luma, the
// candidates' order and the sub-cell refinement are yh_motion's (csrc/motion_host.h).
#ifndef YH_PROPAGATE_HOST_H
#define YH_PROPAGATE_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "motion_host.h"

// State, in bytes (no pointers; host and device use the same bytes): per stream a YH_PROP_HDR byte
// header (word 0: the number of entries n, words 1 .. 3 zero), then max_tracks entries of
// YH_PROP_ENTRY bytes: the 64 bytes of yh_prop_entry, then the template, P * P luma bytes, row major.
// Slots at or beyond n are never read; yh_propagate zeroes the slots its compaction vacates.
enum {
    YH_PROP_P = YH_PROPAGATE_P,
    YH_PROP_CMAX = YH_PROPAGATE_CMAX,
    YH_PROP_HDR = 16,
    YH_PROP_ENTRY_HDR = 64,
    YH_PROP_ENTRY = YH_PROP_ENTRY_HDR + YH_PROP_P * YH_PROP_P,
    YH_PROP_LAUNCH = 32,   // batch rows per launch: their frame descriptors travel as kernel arguments
    YH_PROP_REC = 32       // bytes of a workspace record (yh_prop_rec)
};

struct yh_prop_entry {
    int32_t id;
    float box0[4];         // the remembered box, score and class
    float score, cls;
    int32_t cw, ch;        // the cell size in source pixels
    int32_t ox0, oy0;      // the origin of cell (0, 0) when the box was remembered
    int32_t ox, oy;        // and now
    int32_t zero[3];
};
static_assert(sizeof(yh_prop_entry) == YH_PROP_ENTRY_HDR, "the entry header is 64 bytes");

// what the search leaves per entry for the compaction (the device's workspace, the twin's scratch)
struct yh_prop_rec {
    int32_t ox, oy;        // the origin after the best shift
    int32_t s0;            // the best SAD
    int32_t ok;            // 0: the gate dropped the entry
    float box[4];          // the moved box
};
static_assert(sizeof(yh_prop_rec) == YH_PROP_REC, "a workspace record is 32 bytes");

YH_HD size_t yh_prop_stream_bytes(int max_tracks) { return (size_t)YH_PROP_HDR + (size_t)max_tracks * YH_PROP_ENTRY; }

// rule 2 along one axis: the cell size and the origin of a box side lo .. hi. A coordinate is first
// brought into [-2^20, 2^20] (NaN counts as the lower end), so that the conversions are defined.
YH_HD float yh_prop_coord(float v) { return !(v >= -1048576.0f) ? -1048576.0f : (v > 1048576.0f ? 1048576.0f : v); }
YH_HD void yh_prop_axis(float lo, float hi, int32_t* cell, int32_t* origin) {
    const int b0 = (int)floorf(yh_prop_coord(lo)), b1 = (int)ceilf(yh_prop_coord(hi));
    const int bw = b1 - b0 > 1 ? b1 - b0 : 1;
    int c = (bw + 16) / 32;
    c = c < 1 ? 1 : (c > YH_PROP_CMAX ? YH_PROP_CMAX : c);
    *cell = c;
    *origin = ((b0 + b1) >> 1) - 16 * c;
}
YH_HD int yh_prop_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// An entry as yh_propagate reads it. What yh_propagate_remember and yh_propagate wrote passes
// unchanged: the cells are in [1, CMAX], and the origins stay within 2^20 + 16 * CMAX of 0 by rule 2
// and the centre gate. A state from elsewhere is brought into the same ranges, so that no cell
// indexes past a window and no coordinate sum overflows.
YH_HD int32_t yh_prop_bound(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
YH_HD void yh_prop_sanitize(yh_prop_entry* e) {
    e->cw = yh_prop_bound(e->cw, 1, YH_PROP_CMAX);
    e->ch = yh_prop_bound(e->ch, 1, YH_PROP_CMAX);
    e->ox0 = yh_prop_bound(e->ox0, -(1 << 21), 1 << 21);
    e->oy0 = yh_prop_bound(e->oy0, -(1 << 21), 1 << 21);
    e->ox = yh_prop_bound(e->ox, -(1 << 21), 1 << 21);
    e->oy = yh_prop_bound(e->oy, -(1 << 21), 1 << 21);
}

// the number of rows yh_propagate_remember takes from a batch row
YH_HD int yh_prop_rows(int count, int max_det, int max_tracks) {
    const int m = max_det < max_tracks ? max_det : max_tracks;
    return count < 0 ? 0 : (count > m ? m : count);
}

// rule 4 from the SAD table of an entry ((2 R + 1)^2 values, entry (dy + R) * (2 R + 1) + dx + R) and
// its smallest yh_motion_key: the new origin, the moved box and the gate. fp32, one rounding per
// operation, no FMA.
YH_HD void yh_prop_result(const int32_t* table, int R, uint64_t best, const yh_prop_entry& e, int H, int W, int max_mad,
                          yh_prop_rec* r) {
    const int n = 2 * R + 1, dy = yh_motion_key_dy(best), dx = yh_motion_key_dx(best);
    const int32_t* c = table + (dy + R) * n + (dx + R);
    const int32_t s0 = c[0];
    const float fx = (dx > -R && dx < R) ? yh_motion_refine(s0, c[-1], c[1]) : 0.0f;
    const float fy = (dy > -R && dy < R) ? yh_motion_refine(s0, c[-n], c[n]) : 0.0f;
    r->ox = e.ox + dx * e.cw;
    r->oy = e.oy + dy * e.ch;
    r->s0 = s0;
    const float mx = (float)(r->ox - e.ox0) + fx * (float)e.cw;
    const float my = (float)(r->oy - e.oy0) + fy * (float)e.ch;
    r->box[0] = e.box0[0] + mx;
    r->box[1] = e.box0[1] + my;
    r->box[2] = e.box0[2] + mx;
    r->box[3] = e.box0[3] + my;
    const float cx = 0.5f * (r->box[0] + r->box[2]), cy = 0.5f * (r->box[1] + r->box[3]);
    const bool matched = max_mad < 0 || (long long)s0 <= (long long)max_mad * (YH_PROP_P * YH_PROP_P);
    r->ok = matched && cx >= 0.0f && cx < (float)W && cy >= 0.0f && cy < (float)H ? 1 : 0;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL). On
// success src[k] describes frames[k] (src: batch entries, may be NULL for batch == 0).
const char* yh_propagate_remember_check(const yh_frame* frames, int batch, const float* dets, const int32_t* ids,
                                        const int* counts, int max_det, const void* state, int streams, int max_tracks,
                                        yh_motion_src* src);
const char* yh_propagate_check(const yh_frame* frames, int batch, const void* state, int streams, int max_tracks,
                               int radius, int max_out, const float* dets, const int32_t* ids, const int32_t* sad,
                               const int* counts, yh_motion_src* src);

// The host twins proper; arguments already checked. Batch rows run in parallel over `threads`
// (<= 0: every hardware thread).
int yh_propagate_remember_host_run(const yh_motion_src* src, int batch, const int* stream_ids, const float* dets,
                                   const int32_t* ids, const int* counts, int max_det, void* state, int streams,
                                   int max_tracks, int threads);
int yh_propagate_host_run(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                          int max_tracks, int radius, int max_mad, int max_out, float* dets, int32_t* ids, int32_t* sad,
                          int* counts, int threads);

#endif
