// Internal interface of csrc/track_host.cpp (HIP-free): the argument check shared by the device
// and the host entry point of the tracker, the host tracking loop, and - because the kernel
// (csrc/track.hip) and the host twin must agree bit for bit - the state layout and the
// arithmetic of one track, written once for both. The C ABI wrappers live in post_abi.cpp; host_util.h
// holds yh_last_error()'s message. The semantics are stated in csrc/track_host.cpp.
#ifndef YH_TRACK_HOST_H
#define YH_TRACK_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "box_math.h"
#include "yolo_hip.h"

// State of one stream, in 32-bit words (no pointers; host and device use the same bytes):
//   [0] frame counter f   [1] ids handed out so far (next_id - 1)   [2] [3] zero
//   then YH_TRACK_FIELDS arrays of max_tracks words, field major: word (field, slot) lies at
//   YH_TRACK_HDR + field * max_tracks + slot.
// All-zero bytes are the empty state. A slot that becomes free keeps its other fields (both
// sides write the same values there), only its status is cleared.
enum {
    YH_TRACK_HDR = 4,
    YH_TRK_STATUS = 0,   // int: 0 free, 1 tentative, 2 tracked, 3 lost
    YH_TRK_ID = 1,       // int, >= 1
    YH_TRK_LAST = 2,     // int: frame of the last match (or of the birth)
    YH_TRK_CLS = 3,      // f32
    YH_TRK_X = 4,        // f32 x 4 each: cx, cy, w, h
    YH_TRK_V = 8,
    YH_TRK_A = 12,       // Pxx
    YH_TRK_B = 16,       // Pxv
    YH_TRK_C = 20,       // Pvv
    YH_TRACK_FIELDS = 24
};

YH_HD size_t yh_track_stream_words(int max_tracks) {
    return (size_t)YH_TRACK_HDR + (size_t)YH_TRACK_FIELDS * (size_t)max_tracks;
}

// The Kalman state of one slot: four independent (position, velocity) pairs.
struct yh_track_kal {
    float x[4], v[4], a[4], b[4], c[4];
};

struct yh_track_box {
    float x1, y1, x2, y2;
};

YH_HD float yh_trk_sq(float c, float u) {
    const float s = c * u;
    return s * s;
}

// step 1 of one non-free slot (status: as stored, before this frame)
YH_HD void yh_trk_predict(yh_track_kal& k, int status) {
    if (status != 2) k.v[3] = 0.0f;
    const float w = k.x[2], h = k.x[3];
    for (int i = 0; i < 4; ++i) {
        const float u = (i & 1) ? h : w;
        const float qp = yh_trk_sq(0.05f, u);
        const float qv = yh_trk_sq(0.00625f, u);
        k.x[i] = k.x[i] + k.v[i];
        k.a[i] = ((k.a[i] + 2.0f * k.b[i]) + k.c[i]) + qp;
        k.b[i] = k.b[i] + k.c[i];
        k.c[i] = k.c[i] + qv;
    }
}

// the box of a state (steps 1 and 6)
YH_HD yh_track_box yh_trk_box(const yh_track_kal& k) {
    const float hw = k.x[2] * 0.5f, hh = k.x[3] * 0.5f;
    yh_track_box b;
    b.x1 = k.x[0] - hw;
    b.x2 = k.x[0] + hw;
    b.y1 = k.x[1] - hh;
    b.y2 = k.x[1] + hh;
    return b;
}

// the measurement of a detection row
YH_HD void yh_trk_measure(const yh_track_box& d, float z[4]) {
    z[0] = (d.x1 + d.x2) * 0.5f;
    z[1] = (d.y1 + d.y2) * 0.5f;
    z[2] = d.x2 - d.x1;
    z[3] = d.y2 - d.y1;
}

// step 4 of a matched slot
YH_HD void yh_trk_update(yh_track_kal& k, const yh_track_box& d) {
    float z[4];
    yh_trk_measure(d, z);
    const float w = k.x[2], h = k.x[3];
    for (int i = 0; i < 4; ++i) {
        const float u = (i & 1) ? h : w;
        const float r = yh_trk_sq(0.05f, u);
        const float a = k.a[i], b = k.b[i], c = k.c[i];
        const float S = a + r;
        const float kx = a / S;
        const float kv = b / S;
        const float y = z[i] - k.x[i];
        k.x[i] = k.x[i] + kx * y;
        k.v[i] = k.v[i] + kv * y;
        k.a[i] = a - kx * a;
        k.b[i] = b - kx * b;
        k.c[i] = c - kv * b;
    }
}

// step 5 of a new slot
YH_HD void yh_trk_birth(yh_track_kal& k, const yh_track_box& d) {
    float z[4];
    yh_trk_measure(d, z);
    for (int i = 0; i < 4; ++i) {
        const float u = (i & 1) ? z[3] : z[2];
        k.x[i] = z[i];
        k.v[i] = 0.0f;
        k.a[i] = yh_trk_sq(0.1f, u);
        k.b[i] = 0.0f;
        k.c[i] = yh_trk_sq(0.0625f, u);
    }
}

// yh_track_warp: is (s, tx, ty) a motion to apply? Finite (the exponent is not all ones: a bit
// test, which no floating-point assumption can fold away) and s > 0.
YH_HD bool yh_trk_warp_valid(const float* m) {
    for (int i = 0; i < 3; ++i) {
        uint32_t u;
#ifdef __HIP_DEVICE_COMPILE__
        u = __float_as_uint(m[i]);
#else
        __builtin_memcpy(&u, m + i, 4);
#endif
        if ((u & 0x7f800000u) == 0x7f800000u) return false;
    }
    return m[0] > 0.0f;
}

// yh_track_warp of one non-free slot: x -> s x + t for the centre, s x for the size, s v, s^2 P
YH_HD void yh_trk_warp(yh_track_kal& k, float s, float tx, float ty) {
    const float s2 = s * s;
    k.x[0] = s * k.x[0] + tx;
    k.x[1] = s * k.x[1] + ty;
    k.x[2] = s * k.x[2];
    k.x[3] = s * k.x[3];
    for (int i = 0; i < 4; ++i) {
        k.v[i] = s * k.v[i];
        k.a[i] = s2 * k.a[i];
        k.b[i] = s2 * k.b[i];
        k.c[i] = s2 * k.c[i];
    }
}

// step 3: is (slot box t, row box d) a candidate pair at threshold thr, and with which IoU?
// (the class test is the caller's) The pair order is yh::float_order(iou) descending, then the
// slot, then the row.
YH_HD bool yh_trk_pair(const yh_track_box& t, const yh_track_box& d, float thr, float& iou) {
    const float inter = yh::intersection(t.x1, t.y1, t.x2, t.y2, d.x1, d.y1, d.x2, d.y2);
    if (inter == 0.0f) return false;
    const float at = (t.x2 - t.x1) * (t.y2 - t.y1);
    const float ad = (d.x2 - d.x1) * (d.y2 - d.y1);
    iou = inter / ((at + ad) - inter);
    return iou >= thr;
}

// The appearance term of yh_track_reid's first association, in place of yh_trk_pair: is the pair
// a candidate, and with which sort value? feat: the slot's gallery row and the row's quantised
// feature are both non-zero; dot: their int32 product (read only when feat).
YH_HD bool yh_trk_pair_reid(const yh_track_box& t, const yh_track_box& d, float thr, bool feat, int dot,
                            float cos_min, float iou_min, float& val) {
    const float inter = yh::intersection(t.x1, t.y1, t.x2, t.y2, d.x1, d.y1, d.x2, d.y2);
    float iou = 0.0f;
    if (inter != 0.0f) {
        const float at = (t.x2 - t.x1) * (t.y2 - t.y1);
        const float ad = (d.x2 - d.x1) * (d.y2 - d.y1);
        iou = inter / ((at + ad) - inter);
    }
    val = iou;
    bool eligible = false;
    if (feat) {
        const float cosv = (float)dot / 16129.0f;
        const float app = 0.5f + 0.5f * cosv;
        eligible = cosv >= cos_min && iou >= iou_min;
        if (eligible && app > iou) val = app;
    }
    return (inter != 0.0f && iou >= thr) || eligible;
}

// An integer vector of squared length S scaled to length 127: the factor, and an element
// (yh_embed_quantize's step 4 and the gallery update). fp64, one rounding per operation.
YH_HD double yh_reid_scale(int64_t S) { return 127.0 / sqrt((double)S); }
YH_HD int yh_reid_round(int v, double scale) { return (int)rint((double)v * scale); }

// yh_track_reid's state: per stream yh_track's words, then the gallery (max_tracks, dim) int8
YH_HD size_t yh_track_reid_stream_bytes(int max_tracks, int dim) {
    return yh_track_stream_words(max_tracks) * 4 + (size_t)max_tracks * (size_t)dim;
}

// yh_track_reid's workspace: q (batch, max_det, dim) int8, flags (batch, max_det) int32 (bit 0:
// the row has a feature, bit 1: its q is non-zero), and for the device only sim (batch, max_tracks,
// max_det) int32 and its transpose sim_t, gnz (batch, max_tracks) int32 (the slot's gallery row is non-zero) and code
// (batch, max_tracks) int32 (the gallery update's work); sections 256-byte aligned
YH_HD size_t yh_reid_al(size_t v) { return (v + 255) & ~(size_t)255; }
YH_HD size_t yh_reid_ws_flags(int batch, int max_det, int dim) { return yh_reid_al((size_t)batch * max_det * dim); }
YH_HD size_t yh_reid_ws_sim(int batch, int max_det, int dim) {
    return yh_reid_al(yh_reid_ws_flags(batch, max_det, dim) + (size_t)batch * max_det * 4);
}
YH_HD size_t yh_reid_ws_sim_t(int batch, int max_det, int max_tracks, int dim) {
    return yh_reid_al(yh_reid_ws_sim(batch, max_det, dim) + (size_t)batch * max_tracks * max_det * 4);
}
YH_HD size_t yh_reid_ws_gnz(int batch, int max_det, int max_tracks, int dim) {
    return yh_reid_al(yh_reid_ws_sim_t(batch, max_det, max_tracks, dim) + (size_t)batch * max_tracks * max_det * 4);
}
YH_HD size_t yh_reid_ws_code(int batch, int max_det, int max_tracks, int dim) {
    return yh_reid_al(yh_reid_ws_gnz(batch, max_det, max_tracks, dim) + (size_t)batch * max_tracks * 4);
}
YH_HD size_t yh_reid_ws_bytes(int batch, int max_det, int max_tracks, int dim) {
    return yh_reid_al(yh_reid_ws_code(batch, max_det, max_tracks, dim) + (size_t)batch * max_tracks * 4);
}

// The appearance arguments of yh_track_reid as the host loop takes them (NULL: plain yh_track)
struct yh_track_reid_args {
    const float* embed;
    int capacity, dim;
    const int* feat_counts;
    const int* embed_total;
    yh_reid_params rp;
    void* workspace;
};

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_reid_dim_check(int dim);
const char* yh_track_reid_check(int batch, int max_det, int max_tracks, int capacity, int dim, const yh_reid_params* rp,
                                const void* workspace, size_t workspace_bytes);
const char* yh_embed_quantize_check(const void* e, int rows, int dim, const void* q);
const char* yh_embed_similarity_check(const void* a, size_t a_block_stride, int nblocks, const void* b, int batch,
                                      int ra, int rb, int dim, const void* out);
const char* yh_track_check(const void* dets, const void* counts, int batch, int max_det, const void* state,
                           int streams, int max_tracks, const yh_track_params* p, int max_out, const void* out,
                           const void* ids, const void* det_index, const void* out_counts);

// The host twin proper; arguments already checked. Batch rows (streams) run in parallel over
// `threads` (<= 0: every hardware thread). assign_mode: YH_ASSIGN_GREEDY or YH_ASSIGN_OPTIMAL.
int yh_track_host_run(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                      void* state, int streams, int max_tracks, const yh_track_params* p, int max_out, float* out,
                      int* ids, int* det_index, int* out_counts, int threads,
                      const yh_track_reid_args* reid = nullptr, int assign_mode = YH_ASSIGN_GREEDY);

// yh_track_warp: the argument check of both entry points, the bytes of one stream's block
// (reid_dim 0: yh_track's state, else yh_track_reid's), and the host twin (arguments already checked).
const char* yh_track_warp_check(const void* state, int streams, int max_tracks, int reid_dim, const void* motion,
                                int batch);
YH_HD size_t yh_track_warp_stride(int max_tracks, int reid_dim) {
    return reid_dim ? yh_track_reid_stream_bytes(max_tracks, reid_dim) : yh_track_stream_words(max_tracks) * 4;
}
int yh_track_warp_host_run(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                           const int* stream_ids, int batch, int threads);

// The host twins of yh_embed_quantize / yh_embed_similarity; arguments already checked.
void yh_embed_quantize_row(const float* e, int dim, int8_t* q);   // one row; e NULL: zeros
int yh_embed_quantize_host_run(const float* e, int rows, int dim, const int* count, int8_t* q, int threads);
int yh_embed_similarity_host_run(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index,
                                 const int8_t* b, int batch, int ra, int rb, int dim, int32_t* out, int threads);

#endif
