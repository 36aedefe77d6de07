// C ABI of the stages after the forward, none of which needs a handle: yh_nms, yh_match, yh_merge, yh_track, yh_embed_quantize, yh_embed_similarity,
// yh_track_reid, yh_gallery_search, yh_gallery_enrol, yh_assign, yh_track2, yh_track_reid2, yh_motion, yh_track_warp
// and their *_host twins.
#include <algorithm>
#include <vector>

#include "common.h"
#include "assign_host.h"
#include "gallery_host.h"
#include "host_util.h"
#include "match_host.h"
#include "merge_host.h"
#include "motion_host.h"
#include "track_host.h"

using yh::Fail;
using yh::guarded;

namespace {
// the *_check functions return the complaint, or null
void checked(const char* bad) { yh::require(!bad, bad ? bad : ""); }
// what yh_track and yh_track_reid pass on to yh_track2 and yh_track_reid2
const yh_assign_params kGreedy = {YH_ASSIGN_GREEDY, {0, 0, 0}};
}  // namespace

extern "C" {

// the layout is nms.hip's (yh::nms_workspace_bytes / nms_workspace_bind)
size_t yh_nms_workspace_bytes(int batch, int num_classes, int anchors) {
    if (batch <= 0 || num_classes <= 0 || anchors <= 0) return 0;
    return yh::nms_workspace_bytes(batch);
}

#ifdef YH_ABLATION
// Diagnostic builds only (make EXTRA=-DYH_ABLATION; not in the ABI header):
// yh_debug_nms_trace(buf) makes later yh_nms calls record per-image phase timestamps
// into the device buffer buf ([batch][16] u64, the slots of nms.hip's TraceSlot).
static unsigned long long* nms_trace = nullptr;
int yh_debug_nms_trace(void* device_buf) {
    nms_trace = (unsigned long long*)device_buf;
    return 0;
}
#endif

int yh_nms(int dtype, const void* y, int batch, int num_classes, int anchors, float conf_threshold,
           double iou_threshold, int max_det, int max_nms, float max_wh, void* workspace, size_t workspace_bytes,
           float* dets, int* counts, void* stream) {
    return guarded([&] {
        yh::require(y && dets && counts && workspace, "null argument");
        yh::require(dtype == YH_F32 || dtype == YH_F16 || dtype == YH_BF16, "bad dtype");
        yh::require(batch > 0 && anchors > 0 && num_classes > 0, "bad shape");
        static_assert(yh::NMS_MAX_DET == 1024 && yh::NMS_PAIR_BITS == 26, "the two messages below name these limits");
        yh::require(max_det > 0 && max_det <= yh::NMS_MAX_DET, "max_det must be in [1, 1024]");
        yh::require(max_nms > 0, "max_nms must be positive");
        yh::require(conf_threshold >= 0.0f, "conf_threshold must be >= 0");
        yh::require((long long)anchors * num_classes < (1ll << yh::NMS_PAIR_BITS), "anchors * classes exceeds 2^26");
        yh::require(workspace_bytes >= yh_nms_workspace_bytes(batch, num_classes, anchors), "NMS workspace too small");
        yh::NmsArgs a{};
        a.y = y; a.B = batch; a.A = anchors; a.nc = num_classes;
        // compare in the input dtype: torch rounds the Python-float threshold to
        // the tensor dtype before comparing (util.py:130,147)
        a.conf = yh::round_to_dtype(dtype, conf_threshold);
        // largest float <= iou_threshold: for any float ovr, ovr > thr (double) <=> ovr > a.iou
        float t = (float)iou_threshold;
        if ((double)t > iou_threshold) t = std::nextafter(t, -INFINITY);
        a.iou = t;
        a.max_wh = max_wh;
        a.max_det = max_det;
        a.max_nms = max_nms;
#ifdef YH_ABLATION
        a.trace = nms_trace;
#endif
        yh::nms_workspace_bind(a, workspace);
        {   // lowest bin at the threshold (or 2047 bins below 1.0 for tiny thresholds)
            uint32_t cb;
            std::memcpy(&cb, &a.conf, 4);
            const int one = 0x3F80;
            a.bin_base = std::max((int)(cb >> 16), one - 2047);
        }
        a.dets = dets;
        a.ndet = counts;
        const int rc = yh::launch_nms(dtype, a, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("NMS launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_match(const float* dets, const int* counts, int batch, int max_det, const float* labels,
             const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
             int* counts_out, void* stream) {
    return guarded([&] {
        static_assert(YH_MATCH_MAX_DET >= 1024, "the ABI promises at least 1024");
        checked(yh_match_check(dets, counts, batch, max_det, labels, label_offsets, iou_v, num_iou, tp));
        const int rc = yh::launch_match(dets, counts, batch, max_det, labels, label_offsets, iou_v, num_iou, tp,
                                        score_cls, counts_out, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("match launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_match_host(const float* dets, const int* counts, int batch, int max_det, const float* labels,
                  const int* label_offsets, const float* iou_v, int num_iou, uint8_t* tp, float* score_cls,
                  int* counts_out, int threads) {
    return guarded([&] {
        checked(yh_match_check(dets, counts, batch, max_det, labels, label_offsets, iou_v, num_iou, tp));
        yh_match_host_run(dets, counts, batch, max_det, labels, label_offsets, iou_v, num_iou, tp, score_cls,
                          counts_out, threads);
    });
}

int yh_merge(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
             const int* tile_offsets, const float* image_wh, int images, int max_tiles, double iou_threshold,
             int max_out, float* out, int* out_counts, void* stream) {
    return guarded([&] {
        checked(yh_merge_check(dets, counts, tiles, max_det, tile_xf, tile_offsets, image_wh, images,
                               max_tiles, max_out, out, out_counts));
        const int rc = yh::launch_merge(dets, counts, tiles, max_det, tile_xf, tile_offsets, image_wh, images,
                                        max_tiles, iou_threshold, max_out, out, out_counts, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("merge launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_merge_host(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
                  const int* tile_offsets, const float* image_wh, int images, int max_tiles, double iou_threshold,
                  int max_out, float* out, int* out_counts, int threads) {
    return guarded([&] {
        checked(yh_merge_check(dets, counts, tiles, max_det, tile_xf, tile_offsets, image_wh, images,
                               max_tiles, max_out, out, out_counts));
        yh_merge_host_run(dets, counts, tiles, max_det, tile_xf, tile_offsets, image_wh, images, max_tiles,
                          iou_threshold, max_out, out, out_counts, threads);
    });
}

size_t yh_track_state_bytes(int streams, int max_tracks) {
    if (streams < 0 || max_tracks < 1) return 0;
    return (size_t)streams * yh_track_stream_words(max_tracks) * 4;
}

int yh_track2(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
              int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids, int* det_index,
              int* out_counts, const yh_assign_params* ap, void* stream) {
    return guarded([&] {
        checked(yh_track_check(dets, counts, batch, max_det, state, streams, max_tracks, p, max_out, out, ids,
                               det_index, out_counts));
        checked(yh_assign_params_check(ap));
        const int rc = yh::launch_track(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, *p, max_out,
                                        out, ids, det_index, out_counts, ap->mode == YH_ASSIGN_OPTIMAL,
                                        (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("track launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_track2_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                   int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids,
                   int* det_index, int* out_counts, const yh_assign_params* ap, int threads) {
    return guarded([&] {
        checked(yh_track_check(dets, counts, batch, max_det, state, streams, max_tracks, p, max_out, out, ids,
                               det_index, out_counts));
        checked(yh_assign_params_check(ap));
        yh_track_host_run(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out, ids,
                          det_index, out_counts, threads, nullptr, ap->mode);
    });
}

int yh_track(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
             int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids, int* det_index,
             int* out_counts, void* stream) {
    return yh_track2(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out, ids,
                     det_index, out_counts, &kGreedy, stream);
}

int yh_track_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                  int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids,
                  int* det_index, int* out_counts, int threads) {
    return yh_track2_host(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out, ids,
                          det_index, out_counts, &kGreedy, threads);
}

int yh_track_warp(void* state, int streams, int max_tracks, int reid_dim, const float* motion, const int* stream_ids,
                  int batch, void* stream) {
    return guarded([&] {
        checked(yh_track_warp_check(state, streams, max_tracks, reid_dim, motion, batch));
        yh::require((uintptr_t)state % 4 == 0, "state must be 4-byte aligned");
        const int rc = yh::launch_track_warp(state, streams, max_tracks, reid_dim, motion, stream_ids, batch,
                                             (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("track_warp launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_track_warp_host(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                       const int* stream_ids, int batch, int threads) {
    return guarded([&] {
        checked(yh_track_warp_check(state, streams, max_tracks, reid_dim, motion, batch));
        yh_track_warp_host_run(state, streams, max_tracks, reid_dim, motion, stream_ids, batch, threads);
    });
}

size_t yh_motion_state_bytes(int streams, int thumb_h, int thumb_w) {
    if (streams < 0 || thumb_h < 1 || thumb_w < 1 || (long long)thumb_h * thumb_w > YH_MOTION_MAX_THUMB) return 0;
    return yh_motion_staging_offset(streams, thumb_h, thumb_w) + (size_t)YH_MOTION_LAUNCH * thumb_h * thumb_w;
}

int yh_motion(const yh_frame* frames, int batch, const int* stream_ids, void* state, int streams, int thumb_h,
              int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, void* stream) {
    return guarded([&] {
        std::vector<yh_motion_src> src((size_t)std::max(batch, 0));
        checked(yh_motion_check(frames, batch, state, streams, thumb_h, thumb_w, radius, motion, sad, src.data()));
        yh::require((uintptr_t)state % 4 == 0, "motion: state must be 4-byte aligned on the device");
        const int rc = yh::launch_motion(src.data(), batch, stream_ids, state, streams, thumb_h, thumb_w, radius, max_mad,
                                         motion, sad, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("motion launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_motion_host(const yh_frame* frames, int batch, const int* stream_ids, void* state, int streams, int thumb_h,
                   int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, int threads) {
    return guarded([&] {
        std::vector<yh_motion_src> src((size_t)std::max(batch, 0));
        checked(yh_motion_check(frames, batch, state, streams, thumb_h, thumb_w, radius, motion, sad, src.data()));
        yh_motion_host_run(src.data(), batch, stream_ids, state, streams, thumb_h, thumb_w, radius, max_mad, motion, sad,
                           threads);
    });
}

int yh_assign(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts, const int32_t* d_counts,
              int32_t* row_of_slot, int32_t* slot_of_row, void* stream) {
    return guarded([&] {
        checked(yh_assign_check(weights, problems, T, D, row_of_slot, slot_of_row));
        const int rc = yh::launch_assign(weights, problems, T, D, t_counts, d_counts, row_of_slot, slot_of_row,
                                         (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("assign launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_assign_host(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts,
                   const int32_t* d_counts, int32_t* row_of_slot, int32_t* slot_of_row, int threads) {
    return guarded([&] {
        checked(yh_assign_check(weights, problems, T, D, row_of_slot, slot_of_row));
        yh_assign_host_run(weights, problems, T, D, t_counts, d_counts, row_of_slot, slot_of_row, threads);
    });
}

int yh_embed_quantize(const float* e, int rows, int dim, const int* count, int8_t* q, void* stream) {
    return guarded([&] {
        checked(yh_embed_quantize_check(e, rows, dim, q));
        const int rc = yh::launch_embed_quantize(e, rows, dim, count, q, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("embed_quantize launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_embed_quantize_host(const float* e, int rows, int dim, const int* count, int8_t* q, int threads) {
    return guarded([&] {
        checked(yh_embed_quantize_check(e, rows, dim, q));
        yh_embed_quantize_host_run(e, rows, dim, count, q, threads);
    });
}

int yh_embed_similarity(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                        int batch, int ra, int rb, int dim, int32_t* out, void* stream) {
    return guarded([&] {
        checked(yh_embed_similarity_check(a, a_block_stride, nblocks, b, batch, ra, rb, dim, out));
        yh::require(((uintptr_t)a | (uintptr_t)b | a_block_stride) % 16 == 0,
                    "a, b and a_block_stride must be multiples of 16 bytes on the device");
        const int rc = yh::launch_embed_similarity(a, a_block_stride, nblocks, a_index, b, batch, ra, rb, dim, out,
                                                   nullptr, nullptr, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("embed_similarity launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_embed_similarity_host(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                             int batch, int ra, int rb, int dim, int32_t* out, int threads) {
    return guarded([&] {
        checked(yh_embed_similarity_check(a, a_block_stride, nblocks, b, batch, ra, rb, dim, out));
        yh_embed_similarity_host_run(a, a_block_stride, nblocks, a_index, b, batch, ra, rb, dim, out, threads);
    });
}

size_t yh_track_reid_state_bytes(int streams, int max_tracks, int dim) {
    if (streams < 0 || max_tracks < 1 || yh_reid_dim_check(dim)) return 0;
    return (size_t)streams * yh_track_reid_stream_bytes(max_tracks, dim);
}

size_t yh_track_reid_workspace_bytes(int batch, int max_det, int max_tracks, int dim) {
    if (batch < 0 || max_det < 0 || max_tracks < 1 || yh_reid_dim_check(dim)) return 0;
    return yh_reid_ws_bytes(batch, max_det, max_tracks, dim);
}

int yh_track_reid2(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                   int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids,
                   int* det_index, int* out_counts, const float* embed, int capacity, int dim, const int* feat_counts,
                   const int* embed_total, const yh_reid_params* rp, void* workspace, size_t workspace_bytes,
                   const yh_assign_params* ap, void* stream) {
    return guarded([&] {
        checked(yh_assign_params_check(ap));
        checked(yh_track_check(dets, counts, batch, max_det, state, streams, max_tracks, p, max_out, out, ids,
                               det_index, out_counts));
        checked(yh_track_reid_check(batch, max_det, max_tracks, capacity, dim, rp, workspace, workspace_bytes));
        yh::require(((uintptr_t)workspace | (uintptr_t)state) % 16 == 0,
                    "state and workspace must be 16-byte aligned on the device");
        if (batch == 0) return;
        char* ws = static_cast<char*>(workspace);
        yh::TrackReid rd{};
        rd.q = reinterpret_cast<const int8_t*>(ws);
        rd.flags = reinterpret_cast<const int*>(ws + yh_reid_ws_flags(batch, max_det, dim));
        rd.sim = reinterpret_cast<const int*>(ws + yh_reid_ws_sim(batch, max_det, dim));
        rd.sim_t = reinterpret_cast<const int*>(ws + yh_reid_ws_sim_t(batch, max_det, max_tracks, dim));
        int* gnz = reinterpret_cast<int*>(ws + yh_reid_ws_gnz(batch, max_det, max_tracks, dim));
        const bool features = embed && streams > 0 && max_det > 0;
        rd.gnz = features ? gnz : nullptr;
        rd.code = reinterpret_cast<int*>(ws + yh_reid_ws_code(batch, max_det, max_tracks, dim));
        rd.dim = dim;
        rd.cos_min = rp->cos_min;
        rd.iou_min = rp->iou_min;
        hipStream_t s = (hipStream_t)stream;
        int rc = yh::launch_embed_scatter(embed, capacity, dim, counts, feat_counts, embed_total, batch, max_det,
                                          const_cast<int8_t*>(rd.q), const_cast<int*>(rd.flags), s);
        // the galleries are read where they lie: block stream_ids[b] of `streams`, behind the words
        // of yh_track's state. Without features no pair reads a similarity.
        const size_t gallery_offset = yh_track_stream_words(max_tracks) * 4;
        const size_t stream_bytes = yh_track_reid_stream_bytes(max_tracks, dim);
        if (rc == 0 && features)
            rc = yh::launch_embed_similarity(static_cast<const int8_t*>(state) + gallery_offset, stream_bytes, streams,
                                             stream_ids, rd.q, batch, max_tracks, max_det, dim,
                                             const_cast<int*>(rd.sim), gnz, const_cast<int*>(rd.sim_t), s);
        if (rc == 0)
            rc = yh::launch_track_reid(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, *p, max_out,
                                       out, ids, det_index, out_counts, rd, ap->mode == YH_ASSIGN_OPTIMAL, s);
        if (rc == 0)
            rc = yh::launch_gallery_update(state, stream_bytes, gallery_offset, stream_ids, batch, max_tracks, max_det,
                                           dim, rd.q, rd.flags, rd.code, s);
        if (rc != 0) throw Fail(YH_EHIP, std::string("track_reid launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_track_reid2_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                        void* state, int streams, int max_tracks, const yh_track_params* p, int max_out, float* out,
                        int* ids, int* det_index, int* out_counts, const float* embed, int capacity, int dim,
                        const int* feat_counts, const int* embed_total, const yh_reid_params* rp, void* workspace,
                        size_t workspace_bytes, const yh_assign_params* ap, int threads) {
    return guarded([&] {
        checked(yh_assign_params_check(ap));
        checked(yh_track_check(dets, counts, batch, max_det, state, streams, max_tracks, p, max_out, out, ids,
                               det_index, out_counts));
        checked(yh_track_reid_check(batch, max_det, max_tracks, capacity, dim, rp, workspace, workspace_bytes));
        const yh_track_reid_args ra{embed, capacity, dim, feat_counts, embed_total, *rp, workspace};
        yh_track_host_run(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out, ids,
                          det_index, out_counts, threads, &ra, ap->mode);
    });
}

int yh_track_reid(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                  int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids,
                  int* det_index, int* out_counts, const float* embed, int capacity, int dim, const int* feat_counts,
                  const int* embed_total, const yh_reid_params* rp, void* workspace, size_t workspace_bytes,
                  void* stream) {
    return yh_track_reid2(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out, ids,
                          det_index, out_counts, embed, capacity, dim, feat_counts, embed_total, rp, workspace,
                          workspace_bytes, &kGreedy, stream);
}

int yh_track_reid_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids, void* state,
                       int streams, int max_tracks, const yh_track_params* p, int max_out, float* out, int* ids,
                       int* det_index, int* out_counts, const float* embed, int capacity, int dim,
                       const int* feat_counts, const int* embed_total, const yh_reid_params* rp, void* workspace,
                       size_t workspace_bytes, int threads) {
    return yh_track_reid2_host(dets, counts, batch, max_det, stream_ids, state, streams, max_tracks, p, max_out, out,
                               ids, det_index, out_counts, embed, capacity, dim, feat_counts, embed_total, rp, workspace,
                               workspace_bytes, &kGreedy, threads);
}

size_t yh_gallery_workspace_bytes(int capacity, int nq, int k, int chunk_rows) {
    if (capacity < 0 || capacity > YH_GALLERY_MAX_CAPACITY || nq < 0 || k < 1 || k > YH_GALLERY_MAX_K ||
        chunk_rows < 0 || chunk_rows % 64)
        return 0;
    return yh_gal_ws_bytes(capacity, nq, k, chunk_rows);
}

int yh_gallery_search(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                      const int8_t* q, int nq, const int32_t* nq_count, int k, int chunk_rows, int32_t* scores,
                      int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded([&] {
        checked(yh_gallery_search_check(gallery, capacity, dim, q, nq, k, chunk_rows, scores, index, workspace,
                                        workspace_bytes));
        yh::require(((uintptr_t)gallery | (uintptr_t)q | (uintptr_t)workspace) % 16 == 0,
                    "gallery, q and workspace must be 16-byte aligned on the device");
        const int rc = yh::launch_gallery_search(gallery, labels, size, capacity, dim, q, nq, nq_count, k, chunk_rows,
                                                 scores, index, workspace, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("gallery_search launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_gallery_search_host(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                           const int8_t* q, int nq, const int32_t* nq_count, int k, int chunk_rows, int32_t* scores,
                           int32_t* index, void* workspace, size_t workspace_bytes, int threads) {
    return guarded([&] {
        checked(yh_gallery_search_check(gallery, capacity, dim, q, nq, k, chunk_rows, scores, index, workspace,
                                        workspace_bytes));
        yh_gallery_search_host_run(gallery, labels, size, capacity, dim, q, nq, nq_count, k, scores, index, threads);
    });
}

int yh_gallery_enrol(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q, int nq,
                     const int32_t* nq_count, const int32_t* take, const int32_t* labels_in, int32_t* next_label,
                     int32_t* rows_out, void* stream) {
    return guarded([&] {
        checked(yh_gallery_enrol_check(gallery, labels, size, capacity, dim, q, nq, labels_in, next_label, rows_out));
        yh::require(((uintptr_t)gallery | (uintptr_t)q) % 16 == 0, "gallery and q must be 16-byte aligned on the device");
        const int rc = yh::launch_gallery_enrol(gallery, labels, size, capacity, dim, q, nq, nq_count, take, labels_in,
                                                next_label, rows_out, (hipStream_t)stream);
        if (rc != 0) throw Fail(YH_EHIP, std::string("gallery_enrol launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int yh_gallery_enrol_host(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q,
                          int nq, const int32_t* nq_count, const int32_t* take, const int32_t* labels_in,
                          int32_t* next_label, int32_t* rows_out, int threads) {
    (void)threads;   // one walk: a row's place depends on every row before it
    return guarded([&] {
        checked(yh_gallery_enrol_check(gallery, labels, size, capacity, dim, q, nq, labels_in, next_label, rows_out));
        yh_gallery_enrol_host_run(gallery, labels, size, capacity, dim, q, nq, nq_count, take, labels_in, next_label,
                                  rows_out);
    });
}

}  // extern "C"
