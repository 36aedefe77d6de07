/*
 * yolo_hip.h — C ABI of the MI355X (gfx950) YOLOv11 inference path.
 *
 * This is the drop-in boundary between the Python mirror of the reference's
 * module API (yolo-infer-pt_amd/nets/nn.py, yolo-infer-pt_amd/utils/util.py)
 * and the hand-written HIP kernels in yolo-infer-pt_amd/csrc/.  Signatures use
 * plain pointers and sizes only; no torch types cross this line.
 *
 * Reference interfaces replaced (file:line into t0saki/YOLO-Infer-pt):
 *   yh_create           nets/nn.py:308-347  yolo_v11_{n,t,s,m,l,x}() -> YOLO(width, depth, csp, nc)
 *                       nets/nn.py:282-292  YOLO.__init__ (DarkNet + DarkFPN + Head graph)
 *   yh_conv_count,
 *   yh_conv_info        the reference's state_dict naming (nets/nn.py module tree), one entry per conv
 *   yh_load_conv        nets/nn.py:8-25     fuse_conv (BN folded into conv in fp32), nets/nn.py:299-305 YOLO.fuse
 *   yh_forward          nets/nn.py:294-297  YOLO.forward in eval mode, incl. Head.forward decode
 *                       (nets/nn.py:255-270), DFL (nets/nn.py:222-225) and make_anchors (utils/util.py:85-96)
 *   yh_forward_u8       main.py:265-267     uint8 -> dtype, / 255 preprocessing fused into yh_forward's stem
 *   yh_nms              utils/util.py:123-169 non_max_suppression (+ torchvision.ops.nms, util.py:162)
 *   yh_nms_host         the same for head outputs on the CPU device (main.py:20 device fallback)
 *   yh_match            utils/util.py:99-120 compute_metric for a whole batch (main.py:275-294 loop)
 *   yh_match_host       the same in host memory
 *   yh_merge            no reference counterpart (the reference never leaves the network canvas and
 *                       has no tiled inference): the inverse of the letterbox of utils/dataset.py:95-103,
 *                       292-313 per tile, plus a cross-tile greedy NMS under the torchvision.ops.nms contract
 *   yh_merge_host       the same in host memory
 *   yh_letterbox        utils/dataset.py:95-103, 292-313, 86-88: eval-mode load_image resize
 *                       (cv2 INTER_LINEAR) + zero border + HWC->CHW, BGR->RGB, on the device
 *   yh_letterbox_host   the same on the host (Dataset.__getitem__ in the loader workers)
 *   yh_letterbox_frames no reference counterpart: the same letterbox for video - BGR or NV12 frames
 *                       onto a square or rectangular canvas (yh_letterbox is this for BGR, square)
 *   yh_letterbox_frames_host, yh_nv12_to_bgr_host   the same, and the conversion alone, on the host
 *   yh_crop_rois        no reference counterpart (the reference has no second stage): one fixed-size
 *                       RGB crop per detection, cut from the BGR or NV12 source frame with the
 *                       letterbox's resize, for a batch in one launch
 *   yh_crop_rois_host   the same in host memory
 *   yh_create_cls       no reference counterpart (the reference has no classifier): the graph of
 *                       nets/nn.py YOLOCls - Ultralytics' YOLO11-cls: DarkNet without the SPPF, C2PSA,
 *                       then Classify (1x1 conv to 1280 + BN + SiLU, global average pool, linear, softmax)
 *   yh_classify         YOLOCls.forward / YOLOCls.features in eval mode on a batch of crops
 *   yh_embed_quantize,
 *   yh_embed_similarity no reference counterpart: unit int8 features and their exact int32 cosine
 *                       matrix on the int8 MFMA, for gallery search and for the tracker
 *   yh_track_reid       no reference counterpart: yh_track with an appearance term in the first
 *                       association and a per-slot int8 feature gallery in the state
 *   yh_embed_quantize_host, yh_embed_similarity_host, yh_track_reid_host   the same in host memory
 *   yh_gallery_search,
 *   yh_gallery_enrol    no reference counterpart: the k best rows of a large int8 gallery per query
 *                       on the int8 MFMA (identities across streams and time), and appending to it
 *   yh_gallery_search_host, yh_gallery_enrol_host   the same in host memory
 *   yh_assign           no reference counterpart: batched maximum-weight assignment by shortest
 *                       augmenting paths, one workgroup per problem
 *   yh_track2,
 *   yh_track_reid2      yh_track / yh_track_reid with that assignment in place of the greedy walk
 *                       of the associations, on request (ByteTrack's lapjv step)
 *   yh_assign_host, yh_track2_host, yh_track_reid2_host   the same in host memory
 *   yh_motion           no reference counterpart: the camera's translation between consecutive frames
 *                       of a stream, by block matching on luma thumbnails (BoT-SORT's global-motion step)
 *   yh_track_warp       no reference counterpart: that motion applied to a stream's tracks before the
 *                       frame's yh_track* call
 *   yh_motion_host, yh_track_warp_host   the same in host memory
 *
 * Conventions
 *   - Every function returns 0 on success and a negative YH_E* code on failure;
 *     yh_last_error() returns a thread-local message describing the last failure.
 *   - Device pointers are HIP device memory owned by the caller (PyTorch tensors).
 *     The library owns its packed weights and its activation workspace.
 *   - `stream` is a hipStream_t passed as void* (0 = legacy default stream).
 *     yh_forward and yh_nms are asynchronous on that stream: they never
 *     synchronise the host and allocate nothing once the workspace for a
 *     given (batch, height, width) exists.
 *   - One handle is bound to one device and one compute dtype.  Calls on one
 *     handle must be serialised by the caller; distinct handles are independent
 *     (data-parallel serving = one handle per GPU).
 */
#ifndef YOLO_HIP_H
#define YOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YH_ABI_VERSION 7

/* status codes */
#define YH_OK 0
#define YH_EINVAL -1     /* bad argument / shape */
#define YH_ESTATE -2     /* call out of order (e.g. forward before all weights loaded) */
#define YH_EHIP -3       /* HIP runtime error */
#define YH_ENOMEM -4     /* device allocation failed */

/* compute / storage dtypes of a handle (activations and outputs) */
#define YH_F32 0
#define YH_F16 1
#define YH_BF16 2

typedef struct yh_handle yh_handle;

/* Network description: the (width, depth, csp) triple of nets/nn.py:308-347 plus
 * the class count (Head nc, nets/nn.py:232-238). */
typedef struct {
    int width[6];     /* e.g. {3,16,32,64,128,256} for v11_n */
    int depth[6];     /* repeat counts; only depth[0..5] as used by DarkNet/DarkFPN */
    int csp[2];       /* 0/1: C3k nesting for shallow / deep C3k2 blocks */
    int num_classes;  /* nc */
} yh_variant;

/* ABI version of the loaded library (YH_ABI_VERSION). */
int yh_abi_version(void);

/* Thread-local message of the last failing call ("" if none). */
const char* yh_last_error(void);

/* Build the layer graph of a variant for `device` in `dtype` (YH_F32/F16/BF16). */
int yh_create(const yh_variant* variant, int device, int dtype, yh_handle** out);

/* Release all device memory owned by the handle. NULL is accepted. */
void yh_destroy(yh_handle* h);

/* Number of convolutions whose weights the handle expects. */
int yh_conv_count(const yh_handle* h);

/* Describe conv `index`: `name` = state_dict prefix of the owning module
 * (e.g. "net.p2.1.res_m.0.conv1" for a Conv block, "head.box.0.2" for a plain
 * nn.Conv2d); shape of the expected fp32 weight (cout, cin_per_group, k, k);
 * `has_bias` = 1 if the reference module carries a conv bias (head output
 * convs). The pointer in *name stays valid for the handle's lifetime. */
int yh_conv_info(const yh_handle* h, int index, const char** name, int* cout,
                 int* cin_per_group, int* ksize, int* groups, int* has_bias);

/* Load one conv from host fp32 arrays. `weight` is (cout, cin/groups, k, k)
 * contiguous. `bias` may be NULL (treated as zeros). If `bn_gamma` is non-NULL
 * the BatchNorm (gamma, beta, running mean, running var, eps) is folded in
 * exactly as fuse_conv (nets/nn.py:8-25) does it, in fp32. Packed, dtype-cast
 * copies are uploaded to the handle's device; host arrays may be freed after. */
int yh_load_conv(yh_handle* h, int index, const float* weight, const float* bias,
                 const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                 const float* bn_var, double bn_eps);

/* Anchors produced for an input of height x width (sum over strides 8/16/32). */
int yh_num_anchors(const yh_handle* h, int height, int width, int* anchors);

/* Bytes of device workspace the handle holds for (batch, height, width)
 * after yh_reserve (activations, excluding weights). */
int yh_workspace_bytes(const yh_handle* h, int batch, int height, int width, size_t* bytes);

/* Optional: allocate the workspace for (batch, height, width) up front. */
int yh_reserve(yh_handle* h, int batch, int height, int width);

/* Eval-mode forward.
 *   x: device (batch, 3, height, width) NCHW contiguous, handle dtype
 *   y: device (batch, 4 + nc, anchors) contiguous, handle dtype:
 *      rows 0..3 = (cx, cy, w, h) in pixels, rows 4.. = sigmoid class scores
 * height, width: multiples of 32. */
int yh_forward(yh_handle* h, const void* x, int batch, int height, int width,
               void* y, void* stream);

/* yh_forward on the data loader's image tensor: x is device (batch, 3, height,
 * width) NCHW uint8 (RGB, utils/dataset.py:86-88 layout), and the reference's
 * preprocessing `samples.half() / 255.` (main.py:265-267; to the handle dtype)
 * is fused into the stem's input load - no converted copy of x is made.
 * Bit-identical to yh_forward on x.to(dtype) / 255. computed by torch on the
 * device (u * fp32(1/255), rounded to the dtype). */
int yh_forward_u8(yh_handle* h, const void* x, int batch, int height, int width,
                  void* y, void* stream);

/* Second stage: a classifier over fixed-size crops (yh_crop_rois's output layout).
 *
 * yh_create_cls builds the graph of nets/nn.py YOLOCls for a variant: the detector's backbone up
 * to net.p5.1, C2PSA as net.p5.2, then the head. Its convs are named as in the module's
 * state_dict; the last two are "head.conv" (1x1, BatchNorm, SiLU, YH_CLS_EMBED couts) and
 * "head.linear" (the Linear layer described as a 1x1 conv with bias: weight (nc, 1280, 1, 1)).
 * Everything that takes a handle works on both kinds, except: yh_classify on a detection handle,
 * and yh_forward / yh_forward_u8 / yh_num_anchors on a classifier handle, return YH_ESTATE with
 * a message and launch nothing. On a classifier handle yh_debug_run_ops' y is the (batch, nc)
 * fp32 probs (no logits / embed copies, no count), and per-image fp32 vectors appear among the
 * operands of yh_debug_op_desc as 1 x 1 maps with "f32": 1 (roles "e": the embedding, "z": the
 * logits, "a": the head conv's output), which yh_debug_operand copies as fp32.
 *
 * yh_classify: x as for yh_forward (x_u8 = 0: handle dtype) or yh_forward_u8 (x_u8 = 1: uint8 RGB,
 * / 255 fused into the stem); height and width multiples of 32 (a shape some kernel of the graph
 * has no plan for is refused with YH_EINVAL before anything is launched).
 *   probs  (batch, nc) f32, required; logits (batch, nc) f32 and embed (batch, YH_CLS_EMBED) f32
 *   may be NULL. count: device int32* or NULL.
 * Asynchronous on `stream`; allocates nothing once the workspace of the shape exists; replays one
 * captured single-chain graph per (batch, height, width, input kind) - the outputs and count are
 * reached through an indirection, so any pointers serve.
 *
 * Classifier arithmetic (every dtype; f = the last feature map, HW its pixels per image):
 *  1. a = head.conv(f), bit for bit the per-layer dense 1x1 conv's output: conv_mx's single
 *     reduction order on 16-bit handles, folded BN, bias and SiLU in fp32, one rounding to the
 *     handle dtype. On the fp32 handle the K sum is exact (fp64 accumulation) and this layer's bias
 *     and SiLU are evaluated in fp64 too, so a is the fp64 conv rounded once to fp32.
 *  2. e[b, c] = s * (float)(1.0 / HW) where s is one fp32 chain from zero over image b's pixels
 *     in ascending row-major order: s = (..((a[b,0,c] + a[b,1,c]) + a[b,2,c]) ..) + a[b,HW-1,c].
 *     The fused head (16-bit handles, YH_CLSHEAD=1 at yh_create_cls; the default is conv + pool,
 *     which measured faster) runs the same chain in its epilogue, so both paths give the same e
 *     bit for bit. The order does
 *     not depend on the batch size, on the image's place in the batch or on the conv plan.
 *  3. z = W e + b with W in the handle dtype (fp32 on the fp32 handle), e and the accumulation in
 *     fp32 (per class: 64 partial fmaf chains over interleaved 8-channel chunks, added in a fixed
 *     butterfly, the bias last); probs = exp(z - max z) / sum exp(z - max z) in fp32. Each output
 *     element is written exactly once.
 *  4. n = clamp(*count, 0, batch) (batch when count is NULL). Rows at or beyond n are all-zero in
 *     probs, logits and embed. The forward still runs on every row: the shape stays fixed, nothing
 *     synchronises and the graph replays. This is how yh_crop_rois' `total` is consumed without a
 *     read-back. */
#define YH_CLS_EMBED 1280
int yh_create_cls(const yh_variant* variant, int device, int dtype, yh_handle** out);
int yh_classify(yh_handle* h, const void* x, int x_u8, int batch, int height, int width,
                const int* count, float* probs, float* logits, float* embed, void* stream);

/* Bytes of device workspace yh_nms needs for a (batch, 4 + num_classes, anchors) input. */
size_t yh_nms_workspace_bytes(int batch, int num_classes, int anchors);

/* Batched NMS over a head output y (batch, 4 + num_classes, anchors) of dtype
 * YH_F32/F16/BF16, on the current HIP device. Stateless: the caller supplies the
 * workspace (yh_nms_workspace_bytes). Semantics of non_max_suppression
 * (utils/util.py:123-169): candidate (anchor, class) pairs with score >
 * conf_threshold (threshold rounded to the input dtype, as torch compares),
 * sorted by score descending (ties: lower anchor*nc + class first), truncated to
 * max_nms, class-offset boxes (class * max_wh), greedy IoU > iou_threshold
 * suppression (torchvision.ops.nms contract), at most max_det kept per image.
 *   dets:   device float (batch, max_det, 6) = x1, y1, x2, y2, score, class
 *   counts: device int32 (batch) kept detections per image
 * Box geometry is evaluated in fp32 for every dtype; class scores must lie in
 * [0, 2) (sigmoid outputs). Asynchronous on `stream`. */
int yh_nms(int dtype, const void* y, int batch, int num_classes, int anchors,
           float conf_threshold, double iou_threshold, int max_det, int max_nms,
           float max_wh, void* workspace, size_t workspace_bytes,
           float* dets, int* counts, void* stream);

/* The same NMS on the host CPU for a head output in HOST memory (the reference's
 * CPU device path, main.py:20): identical candidate / order / suppression rules,
 * torchvision's CPU loop in float32. dets (batch, max_det, 6) and counts (batch)
 * are host arrays; `threads` <= 0 uses every hardware thread (images in parallel).
 * Synchronous. */
int yh_nms_host(int dtype, const void* y, int batch, int num_classes, int anchors,
                float conf_threshold, double iou_threshold, int max_det, int max_nms,
                float max_wh, float* dets, int* counts, int threads);

/* Largest max_det yh_match / yh_match_host accept: the kernel keeps 12 bytes of LDS per
 * detection slot plus a 6 KiB label chunk (54 KiB at the cap). */
#define YH_MATCH_MAX_DET 4096

/* Match a whole batch's detections to its labels (compute_metric, utils/util.py:99-120, for
 * every image and every IoU threshold) in one launch, straight from yh_nms's output.
 *   dets (batch, max_det, 6), counts (batch): as yh_nms writes them. counts is clamped to
 *       [0, max_det]; rows at or beyond counts[b] may be uninitialised and are never read.
 *   labels (N, 5) f32 [cls, x1, y1, x2, y2] in pixels, grouped by image; label_offsets
 *       (batch + 1) int32 ascending: image b owns rows offsets[b] .. offsets[b + 1]. The caller
 *       guarantees 0 <= offsets <= N; any number of labels per image.
 *   iou_v (num_iou) f32 thresholds, 1 <= num_iou <= 32.
 *   tp (batch, max_det, num_iou) uint8 0/1: every byte is written, rows beyond counts[b] are 0.
 *   score_cls (batch, max_det, 2) f32, optional (NULL): columns 4, 5 of the valid rows, 0 beyond.
 *   counts_out (batch) int32, optional (NULL): the clamped counts.
 * Per image: best[d] = the label of equal class (f32 ==) with the highest IoU, the lower label
 * index on ties, biou[d] that IoU; tp[d, t] = 1 iff d has a best label, biou[d] >= iou_v[t] and
 * no e < d has best[e] == best[d] and biou[e] >= iou_v[t]. The IoU is fp32, bit-identical to
 * yolo_hip.metrics._iou: inter = max(0, iw) * max(0, ih), inter / (((areaA + areaB) - inter) + 1e-7f).
 * Box coordinates must be finite (device and host agree on any input; torch's min / max
 * propagate NaN, these do not).
 * yh_match: device pointers, asynchronous on `stream`, allocates nothing, never synchronises.
 * yh_match_host: the same for host pointers, images in parallel over `threads` (<= 0: all
 * hardware threads), synchronous.
 * YH_EINVAL (message in yh_last_error()): num_iou outside [1, 32], a negative size, max_det
 * above YH_MATCH_MAX_DET, a NULL required pointer. */
int yh_match(const float* dets, const int* counts, int batch, int max_det,
             const float* labels, const int* label_offsets,
             const float* iou_v, int num_iou,
             uint8_t* tp, float* score_cls, int* counts_out, void* stream);
int yh_match_host(const float* dets, const int* counts, int batch, int max_det,
                  const float* labels, const int* label_offsets,
                  const float* iou_v, int num_iou,
                  uint8_t* tp, float* score_cls, int* counts_out, int threads);

/* Largest max_tiles * max_det yh_merge / yh_merge_host accept: the candidates of one image. The
 * kernel keeps an 8-byte sort key per candidate in LDS (64 KiB, requested with
 * hipFuncAttributeMaxDynamicSharedMemorySize) and the candidates themselves in registers, 8 per
 * thread of a 1024-thread workgroup. */
#define YH_MERGE_MAX_CAND 8192

/* Map the NMS output of a batch of tiles back to the source images and merge the tiles of each
 * image, in one launch.
 *   dets (tiles, max_det, 6), counts (tiles): as yh_nms writes them for the tile batch. counts is
 *       clamped to [0, max_det]; rows at or beyond counts[t] may be uninitialised and are never read.
 *   tile_xf (tiles, 6) f32: sx, sy, px, py, ox, oy of each tile (below).
 *   tile_offsets (images + 1) int32 ascending: image i owns tiles tile_offsets[i] .. tile_offsets[i + 1].
 *       The tile axis may hold more tiles than the offsets reference (padding of a last partial
 *       batch): they are never visited. Each range is clamped to [0, tiles] and to max_tiles tiles.
 *   image_wh (images, 2) f32: W, H of the source image.
 *   max_tiles: the caller's bound on tiles per image; max_tiles * max_det <= YH_MERGE_MAX_CAND.
 *   out (images, max_out, 6) f32 = x1, y1, x2, y2, score, class in source pixels; out_counts (images)
 *       int32. Every byte of both is written; rows beyond an image's count are 0; an image with no
 *       tiles has count 0.
 * Per image, identical on device and host bit for bit:
 *   1. every valid row of every tile of the image is a candidate; its position is (tile, row) in
 *      input order;
 *   2. the box is mapped in fp32, one rounding per operation, no FMA: t = x - px; t = t * sx;
 *      X = t + ox (y with sy, py, oy), then clipped to [0, W] / [0, H]. A row whose clipped box has
 *      x2 <= x1 or y2 <= y1 is dropped;
 *   3. an image of exactly one tile writes its surviving rows in input order, up to max_out: the
 *      plain inverse letterbox, no suppression;
 *   4. an image of two or more tiles runs a greedy NMS under the torchvision.ops.nms contract
 *      (yh_nms_host): candidates by score descending, ties to the lower position; a live candidate
 *      is kept and kills every later candidate of equal class (f32 ==) whose
 *      inter / (area_i + area_j - inter), in fp32 on the mapped boxes, is as a double >
 *      iou_threshold; at most max_out are kept. Classes are compared, not offset by max_wh: source
 *      coordinates of several thousand pixels would lose bits to the offset.
 * Boxes and scores must be finite. Duplicates are merged by IoU only: there is no
 * intersection-over-smaller rule and no dropping of boxes that touch an interior tile edge.
 * yh_merge: device pointers, one workgroup per image, asynchronous on `stream`, allocates nothing,
 * never synchronises. yh_merge_host: the same for host pointers, images in parallel over `threads`
 * (<= 0: all hardware threads), synchronous.
 * YH_EINVAL (message in yh_last_error()): a negative size, max_tiles < 1, max_tiles * max_det above
 * YH_MERGE_MAX_CAND, a NULL required pointer. */
int yh_merge(const float* dets, const int* counts, int tiles, int max_det,
             const float* tile_xf, const int* tile_offsets, const float* image_wh,
             int images, int max_tiles, double iou_threshold, int max_out,
             float* out, int* out_counts, void* stream);
int yh_merge_host(const float* dets, const int* counts, int tiles, int max_det,
                  const float* tile_xf, const int* tile_offsets, const float* image_wh,
                  int images, int max_tiles, double iou_threshold, int max_out,
                  float* out, int* out_counts, int threads);

/* Multi-object tracking over video streams, one launch per frame for all streams of a batch
 * (no reference counterpart: the rules below are the specification; tests/_track_cases.py
 * restates them in numpy). Row b of the NMS output dets (batch, max_det, 6) / counts (batch) is
 * the next frame of stream stream_ids[b] (NULL: of stream b); the entries of stream_ids must be
 * distinct, and a row whose id is outside [0, streams) writes count 0 and zero rows and touches
 * no state. Frames of one stream must arrive in order.
 *
 * `state` is opaque: yh_track_state_bytes(streams, max_tracks) bytes, all-zero = no tracks, frame
 * 0. It holds no pointers and has the same layout on host and device, so it can be copied
 * between them (and saved) in the middle of a sequence. A stream owns max_tracks slots; a slot
 * has a status (0 free, 1 tentative, 2 tracked, 3 lost), an id >= 1, the frame of its last
 * match, a class and the state of ultralytics' KalmanFilterXYWH, stored as four independent
 * (position x, velocity v, covariance a = Pxx, b = Pxv, c = Pvv) filters over cx, cy, w, h (its
 * F, H, Q, R and initial P never couple the components).
 *
 * Per stream and call, in fp32 with one rounding per operation and no FMA; wh4 = (w, h, w, h),
 * sq(c, u) = (c * u) * (c * u):
 *   1. predict: f += 1; every slot that is not free: v[h] = 0 unless its status is 2; with wh4 of
 *      the current x: x += v; a = ((a + 2 b) + c) + sq(0.05, wh4); b += c; c += sq(0.00625, wh4).
 *      Its box is cx -+ w * 0.5, cy -+ h * 0.5.
 *   2. rows 0 .. min(max(counts, 0), max_det) are read, the others never: "high" rows have
 *      score >= track_high, "low" rows track_low <= score < track_high.
 *   3. assoc(slots, rows, thr): the candidate pairs have equal class (f32 ==; not tested when
 *      class_aware is 0), an intersection != 0 and iou = inter / ((area_t + area_d) - inter)
 *      >= thr; they are walked by iou descending, then slot, then row ascending, and a pair is
 *      taken when both sides are unmatched (greedy; yh_track2 can solve the assignment instead, as
 *      ByteTrack's lapjv does). Three calls:
 *      (status 2 or 3, high, iou_first); (status 2 still unmatched, low, iou_second);
 *      (status 1, high still unmatched, iou_tentative).
 *   4. a matched slot is updated with z = (centre, size) of its row: r = sq(0.05, wh4 of the
 *      predicted x); S = a + r; kx = a / S; kv = b / S; y = z - x; x += kx y; v += kv y;
 *      (a, b, c) = (a - kx a, b - kx b, c - kv b); its status becomes 2, its last frame f, its
 *      class the row's. An unmatched status-2 slot becomes 3, an unmatched status-1 slot free;
 *      then a status-3 slot with f - last frame > max_age becomes free.
 *   5. births: the unmatched high rows with score >= track_new take, in row order, the free
 *      slots in slot order (rows left over are dropped): x = z, v = 0, a = sq(0.1, wh4 of z),
 *      b = 0, c = sq(0.0625, wh4 of z), the next id; status 2 in frame 1, else 1.
 *   6. output: every slot of status 2 matched or born in this frame, ordered by its row, at most
 *      max_out: out (batch, max_out, 6) = the box of the updated x, the row's score and class;
 *      ids (batch, max_out) the track id; det_index (batch, max_out) the row; out_counts (batch).
 *      Every byte of the four is written, rows beyond the count are 0.
 * Inputs must be finite.
 * yh_track: device pointers, one workgroup per batch row, asynchronous on `stream`, allocates
 * nothing, never synchronises. yh_track_host: the same bytes for host pointers, rows in parallel
 * over `threads` (<= 0: all hardware threads), synchronous.
 * YH_EINVAL (message in yh_last_error()): max_tracks above YH_TRACK_MAX_TRACKS or max_det above
 * YH_TRACK_MAX_DET, a negative size, max_tracks < 1, a NULL required pointer, track_low >
 * track_high, max_age < 0. */
#define YH_TRACK_MAX_TRACKS 1024
#define YH_TRACK_MAX_DET 1024
typedef struct {
    float track_high, track_low, track_new, iou_first, iou_second, iou_tentative;
    int max_age, class_aware;
} yh_track_params;
size_t yh_track_state_bytes(int streams, int max_tracks);
int yh_track(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
             void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
             float* out, int* ids, int* det_index, int* out_counts, void* stream);
int yh_track_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                  void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                  float* out, int* ids, int* det_index, int* out_counts, int threads);

/* Appearance features for re-identification (no reference counterpart: the rules below are the
 * specification; tests/_reid_cases.py restates them in numpy). A feature is any (rows, dim) f32
 * embedding - yh_classify's, or a trained re-ID head's; dim % 64 == 0 and 64 <= dim <=
 * YH_REID_MAX_DIM. Every sum below is an integer sum, so no order needs fixing and the device
 * and the host compute the same bytes.
 *
 * yh_embed_quantize: e (rows, dim) f32 -> q (rows, dim) int8, the unit vector of each row scaled
 * to length 127. Per row, in fp64 with one rounding per operation and no FMA:
 *   1. m = max |e_i|. If m == 0 or any element is not finite, q = 0 ("no feature").
 *   2. p_i = (int)rint((double)e_i * (16384.0 / (double)m)).
 *   3. S = sum p_i^2 (int64).
 *   4. q_i = (int)rint((double)p_i * (127.0 / sqrt((double)S))).
 * count: NULL, or (1) int32 (device memory for yh_embed_quantize): rows at or beyond
 * min(max(*count, 0), rows) are written as zero and their e is never read. Every byte of q is
 * written.
 *
 * yh_embed_similarity: out[b] = A[b] . B[b]^T in exact int32, for a batch.
 *   a:       int8 blocks of (ra, dim), row-major, block k at a + k * a_block_stride bytes, nblocks
 *            of them
 *   a_index: NULL, or (batch) int32: batch row b reads block a_index[b] (NULL: block b). An index
 *            outside [0, nblocks) gives a zero block and touches nothing else (stream_ids' rule)
 *   b:       (batch, rb, dim) int8
 *   out:     (batch, ra, rb) int32; every element is written
 * Any int8 value is legal, -128 included. The device kernel is the gfx950 int8 MFMA
 * (v_mfma_i32_32x32x32_i8); it loads 16 bytes at a time, so on the device a, b and
 * a_block_stride must be multiples of 16 bytes.
 *
 * Both are asynchronous on `stream`, allocate nothing and never synchronise; the *_host twins
 * split the rows over `threads` (<= 0: every hardware thread) and are synchronous.
 * YH_EINVAL (message in yh_last_error()), nothing launched: a bad dim, a negative size, a NULL
 * required pointer (none is required when there is nothing to write), a_block_stride smaller
 * than ra * dim, a misaligned device operand. */
#define YH_REID_MAX_DIM 2048
int yh_embed_quantize(const float* e, int rows, int dim, const int* count, int8_t* q, void* stream);
int yh_embed_quantize_host(const float* e, int rows, int dim, const int* count, int8_t* q, int threads);
int yh_embed_similarity(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                        int batch, int ra, int rb, int dim, int32_t* out, void* stream);
int yh_embed_similarity_host(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index, const int8_t* b,
                             int batch, int ra, int rb, int dim, int32_t* out, int threads);

/* yh_track with an appearance term in its first association (no reference counterpart; BoT-SORT's
 * and DeepSORT's idea under this tracker's greedy walk). Arguments, rules, outputs and errors are
 * yh_track's, plus:
 *
 *   embed:        (capacity, dim) f32 features, or NULL (no row has a feature)
 *   feat_counts:  (batch) int32 or NULL (NULL: the clamped counts)
 *   embed_total:  (1) int32 or NULL; ignored when embed is NULL
 *   rp:           cos_min, iou_min (BoT-SORT: 0.5 / 0.5; iou_min = 0 re-identifies anywhere in
 *                 the frame)
 *   workspace:    caller-owned, yh_track_reid_workspace_bytes(batch, max_det, max_tracks, dim)
 *                 bytes, 16-byte aligned on the device; its contents mean nothing between calls
 *
 * Features of rows. With c_b = min(max(counts[b], 0), max_det), row r of batch row b has a feature
 * iff r < n_b = min(max(feat_counts[b], 0), c_b), and its slot s = n_0 + ... + n_(b-1) + r is
 * below capacity and, when embed_total is given, below *embed_total. This is yh_crop_rois'
 * compaction: crops cut with counts = feat_counts, yh_classify's embedding of them and the crops'
 * total plug in as they lie. (The sum runs over all batch rows, whatever their stream_ids.) The
 * row's quantised feature q is yh_embed_quantize's of embed[s]; every other row has q = 0.
 *
 * State: yh_track_reid_state_bytes(streams, max_tracks, dim) bytes; per stream the words of
 * yh_track's state, unchanged, then a gallery (max_tracks, dim) int8, one row g_t per slot.
 * All-zero is the empty state and a zero gallery row means "no feature". No pointers, the same
 * layout on host and device. The yh_track part evolves exactly as yh_track's would under the
 * same matches.
 *
 * Association 1 (status 2 or 3 against the high rows). For slot t and row d: dot = g_t . q_d
 * (int32); cosv = (float)dot / 16129.0f; app = 0.5f + 0.5f * cosv (fp32, one rounding per
 * operation, no FMA); inter and iou as in step 3, iou counting as 0 when inter == 0. The pair is
 * eligible iff g_t and q_d are both non-zero, cosv >= cos_min and iou >= iou_min. It is a
 * candidate iff the class rule holds and (inter != 0 and iou >= iou_first, or it is eligible).
 * Its sort value is the larger of iou and app when eligible, else iou. The walk is step 3's: value
 * descending, then slot, then row; greedy, both sides unmatched. Associations 2 and 3, predict,
 * update, births and output are yh_track's.
 *
 * Gallery update, after step 5: a slot matched in this frame (any association) or born in it,
 * whose row has a feature, takes g = q if g was zero or the slot was born; else, with t_i =
 * 7 g_i + q_i and S = sum t_i^2 (int64), g_i = (int)rint((double)t_i * (127.0 / sqrt((double)S)))
 * (all zero if S == 0). A birth whose row has no feature zeroes its gallery row. Nothing else
 * writes a gallery row; a freed slot keeps its bytes.
 *
 * With embed NULL, or no row having a feature, out, ids, det_index, out_counts and the yh_track
 * part of the state are byte for byte yh_track's.
 *
 * yh_track_reid launches on `stream`: the quantisation into the workspace, yh_embed_similarity's
 * kernel of the galleries (read where they lie in the state, through stream_ids) against it, the
 * track kernel, which reads the similarities, and the gallery update behind it. Asynchronous,
 * allocates nothing, never synchronises, no atomics. yh_track_reid_host: the same bytes.
 * YH_EINVAL as yh_track, and: a bad dim, cos_min or iou_min not finite, a NULL rp or workspace,
 * a workspace smaller than required, a negative capacity. */
typedef struct {
    float cos_min, iou_min;
} yh_reid_params;
size_t yh_track_reid_state_bytes(int streams, int max_tracks, int dim);
size_t yh_track_reid_workspace_bytes(int batch, int max_det, int max_tracks, int dim);
int yh_track_reid(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                  void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                  float* out, int* ids, int* det_index, int* out_counts, const float* embed, int capacity,
                  int dim, const int* feat_counts, const int* embed_total, const yh_reid_params* rp,
                  void* workspace, size_t workspace_bytes, void* stream);
int yh_track_reid_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                       void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                       float* out, int* ids, int* det_index, int* out_counts, const float* embed, int capacity,
                       int dim, const int* feat_counts, const int* embed_total, const yh_reid_params* rp,
                       void* workspace, size_t workspace_bytes, int threads);

/* Batched linear assignment (no reference counterpart: the rules below are the specification;
 * tests/_assign_cases.py restates them in numpy). Problem p has T slots and D rows and a weight
 * matrix weights[p] (T, D) int32: 0 forbids the pair, 1 .. YH_ASSIGN_MAX_WEIGHT is its weight. A
 * weight below 0 is read as 0 and one above YH_ASSIGN_MAX_WEIGHT as YH_ASSIGN_MAX_WEIGHT, so no
 * input can overflow the arithmetic below. t_counts / d_counts: NULL, or (problems) int32 (device
 * memory for yh_assign): only the slots below nt = min(max(t_counts[p], 0), T) and the rows below
 * nd = min(max(d_counts[p], 0), D) take part, and weights outside that corner are never read.
 *
 * Output: row_of_slot (problems, T) int32, the row matched to each slot or -1, and its inverse
 * slot_of_row (problems, D). Every byte of both is written; entries at or beyond nt / nd are -1.
 *
 * Result: a matching over the allowed pairs of maximum total weight. That is not a matching of
 * maximum size (a pair is left out when taking it would cost more weight elsewhere), and a pair
 * of weight 0 is never output. Several matchings can share the maximum; which one is returned is
 * fixed by the algorithm, which is therefore normative: successive shortest augmenting paths
 * (Jonker-Volgenant / the Hungarian method with duals) in integers, with M = YH_ASSIGN_MAX_WEIGHT.
 *   - The columns are the nd rows ("real" columns) and, per slot, one private column only that
 *     slot can use, which stands for staying unmatched. cost(t, d) = M - w for an allowed pair,
 *     cost(t, private t) = M; forbidden pairs do not exist. Duals u[t] = 0, v[d] = 0 at the start;
 *     a private column's dual stays 0.
 *   - For root = 0 .. nt - 1 in this order, a Dijkstra search over the columns: dist[d] = infinity,
 *     no column scanned; the slot i = root enters the tree at base = 0. Repeat:
 *       a. the private column of i gets the distance base + M - u[i]; the nearest private column
 *          so far is kept, the lower slot on equal distances;
 *       b. every unscanned real column d with w(i, d) > 0 is relaxed: cand = base + (M - w) - u[i]
 *          - v[d]; if cand < dist[d] then dist[d] = cand and pred[d] = i;
 *       c. the next column is the unscanned real column of smallest dist, the lowest index on
 *          equal distances, unless the nearest private column is strictly nearer (a real column
 *          comes before a private one) or no real column has been reached: then the path ends at
 *          that private column, total = its distance;
 *       d. the chosen real column d is scanned. If it is free the path ends there, total =
 *          dist[d]. Otherwise its slot enters the tree: i = slot_of_row[d], base = dist[d].
 *   - The duals are updated: u[root] += total; for every scanned column d other than the end,
 *     with delta = total - dist[d]: u[slot_of_row[d]] += delta, v[d] -= delta.
 *   - Then the path is flipped from its end back to the root along pred. A slot whose path ends
 *     at its private column is unmatched.
 * All arithmetic is int32 and exact: a path is never longer than M (the root's private column),
 * so a dual moves by at most M per root, and with at most YH_ASSIGN_MAX_SIZE roots every dual and
 * every distance stays below (YH_ASSIGN_MAX_SIZE + 2) * M < 2^27. Because every choice above is a
 * minimum under a total order, the result does not depend on how the scan over the columns is
 * parallelised.
 *
 * yh_assign: device pointers, one workgroup per problem, asynchronous on `stream`, allocates
 * nothing, never synchronises, no atomics. yh_assign_host: the same bytes for host pointers,
 * problems in parallel over `threads` (<= 0: all hardware threads), synchronous.
 * YH_EINVAL (message in yh_last_error()): T or D above YH_ASSIGN_MAX_SIZE, a negative size, a NULL
 * required pointer (none is required when there is nothing to read or write). */
#define YH_ASSIGN_MAX_WEIGHT (1 << 16)
#define YH_ASSIGN_MAX_SIZE 1024
int yh_assign(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts,
              const int32_t* d_counts, int32_t* row_of_slot, int32_t* slot_of_row, void* stream);
int yh_assign_host(const int32_t* weights, int problems, int T, int D, const int32_t* t_counts,
                   const int32_t* d_counts, int32_t* row_of_slot, int32_t* slot_of_row, int threads);

/* yh_track and yh_track_reid with a choice of how an association picks among its candidate pairs.
 * Arguments, state, outputs and errors are those of yh_track / yh_track_reid, plus ap (mode; set the
 * reserved words to 0). A sequence may change the mode from frame to frame: the state
 * layout is the same.
 *   YH_ASSIGN_GREEDY   byte for byte yh_track / yh_track_reid (which are these functions in this
 *                      mode): the sorted walk of step 3.
 *   YH_ASSIGN_OPTIMAL  in each of the three assoc calls of step 3 (and in yh_track_reid's
 *                      association 1) the candidate pairs and their sort value val are unchanged
 *                      (for yh_track val is the iou, for yh_track_reid's association 1 the larger
 *                      of iou and app when eligible), but instead of the walk the matching is
 *                      yh_assign's on the weights w = 1 + (int)(val * 65535.0f) (one fp32
 *                      multiply, a truncation, clamped to [1, YH_ASSIGN_MAX_WEIGHT]) for candidate
 *                      pairs and 0 for all others, over the association's slots and rows in
 *                      ascending order. It maximises the sum of val over the gated pairs (lapjv
 *                      with a cost limit maximises the sum of val - thr). Steps 1, 2, 4, 5, 6 and
 *                      the gallery update are untouched.
 * YH_EINVAL as the plain functions, and: a NULL ap, an unknown mode. */
#define YH_ASSIGN_GREEDY 0
#define YH_ASSIGN_OPTIMAL 1
typedef struct {
    int mode;
    int reserved[3];
} yh_assign_params;
int yh_track2(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
              void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
              float* out, int* ids, int* det_index, int* out_counts, const yh_assign_params* ap, void* stream);
int yh_track2_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                   void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                   float* out, int* ids, int* det_index, int* out_counts, const yh_assign_params* ap, int threads);
int yh_track_reid2(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                   void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                   float* out, int* ids, int* det_index, int* out_counts, const float* embed, int capacity,
                   int dim, const int* feat_counts, const int* embed_total, const yh_reid_params* rp,
                   void* workspace, size_t workspace_bytes, const yh_assign_params* ap, void* stream);
int yh_track_reid2_host(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                        void* state, int streams, int max_tracks, const yh_track_params* p, int max_out,
                        float* out, int* ids, int* det_index, int* out_counts, const float* embed, int capacity,
                        int dim, const int* feat_counts, const int* embed_total, const yh_reid_params* rp,
                        void* workspace, size_t workspace_bytes, const yh_assign_params* ap, int threads);

/* Identity search over a gallery of int8 features (no reference counterpart: the rules below are
 * the specification; tests/_gallery_cases.py restates them in numpy). The gallery is a caller-owned
 * database of yh_embed_quantize rows that outlives streams and tracks: yh_gallery_search returns
 * the k best rows of each query without ever writing the (nq, n) score matrix, yh_gallery_enrol
 * appends rows. dim follows the rule above (dim % 64 == 0, 64 <= dim <= YH_REID_MAX_DIM).
 *
 * yh_gallery_search
 *   gallery:   (capacity, dim) int8, row-major; capacity <= YH_GALLERY_MAX_CAPACITY
 *   labels:    (capacity) int32, or NULL
 *   size:      (1) int32, or NULL
 *   q:         (nq, dim) int8
 *   nq_count:  (1) int32, or NULL
 *   k:         1 .. YH_GALLERY_MAX_K
 *   scores, index: (nq, k) int32
 *   workspace: caller-owned, yh_gallery_workspace_bytes(capacity, nq, k, chunk_rows) bytes; its
 *              contents mean nothing between calls
 * n = clamp(*size, 0, capacity), or capacity when size is NULL. m = clamp(*nq_count, 0, nq), or nq
 * when nq_count is NULL. Row g is a candidate of query i iff g < n and (labels == NULL or
 * labels[g] >= 0). Its score is the exact int32 dot product of the two rows; any int8 value is
 * legal, -128 included. The candidates of a query are ordered by score descending, then g
 * ascending, and the first k are written: scores[i][j], index[i][j] = g. Positions beyond the
 * number of candidates get score INT32_MIN and index -1. A query row i >= m, or one whose bytes
 * are all zero ("no feature"), has no candidates. Every element of scores and index is written
 * exactly once; nothing else is written outside the workspace. Rows at or beyond n never
 * influence a result (the device does not read them).
 *
 * chunk_rows: 0, or a positive multiple of 64. The gallery is cut into chunks of that many rows
 * (0: the library chooses, as a function of capacity and nq), each chunk is searched on its own
 * and the chunks' lists are merged. The result does not depend on it; it exists so that a gallery
 * of a few hundred rows exercises many chunks and the merge. The workspace holds k candidates of
 * 8 bytes per chunk and query, rounded up to 256 bytes: it never grows with capacity x nq.
 *
 * yh_gallery_enrol appends query rows to the gallery without a read-back.
 *   gallery, labels: as above, written; both required when capacity > 0
 *   size:       (1) int32, read and written, required
 *   take:       (nq) int32, or NULL (every row)
 *   labels_in:  (nq) int32, or NULL
 *   next_label: (1) int32, read and written; required when labels_in is NULL, untouched otherwise
 *   rows_out:   (nq) int32
 * With n = clamp(*size, 0, capacity) and m as above, the query rows are walked in ascending order.
 * Row i is enrolled iff i < m, (take == NULL or take[i] != 0), q_i has a non-zero byte and n <
 * capacity. Enrolling copies the dim bytes of q_i to gallery row n, sets labels[n] = labels_in ?
 * labels_in[i] : (*next_label)++, writes rows_out[i] = n and increments n. Every other rows_out[i]
 * is -1. At the end *size = n. q must not overlap the gallery.
 *
 * On the device both calls are asynchronous on `stream`, allocate nothing, never synchronise and
 * use no atomics; every pointer is device memory, and gallery, q and workspace must be 16-byte
 * aligned. The search is the gfx950 int8 MFMA (v_mfma_i32_32x32x32_i8) with the queries in LDS
 * and the running k best of every query on chip, then a merge of the chunks; the enrolment is one
 * launch (a workgroup prefix sum over the flags, then the copy). The *_host twins give the same
 * bytes; the search splits the queries over `threads` (<= 0: every hardware thread).
 * YH_EINVAL (message in yh_last_error()), nothing launched: a bad dim, k outside [1,
 * YH_GALLERY_MAX_K], a negative size, a capacity above YH_GALLERY_MAX_CAPACITY, a chunk_rows that
 * is negative or no multiple of 64, a workspace that is NULL or too small, a NULL required
 * pointer (none is required when there is nothing to read or write), a misaligned device operand. */
#define YH_GALLERY_MAX_K 32
#define YH_GALLERY_MAX_CAPACITY 2147482624   /* 2^31 - 1024 */
size_t yh_gallery_workspace_bytes(int capacity, int nq, int k, int chunk_rows);
int yh_gallery_search(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                      const int8_t* q, int nq, const int32_t* nq_count, int k, int chunk_rows, int32_t* scores,
                      int32_t* index, void* workspace, size_t workspace_bytes, void* stream);
int yh_gallery_search_host(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                           const int8_t* q, int nq, const int32_t* nq_count, int k, int chunk_rows, int32_t* scores,
                           int32_t* index, void* workspace, size_t workspace_bytes, int threads);
int yh_gallery_enrol(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q, int nq,
                     const int32_t* nq_count, const int32_t* take, const int32_t* labels_in, int32_t* next_label,
                     int32_t* rows_out, void* stream);
int yh_gallery_enrol_host(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q,
                          int nq, const int32_t* nq_count, const int32_t* take, const int32_t* labels_in,
                          int32_t* next_label, int32_t* rows_out, int threads);

/* Letterbox geometry of one image for a square canvas of `size` (dataset.py:95-103,
 * 292-313): resized height / width (int(h * r), int(w * r) with r = size / max(h, w);
 * unchanged when r == 1) and the top / left border. */
int yh_letterbox_geometry(int height, int width, int size, int* new_h, int* new_w, int* top, int* left);

/* Eval-mode preprocessing of a batch of decoded images, on the device:
 *   srcs[i]: device uint8 HWC BGR image of heights[i] x widths[i], row stride
 *            strides[i] bytes (strides may be NULL: 3 * width)
 *   dst:     device uint8 (batch, 3, size, size) RGB CHW: the image resized as
 *            cv2.resize INTER_LINEAR does (11-bit fixed point; exact 2x
 *            downscales as INTER_AREA) and centred on a zero border.
 * Asynchronous on `stream`. yh_letterbox_host computes the same bytes for one
 * image in host memory (dst (3, size, size)); `threads` > 1 splits the rows. */
int yh_letterbox(const void* const* srcs, const int* heights, const int* widths, const int* strides,
                 int batch, int size, void* dst, void* stream);
int yh_letterbox_host(const void* src, int height, int width, int stride, int size, void* dst, int threads);

/* Video front end: BGR or NV12 frames onto a rectangular canvas, one launch per 32 frames.
 *
 *   frames:  host array of `batch` descriptors; the planes are device memory for
 *            yh_letterbox_frames and host memory for the two _host calls
 *   dst:     uint8 (batch, 3, canvas_h, canvas_w), RGB, CHW - the input of yh_forward_u8 (which
 *            needs both canvas sides to be multiples of 32; the letterbox itself needs
 *            canvas_w % 4 == 0). Every byte is written.
 * yh_letterbox_frames is asynchronous on `stream`, allocates nothing and never synchronises.
 * yh_letterbox_frames_host computes the same bytes for one frame (dst (3, canvas_h, canvas_w));
 * `threads` > 1 splits the rows. yh_letterbox / yh_letterbox_host are these two calls for BGR
 * frames on a square canvas.
 *
 * Geometry (yh_letterbox_geometry2), in double: r = min(canvas_h / height, canvas_w / width);
 * if r != 1, new_w = (int)(width * r) and new_h = (int)(height * r), else the frame's own size;
 * top = nearbyint((canvas_h - new_h) / 2.0 - 0.1), left likewise from the widths. For
 * canvas_h == canvas_w == size, r is the same division as size / max(height, width), so the
 * result equals yh_letterbox_geometry's exactly.
 *
 * NV12 to BGR: integer arithmetic with shift 20, limited range, nearest chroma - pixel (y, x)
 * uses the U, V pair at (y >> 1, x >> 1). Constants (CY, CUB, CUG, CVG, CVR):
 *   YH_YUV_BT601  (1220542, 2116026, -409993, -852492, 1673527) = round(c * 2^20) of 1.164,
 *                 2.018, -0.391, -0.813, 1.596 (OpenCV's published COLOR_YUV2BGR_NV12 constants)
 *   YH_YUV_BT709  (1220542, 2214593, -223347, -558891, 1880097) = round(c * 2^20) of 1.164,
 *                 2.112, -0.213, -0.533, 1.793
 * With yy = max(0, Y - 16) * CY, u = U - 128, v = V - 128:
 *   R = sat_u8((yy + (1 << 19) + CVR * v) >> 20)
 *   G = sat_u8((yy + (1 << 19) + CVG * v + CUG * u) >> 20)
 *   B = sat_u8((yy + (1 << 19) + CUB * u) >> 20)
 * cv2 is not available to the tests, so parity against cv2 itself is unpinned (as for the resize).
 *
 * Composition: for an NV12 frame the canvas is, byte for byte, the BGR letterbox of
 * yh_nv12_to_bgr_host(frame): resize, INTER_AREA fast path, vector/scalar tail rule, border and
 * channel flip are those of yh_letterbox. Only the source taps the resize reads are converted;
 * no BGR image is materialised.
 *
 * YH_EINVAL (message in yh_last_error()): an NV12 frame of odd height or width, a stride smaller
 * than the row, a NULL required plane, an unknown format or matrix, a resized side below 1 or
 * beyond the canvas, canvas_w % 4 != 0 (yh_letterbox_frames). Nothing is launched then. */
#define YH_PIX_BGR   0   /* HWC BGR uint8, as yh_letterbox */
#define YH_PIX_NV12  1   /* plane0 = Y (height x width), plane1 = interleaved U,V (height/2 rows of width bytes) */
#define YH_YUV_BT601 0   /* limited range; OpenCV's COLOR_YUV2BGR_NV12 */
#define YH_YUV_BT709 1   /* limited range */
typedef struct {
    const void* plane0; const void* plane1;   /* plane1 ignored for BGR */
    int height, width;                        /* NV12: both even */
    int stride0, stride1;                     /* bytes per row; 0 = tight */
    int format, matrix;
} yh_frame;
int yh_letterbox_geometry2(int height, int width, int canvas_h, int canvas_w, int* new_h, int* new_w, int* top,
                           int* left);
int yh_letterbox_frames(const yh_frame* frames, int batch, int canvas_h, int canvas_w, void* dst, void* stream);
int yh_letterbox_frames_host(const yh_frame* frame, int canvas_h, int canvas_w, void* dst, int threads);
int yh_nv12_to_bgr_host(const yh_frame* frame, void* dst_bgr /* height x width x 3, tight */);

/* Fixed-size crops of detections from their source frames, for a second-stage model: one launch
 * per 32 frames, nothing read back. (No reference counterpart: the rules below are the
 * specification; tests/_crop_cases.py restates them in numpy.)
 *
 *   frames:  host array of `batch` descriptors as for yh_letterbox_frames (BGR or NV12, mixed, any
 *            sizes, strided rows); the planes are device memory for yh_crop_rois and host memory
 *            for yh_crop_rois_host
 *   boxes:   (batch, max_rois, box_stride) f32, box_stride >= 4; columns 0..3 are x1, y1, x2, y2
 *            in the pixels of frame b (box_stride 6: the rows of yh_nms, yh_merge and yh_track)
 *   counts:  (batch) int32, clamped to [0, max_rois]; rows at or beyond it are never read
 *   crops:   (capacity, 3, out_h, out_w) uint8, RGB, CHW (4-byte aligned on the device)
 *   rois:    (capacity, 6) int32: frame, row, x0, y0, w, h
 *   total:   (1) int32
 * Every byte of crops, rois and total is written.
 *
 * 1. Compaction. With n_b the clamped counts, row r of frame b has slot s = n_0 + ... + n_(b-1) + r.
 *    Rows with s >= capacity are dropped; total = min(sum n_b, capacity); slots at or beyond total
 *    are zero in crops and in rois.
 * 2. Rectangle, in fp32 with one rounding per operation:
 *      bw = x2 - x1; bh = y2 - y1; px = bw * pad; py = bh * pad;
 *      X1 = x1 - px; Y1 = y1 - py; X2 = x2 + px; Y2 = y2 + py.
 *    If any of the four is not finite the ROI is empty. Otherwise, clamped in float before the
 *    conversion, x0 = (int)min(max(floorf(X1), 0), W), ix1 = (int)min(max(ceilf(X2), 0), W),
 *    w = ix1 - x0, and y0, h alike with H. The ROI is empty if w < 1 or h < 1. An empty ROI keeps
 *    its slot: its rois row is (b, r, 0, 0, 0, 0) and its crop is zero.
 * 3. Pixels. Let V be the BGR view [y0 : y0 + h, x0 : x0 + w] of the frame (of the frame's
 *    yh_nv12_to_bgr_host image for NV12; a tap is converted where it is read, with the chroma pair
 *    of the absolute pixel, so odd origins are legal and no BGR frame is materialised).
 *      keep_aspect = 1: the crop is the letterbox of V on an out_h x out_w canvas
 *                       (yh_letterbox_frames_host); where yh_letterbox_geometry2 rejects
 *                       (h, w, out_h, out_w) - a resized side below 1 - the ROI is empty as in 2.
 *      keep_aspect = 0: V resized to out_h x out_w with the same three paths (copy for equal
 *                       sizes, the exact-2x area path, else linear with the vector/scalar tail of
 *                       a 3 * out_w byte row): yh_resize_linear_host of V, flipped to RGB, CHW.
 * 4. YH_EINVAL (message in yh_last_error()), nothing launched: a negative batch, max_rois or
 *    capacity; out_h < 1; out_w < 4 or out_w % 4 != 0; box_stride < 4; pad negative or not finite;
 *    keep_aspect outside {0, 1}; a NULL required pointer; a frame that yh_nv12_to_bgr_host's
 *    validation rejects (each frame is checked against its own size as canvas). batch == 0 or
 *    capacity == 0 is valid: total = 0.
 *
 * yh_crop_rois is asynchronous on `stream`, allocates nothing and never synchronises; the device
 * and the host compute the same bytes. yh_crop_rois_host splits the slots over `threads`
 * (<= 0: every hardware thread) and is synchronous. */
int yh_crop_rois(const yh_frame* frames, int batch, const float* boxes, int box_stride, const int* counts,
                 int max_rois, int out_h, int out_w, int keep_aspect, float pad, int capacity, void* crops,
                 int* rois, int* total, void* stream);
int yh_crop_rois_host(const yh_frame* frames, int batch, const float* boxes, int box_stride, const int* counts,
                      int max_rois, int out_h, int out_w, int keep_aspect, float pad, int capacity, void* crops,
                      int* rois, int* total, int threads);

/* Camera-motion compensation for the tracker (no reference counterpart: the rules below are the
 * specification; tests/_motion_cases.py restates them in numpy). yh_track predicts a track with its
 * own velocity and gates on the IoU with the new rows, which assumes a camera at rest. yh_motion
 * estimates the global translation between a stream's previous and current frame from their luma,
 * yh_track_warp (below) moves the stream's tracks by it before the frame's yh_track* call - BoT-SORT's
 * and ultralytics' global-motion step. Everything up to the last few fp32 operations is integer
 * arithmetic: the device and the host compute the same bytes.
 *
 *   frames:     host array of `batch` descriptors as for yh_letterbox_frames (BGR or NV12, mixed, any
 *               sizes, strided rows); the planes are device memory for yh_motion and host memory for
 *               yh_motion_host. Row b is the next frame of stream stream_ids[b] (NULL: of stream b;
 *               device memory for yh_motion); the ids must be distinct. Frames of one stream must
 *               arrive in order and keep their size.
 *   state:      yh_motion_state_bytes(streams, thumb_h, thumb_w) bytes, all-zero = no previous frame.
 *               Per stream a 16-byte header (word 0 is 1 once a thumbnail is stored, the other words
 *               are 0) and the stream's last thumbnail, thumb_h * thumb_w bytes; behind the `streams`
 *               blocks a staging area of 32 thumbnails: batch row b leaves its current thumbnail in
 *               slot b % 32 (the thumbnail launch needs a place for it while the search still reads
 *               the previous one; the host writes the same bytes). No pointers, the same bytes on host
 *               and device: the state can be copied between them in the middle of a sequence.
 *   motion:     (batch, 3) f32: s, tx, ty - the rows of yh_track_warp. sad: (batch, 2) int32.
 *               Every byte of both is written.
 *
 * 1. Luma. NV12: the Y byte. BGR: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 (OpenCV's fixed-point
 *    BGR2GRAY).
 * 2. Thumbnail. Pixel (i, j) covers the source rows (i * H) / thumb_h .. ((i + 1) * H) / thumb_h and the
 *    columns alike (integer divisions, the end exclusive); its value is (sum + n / 2) / n over the
 *    box's n luma bytes, unsigned and exact.
 * 3. Search. With C the current and P the stored thumbnail and R = radius, for every (dy, dx) in
 *    [-R, R]^2: SAD(dy, dx) = sum |C[i][j] - P[i - dy][j - dx]| over i in [R, thumb_h - R), j in
 *    [R, thumb_w - R). The best shift minimises (SAD, |dy| + |dx|, dy, dx) lexicographically.
 * 4. Refinement, fp32, one rounding per operation, no FMA. With s0 the best SAD and sm, sp the SADs at
 *    dx - 1 and dx + 1 in the same row: if |dx| < R and den = (sm - s0) + (sp - s0) > 0,
 *    fx = (0.5f * (float)(sm - sp)) / (float)den, else fx = 0; fy alike along dy. Then
 *    tx = ((float)dx + fx) * ((float)W / (float)thumb_w), ty = ((float)dy + fy) * ((float)H / (float)thumb_h).
 * 5. Output. motion[b] = (1, tx, ty), sad[b] = (s0, SAD(0, 0)). Without a previous frame: (1, 0, 0)
 *    and (0, 0). If max_mad >= 0 and s0 > max_mad * (thumb_h - 2 R) * (thumb_w - 2 R) - a scene cut, or a
 *    match not to be trusted - motion is (1, 0, 0) and sad still reports both values. A row whose id
 *    is outside [0, streams) writes (1, 0, 0) and (0, 0) and touches no state. In every other case C
 *    becomes the stream's thumbnail and the header word is set.
 * Sign: content at source pixel (x, y) of the previous frame is at about (x + tx, y + ty) now.
 * Limits of the model: one translation per frame, found to within a fraction of a thumbnail pixel and
 * at most R thumbnail pixels long; no rotation, zoom, rolling shutter or parallax, and a moving
 * foreground that fills much of the frame pulls the estimate towards its own motion.
 *
 * yh_motion: asynchronous on `stream`, allocates nothing, never synchronises, uses no atomics; two
 * launches per 32 frames; state 4-byte aligned. yh_motion_host: the same bytes for host pointers, rows
 * in parallel over `threads` (<= 0: all hardware threads), synchronous.
 * YH_EINVAL (message in yh_last_error()), nothing launched or written: a frame yh_letterbox_frames'
 * validation rejects, or smaller than the thumbnail (or so much larger that a box sum could pass
 * 2^32); thumb_w % 4 != 0; radius outside [1, YH_MOTION_MAX_RADIUS]; thumb_h - 2 radius < 4 or
 * thumb_w - 2 radius < 4; thumb_h * thumb_w > YH_MOTION_MAX_THUMB (both thumbnails then fit the
 * workgroup's LDS); a negative size; a NULL required pointer. */
#define YH_MOTION_MAX_RADIUS 32
#define YH_MOTION_MAX_THUMB 32768
size_t yh_motion_state_bytes(int streams, int thumb_h, int thumb_w);
int yh_motion(const yh_frame* frames, int batch, const int* stream_ids, void* state, int streams,
              int thumb_h, int thumb_w, int radius, int max_mad, float* motion /* (batch, 3) */,
              int32_t* sad /* (batch, 2) */, void* stream);
int yh_motion_host(const yh_frame* frames, int batch, const int* stream_ids, void* state, int streams,
                   int thumb_h, int thumb_w, int radius, int max_mad, float* motion, int32_t* sad, int threads);

/* Apply a motion to the tracks of a batch's streams before the frame's yh_track* call (no reference
 * counterpart; tests/_motion_cases.py restates the rule). state: yh_track's (reid_dim 0; a stream's
 * block is yh_track_state_bytes(1, max_tracks) bytes) or yh_track_reid's (reid_dim = its dim; the
 * block is yh_track_reid_state_bytes(1, max_tracks, reid_dim) bytes). motion (batch, 3) f32: s, tx, ty
 * of batch row b, whose stream is stream_ids[b] (NULL: b) as for yh_track.
 * For a row with a valid id and finite s > 0, tx, ty, every slot whose status is not 0 is warped, in
 * fp32 with one rounding per operation and no FMA; s2 = s * s:
 *   x[0] = s * x[0] + tx; x[1] = s * x[1] + ty; x[2] = s * x[2]; x[3] = s * x[3];
 *   v[i] = s * v[i]; a[i] = s2 * a[i]; b[i] = s2 * b[i]; c[i] = s2 * c[i].
 * With s == 1 only the two centre coordinates change bits. A row with an invalid id, or a motion that
 * is not finite or has s <= 0, changes nothing. Free slots, the header words and the gallery bytes are
 * never written.
 * Translation plus isotropic scale is all the state can represent: its four filters (cx, cy, w, h) are
 * independent, and a rotation or shear would couple cx with cy. yh_motion only ever emits s = 1; the
 * scale is for callers with an estimate of their own (zoom telemetry).
 * yh_track_warp: device pointers, one workgroup per batch row, asynchronous on `stream`, allocates
 * nothing, never synchronises. yh_track_warp_host: the same bytes in host memory.
 * YH_EINVAL: a negative batch or streams, max_tracks outside [1, YH_TRACK_MAX_TRACKS], reid_dim neither
 * 0 nor a legal feature length, a NULL required pointer. Nothing is launched or written then. */
int yh_track_warp(void* state, int streams, int max_tracks, int reid_dim /* 0: yh_track's state */,
                  const float* motion /* (batch, 3): s, tx, ty */, const int* stream_ids, int batch, void* stream);
int yh_track_warp_host(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                       const int* stream_ids, int batch, int threads);

/* cv2.resize(src, (new_w, new_h), INTER_LINEAR) of one uint8 HWC 3-channel host image
 * (the resize step alone; dst is new_h x new_w x 3, channel order kept). */
int yh_resize_linear_host(const void* src, int height, int width, int stride, int new_h, int new_w, void* dst);

/* Per-op instrumentation (bench / roofline). With profiling enabled,
 * yh_forward launches the ops eagerly with a HIP event pair around each op on
 * the caller's stream, synchronises at the end and accumulates per-op elapsed
 * milliseconds. Disabled by default (forward then runs as a HIP graph). */
int yh_profile_enable(yh_handle* h, int enable);
int yh_profile_reset(yh_handle* h);

/* Number of ops (kernel launch groups) in the forward. */
int yh_op_count(const yh_handle* h);

/* Describe op `index` for an input of (batch, height, width): label (module
 * path), class (0 dense 3x3 conv, 1 dense 1x1 conv, 2 stem conv, 3 depthwise,
 * 4 SPPF pools, 5 PSA attention, 6 head decode, 7 fused head cls branch,
 * 8 fused box tail with DFL, 9 fused C3k2 block, 10 fused C3k block, 11 unused (no op reports it;
 * the later numbers keep their values), 12 pointwise chain, 13 classifier head: pool, fused conv + pool, linear + softmax),
 * algorithmic bytes (each
 * operand read once, each output written once, handle dtype) and FLOPs per
 * call, accumulated profiled milliseconds and call count. */
int yh_op_info(const yh_handle* h, int index, int batch, int height, int width,
               const char** label, int* op_class, double* bytes, double* flops,
               double* ms_total, int* calls);

/* Use a captured HIP graph for yh_forward (default on). */
int yh_set_graph(yh_handle* h, int enable);

/* Kernel that runs op `index` at (batch, height, width): for a dense conv of a
 * 16-bit handle the conv_mx plan the per-shape tuner picked on the first
 * yh_forward at that shape (e.g. "mxr_k3s1_na2_mb2_b1x2_nb2"; every plan is
 * bit-identical), "gemm_f32" on the fp32 handle, for the other ops the op's
 * kernel name. YH_ESTATE before that forward. */
int yh_op_kernel(const yh_handle* h, int index, int batch, int height, int width, const char** name);

/* Force conv plan `kernel` (an index into each conv's candidate list, clamped)
 * on every dense conv, or -1 to return to per-shape autotuning. Drops the tuned
 * choices and captured graphs. Testing hook: every plan must produce
 * bit-identical outputs. */
int yh_force_conv_kernel(yh_handle* h, int kernel);

/* Launch units of the forward at (batch, height, width), known after the first
 * yh_forward at that shape: a unit is one op's kernel (is_level is always 0; the
 * fused level programs of ABI 1 are gone).
 * yh_unit_count returns the count (YH_ESTATE before that forward). With
 * yh_profile_enable, ms_total / calls accumulate per unit. */
int yh_unit_count(const yh_handle* h, int batch, int height, int width);
int yh_unit_info(const yh_handle* h, int index, int batch, int height, int width, int* first_op,
                 int* num_ops, int* is_level, double* ms_total, int* calls);

/* Parity taps (tests/test_gpu_op_parity.py; no reference counterpart: they expose the
 * per-module intermediates nets/nn.py:28-270 computes, so each fused / 16-bit kernel can be
 * checked against the fp64 oracle on its own device-produced inputs).
 *
 * yh_debug_op_desc writes a JSON description of op `index` at (batch, height, width) into buf
 * (NUL-terminated; returns its length, or a negative status): kind, label, "active" (1 if the
 * op launches at this shape, 0 if a fused alternative replaces it, -1 before the first
 * yh_forward there), the convs it computes ({name, k, s, g, act, cin, cout, bias}, in the
 * op's order, null for an absent one) and its workspace operands ({role, H, W, C, logical,
 * up}: inputs "in0"/"in1"/"res"/"x<l>"/"L<l>", outputs "out"/"y<l>"; an op whose output
 * is the caller's y, or whose input is the caller's x, lists no operand for it).
 *
 * yh_debug_run_ops launches the active ops in [first, last) eagerly on `stream`, after a
 * yh_forward at the same shape (x_u8: x is the uint8 image tensor). Running 0..n in steps
 * reproduces yh_forward's workspace and y exactly.
 *
 * yh_debug_operand copies operand `slot` (the desc's order) of op `index` out of the
 * workspace into dst as a dense (batch, H, W, C) array of the handle dtype, async on stream;
 * dst_bytes must equal that array's size at the workspace's current shape (YH_EINVAL otherwise). */
int yh_debug_op_desc(const yh_handle* h, int index, int batch, int height, int width, char* buf, size_t size);
int yh_debug_run_ops(yh_handle* h, const void* x, int x_u8, int batch, int height, int width, void* y, int first,
                     int last, void* stream);
int yh_debug_operand(const yh_handle* h, int index, int slot, void* dst, size_t dst_bytes, void* stream);

/* The 16-bit epilogues activate two adjacent outputs at once on a register pair (silu2<T>).
 * yh_debug_silu_pairs (tests/test_gpu_epilogue_pairs.py) runs the scalar silu<T> and silu2<T> of
 * dtype YH_F16 / YH_BF16 over the n floats at device pointer x, elements 2k and 2k + 1 forming a
 * pair, and writes both results as fp32 bit patterns to the device arrays y_scalar and y_pair
 * (n uint32 each), on the current device's null stream, asynchronously. */
int yh_debug_silu_pairs(int dtype, const void* x, void* y_scalar, void* y_pair, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* YOLO_HIP_H */
