// Cross-tile detection merge (yh_merge): maps the NMS output of a batch of tiles back to the
// source images (inverse letterbox + crop offset, clipped) and, for images cut into several
// tiles, removes duplicates with a second greedy NMS - one launch for all images of a call.
// The host twin is csrc/merge_host.cpp; the semantics are stated there and in include/yolo_hip.h.
// The map, the sort key and the kill test of a row are shared with it through csrc/merge_host.h.
//
// One workgroup of MERGE_T threads per image, no communication between workgroups, no atomics.
//   phase 1  slot s = (tile, row) of the image's tile range gets a 64-bit key in LDS: inverted
//            score bits above the position (single-tile images: the position alone, so the
//            order below is input order); invalid / dropped rows get the all-ones sentinel,
//            which sorts last;
//   phase 2  bitonic sort of the keys over the next power of two (>= 64);
//   phase 3  sorted candidate s belongs to thread s % MERGE_T, register slot s / MERGE_T: the
//            thread maps the row again (same operations, same bits) and keeps box, score,
//            class and area in registers;
//   phase 4  the walk, 64 sorted candidates (one chunk) at a time. Chunk c lies in one wave
//            (wave c % 16, slot c / 16): that wave resolves the chunk alone with lane reads
//            and ballots, writes the kept rows to `out` and their boxes to LDS; after a
//            barrier every thread tests its later candidate of the same slot (the next up to
//            MERGE_T sorted candidates) against the chunk's kept boxes. When the walk enters
//            the next slot, its candidates first catch up against all rows kept so far, read
//            back from `out`. Candidates the walk never reaches (it stops at max_out) are
//            never tested. Two barriers per chunk; every loop bound around a barrier is read
//            from LDS after a barrier or derived from kernel arguments: workgroup-uniform.
//   phase 5  rows beyond the count are zeroed, the count is stored.
// Rows at or beyond a tile's count are never read: they are uninitialised memory.
// LDS: the kept-box reads of phase 4 are one address per wave (a broadcast); the sort's 8-byte
// accesses at distance j < 32 are 2-way conflicts, at most 15 of the 91 passes at the cap.
// Built with -ffp-contract=off: map and IoU must round exactly as the host twin.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "merge_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int MERGE_T = 1024;                          // threads per workgroup (16 waves)
constexpr int MERGE_WAVES = MERGE_T / 64;
constexpr int MERGE_SLOTS = YH_MERGE_MAX_CAND / MERGE_T;   // sorted candidates per thread
constexpr uint64_t MERGE_NONE = ~(uint64_t)0;
static_assert(YH_MERGE_MAX_CAND % MERGE_T == 0 && MERGE_SLOTS >= 1, "candidates are dealt out MERGE_T at a time");
// LDS plan: the keys, 6 x 64 floats of kept boxes, 4 control words
constexpr size_t MERGE_LDS = (size_t)YH_MERGE_MAX_CAND * 8 + 6 * 64 * sizeof(float) + 16;
// above the 64 KiB a workgroup gets by default: launch_merge requests the size with the attribute
// csrc/c3k.hip uses (up to 160 KiB per workgroup on gfx950)
static_assert(MERGE_LDS <= 160 * 1024, "LDS plan");

// lane i's value of v, i wave-uniform (v_readlane_b32: no LDS round trip)
__device__ inline float lane_value(float v, int i) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

__global__ __launch_bounds__(MERGE_T) void merge_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        int tiles, int max_det, const float* __restrict__ tile_xf,
                                                        const int* __restrict__ tile_offsets,
                                                        const float* __restrict__ image_wh, int max_tiles, double iou,
                                                        int max_out, float* __restrict__ out,
                                                        int* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);                    // [YH_MERGE_MAX_CAND]
    float* kbox = reinterpret_cast<float*>(keys + YH_MERGE_MAX_CAND);      // [6][64] x1 y1 x2 y2 cls area
    int* ctl = reinterpret_cast<int*>(kbox + 6 * 64);                      // [0] kept so far, [1] kept in the chunk

    const int img = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // the tile range, clamped to the tile axis and to max_tiles (<= YH_MERGE_MAX_CAND / max_det:
    // the slots below never exceed the keys)
    int lo = tile_offsets[img], hi = tile_offsets[img + 1];
    lo = lo < 0 ? 0 : (lo > tiles ? tiles : lo);
    hi = hi < lo ? lo : (hi > tiles ? tiles : hi);
    if (hi - lo > max_tiles) hi = lo + max_tiles;
    const bool suppress = hi - lo != 1;
    const float W = image_wh[2 * img], H = image_wh[2 * img + 1];
    const int used = (hi - lo) * max_det;              // <= max_tiles * max_det <= YH_MERGE_MAX_CAND
    int n2 = 64;
    while (n2 < used) n2 <<= 1;

    // phase 1
    for (int s = tid; s < n2; s += MERGE_T) {
        uint64_t key = MERGE_NONE;
        if (s < used) {
            const int tl = s / max_det, r = s - tl * max_det, t = lo + tl;
            int cnt = counts[t];
            cnt = cnt < 0 ? 0 : (cnt > max_det ? max_det : cnt);
            if (r < cnt) {
                const float* d = dets + ((size_t)t * max_det + r) * 6;
                yh_merge_box b;
                if (yh_merge_map_row(d, tile_xf + 6 * (size_t)t, W, H, b))
                    key = suppress ? yh_merge_sort_key(d[4], (uint32_t)s) : (uint64_t)(uint32_t)s;
            }
        }
        keys[s] = key;
    }
    if (tid == 0) {
        ctl[0] = 0;
        ctl[1] = 0;
    }
    __syncthreads();
    // phase 2: ascending bitonic sort of keys[0 .. n2)
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += MERGE_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t a = keys[i], b = keys[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
    // phase 3
    yh_merge_box box[MERGE_SLOTS];
    float score[MERGE_SLOTS], cls[MERGE_SLOTS], area[MERGE_SLOTS];
    bool alive[MERGE_SLOTS];
#pragma unroll
    for (int k = 0; k < MERGE_SLOTS; ++k) {
        const int s = k * MERGE_T + tid;
        const uint64_t key = s < n2 ? keys[s] : MERGE_NONE;
        alive[k] = key != MERGE_NONE;
        box[k] = yh_merge_box{0.0f, 0.0f, 0.0f, 0.0f};
        score[k] = cls[k] = area[k] = 0.0f;
        if (alive[k]) {
            const int pos = (int)(uint32_t)key;         // < used
            const int tl = pos / max_det, r = pos - tl * max_det, t = lo + tl;
            const float* d = dets + ((size_t)t * max_det + r) * 6;
            yh_merge_map_row(d, tile_xf + 6 * (size_t)t, W, H, box[k]);
            score[k] = d[4];
            cls[k] = d[5];
            area[k] = (box[k].x2 - box[k].x1) * (box[k].y2 - box[k].y1);
        }
    }
    // phase 4
    float* rows = out + (size_t)img * max_out * 6;
    int kept = 0;          // workgroup-uniform: ctl[0] as of the last barrier
    bool go = true;        // workgroup-uniform
#pragma unroll
    for (int k = 0; k < MERGE_SLOTS; ++k) {
        // The walk enters slot k: its MERGE_T candidates have not met the boxes kept so far (the
        // cross-chunk test below stays inside the current slot, so the candidates the walk never
        // reaches cost nothing). Catch up against the kept rows, read back from `out` 64 at a
        // time through the kept-box buffer; the barriers at the end of the last chunk ordered
        // those stores. All conditions are workgroup-uniform.
        if (suppress && k > 0 && go && k * MERGE_T < n2 && kept < max_out && keys[k * MERGE_T] != MERGE_NONE) {
            for (int q0 = 0; q0 < kept; q0 += 64) {
                const int nq = kept - q0 < 64 ? kept - q0 : 64;
                if (tid < nq) {
                    const float* r = rows + (size_t)(q0 + tid) * 6;
                    const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
                    kbox[tid] = x1;
                    kbox[64 + tid] = y1;
                    kbox[128 + tid] = x2;
                    kbox[192 + tid] = y2;
                    kbox[256 + tid] = r[5];
                    kbox[320 + tid] = (x2 - x1) * (y2 - y1);     // the same bits as the owner's area
                }
                __syncthreads();
                if (alive[k]) {
                    for (int q = 0; q < nq; ++q) {
                        if (cls[k] == kbox[256 + q] &&
                            yh_merge_kills(kbox[q], kbox[64 + q], kbox[128 + q], kbox[192 + q], kbox[320 + q], box[k],
                                           area[k], iou)) {
                            alive[k] = false;
                            break;
                        }
                    }
                }
                __syncthreads();
            }
        }
        for (int w = 0; w < MERGE_WAVES && go; ++w) {
            const int base = (k * MERGE_WAVES + w) * 64;
            // all threads read the same LDS word; the sentinel sorts last, so the first empty chunk ends the walk
            if (base >= n2 || kept >= max_out || keys[base] == MERGE_NONE) {
                go = false;
                break;
            }
            if (wave == w) {
                unsigned long long live = __ballot(alive[k]);
                if (suppress) {
                    for (int i = 0; i < 63; ++i) {
                        if (!((live >> i) & 1ull)) continue;     // wave-uniform
                        const float kx1 = lane_value(box[k].x1, i), ky1 = lane_value(box[k].y1, i);
                        const float kx2 = lane_value(box[k].x2, i), ky2 = lane_value(box[k].y2, i);
                        const float kc = lane_value(cls[k], i), ka = lane_value(area[k], i);
                        const bool kill = lane > i && ((live >> lane) & 1ull) && cls[k] == kc &&
                                          yh_merge_kills(kx1, ky1, kx2, ky2, ka, box[k], area[k], iou);
                        live &= ~__ballot(kill);
                    }
                }
                const int room = max_out - kept;
                const int rank = __popcll(live & ((1ull << lane) - 1ull));
                const int all = __popcll(live);
                if (((live >> lane) & 1ull) && rank < room) {
                    float* o = rows + (size_t)(kept + rank) * 6;
                    o[0] = box[k].x1; o[1] = box[k].y1; o[2] = box[k].x2; o[3] = box[k].y2;
                    o[4] = score[k]; o[5] = cls[k];
                    kbox[rank] = box[k].x1;
                    kbox[64 + rank] = box[k].y1;
                    kbox[128 + rank] = box[k].x2;
                    kbox[192 + rank] = box[k].y2;
                    kbox[256 + rank] = cls[k];
                    kbox[320 + rank] = area[k];
                }
                if (lane == 0) {
                    const int nk = all < room ? all : room;
                    ctl[0] = kept + nk;
                    ctl[1] = nk;
                }
                alive[k] = false;
            }
            __syncthreads();
            kept = ctl[0];
            const int nk = ctl[1];
            if (suppress && alive[k] && k * MERGE_T + tid >= base + 64) {   // the later candidates of this slot
                for (int q = 0; q < nk; ++q) {
                    if (cls[k] == kbox[256 + q] &&
                        yh_merge_kills(kbox[q], kbox[64 + q], kbox[128 + q], kbox[192 + q], kbox[320 + q], box[k],
                                       area[k], iou)) {
                        alive[k] = false;
                        break;
                    }
                }
            }
            __syncthreads();   // the next chunk's wave rewrites kbox / ctl
        }
    }
    // phase 5
    for (int i = kept * 6 + tid; i < max_out * 6; i += MERGE_T) rows[i] = 0.0f;
    if (tid == 0) out_counts[img] = kept;
}

}  // namespace

int launch_merge(const float* dets, const int* counts, int tiles, int max_det, const float* tile_xf,
                 const int* tile_offsets, const float* image_wh, int images, int max_tiles, double iou_threshold,
                 int max_out, float* out, int* out_counts, hipStream_t s) {
    // arguments were checked by yh_merge (yh_merge_check): 1 <= max_tiles, max_tiles * max_det <= YH_MERGE_MAX_CAND
    if (images <= 0) return 0;
    if (int rc = lds_optin(reinterpret_cast<const void*>(merge_kernel), (int)MERGE_LDS)) return rc;
    hipLaunchKernelGGL(merge_kernel, dim3(images), dim3(MERGE_T), MERGE_LDS, s, dets, counts, tiles, max_det, tile_xf,
                       tile_offsets, image_wh, max_tiles, iou_threshold, max_out, out, out_counts);
    return (int)hipGetLastError();
}

}  // namespace yh
