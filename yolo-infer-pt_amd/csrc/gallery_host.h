// Internal interface of csrc/gallery_host.cpp (HIP-free): the argument checks shared by the device
// and the host entry points of yh_gallery_search / yh_gallery_enrol, the host twins, and - because
// the kernels (csrc/gallery.hip) and the twins must give the same bytes - the order of two
// candidates, the chunking and the workspace layout, written once for both. The C ABI wrappers live
// in post_abi.cpp. The semantics are stated in include/yolo_hip.h.
#ifndef YH_GALLERY_HOST_H
#define YH_GALLERY_HOST_H

#include <cstddef>
#include <cstdint>

#include "box_math.h"   // YH_HD
#include "yolo_hip.h"

// A candidate (score, row) as one unsigned word whose order is the result's: score descending, then
// row ascending. A row is >= 0, so the low word of a key is >= 2^31 and no key is 0: 0 is "no
// candidate", below every key.
YH_HD uint64_t yh_gal_key(int32_t score, int32_t row) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)~row;
}
YH_HD int32_t yh_gal_key_score(uint64_t key) { return key ? (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u) : INT32_MIN; }
YH_HD int32_t yh_gal_key_row(uint64_t key) { return key ? (int32_t)~(uint32_t)key : -1; }

YH_HD int yh_gal_clamp(const int* p, int hi) {
    if (!p) return hi;
    const int v = *p;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

// Rows of a chunk. chunk_rows 0: the library's choice - about 256 workgroups (chunks x tiles of 64
// queries) at a large capacity, one per CU (a workgroup's LDS leaves room for no second one, and
// the longer a chunk, the sooner its lists stop changing), at least 8 chunks, and never below
// 256 rows. It depends on the capacity and on nq only, so the workspace does too.
inline int yh_gal_chunk_rows(int capacity, int nq, int chunk_rows) {
    if (chunk_rows > 0) return chunk_rows;
    const long long tiles = nq > 64 ? ((long long)nq + 63) / 64 : 1;
    const long long want = tiles >= 32 ? 8 : 256 / tiles;
    long long rows = (((long long)capacity + want - 1) / want + 63) / 64 * 64;
    if (rows < 256) rows = 256;
    return (int)rows;
}
inline long long yh_gal_chunks(int capacity, int nq, int chunk_rows) {
    const int rows = yh_gal_chunk_rows(capacity, nq, chunk_rows);
    return ((long long)capacity + rows - 1) / rows;
}
// The workspace: per chunk and query the k best keys of the chunk, (chunks, nq, k) words of 8
// bytes, rounded up to 256 bytes. Nothing in it is of size capacity x nq.
inline size_t yh_gal_ws_bytes(int capacity, int nq, int k, int chunk_rows) {
    const size_t bytes = (size_t)yh_gal_chunks(capacity, nq, chunk_rows) * (size_t)nq * (size_t)k * 8;
    return (bytes + 255) & ~(size_t)255;
}

// NULL when the arguments are acceptable, else the message for yh_last_error() (YH_EINVAL).
const char* yh_gallery_search_check(const void* gallery, int capacity, int dim, const void* q, int nq, int k,
                                    int chunk_rows, const void* scores, const void* index, const void* workspace,
                                    size_t workspace_bytes);
const char* yh_gallery_enrol_check(const void* gallery, const void* labels, const void* size, int capacity, int dim,
                                   const void* q, int nq, const void* labels_in, const void* next_label,
                                   const void* rows_out);

// The host twins proper; arguments already checked. The queries run in parallel over `threads`
// (<= 0: every hardware thread); the enrolment is one walk.
int yh_gallery_search_host_run(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                               const int8_t* q, int nq, const int32_t* nq_count, int k, int32_t* scores,
                               int32_t* index, int threads);
int yh_gallery_enrol_host_run(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q,
                              int nq, const int32_t* nq_count, const int32_t* take, const int32_t* labels_in,
                              int32_t* next_label, int32_t* rows_out);

#endif
