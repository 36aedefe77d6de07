// Host twins of yh_gallery_search and yh_gallery_enrol (csrc/gallery.hip): plain loops giving the
// same bytes. The semantics are stated in include/yolo_hip.h; the order of two candidates is
// gallery_host.h's key, as on the device. HIP-free.
#include "gallery_host.h"

#include <algorithm>
#include <cstring>

#include "host_parallel.h"
#include "track_host.h"   // yh_reid_dim_check

const char* yh_gallery_search_check(const void* gallery, int capacity, int dim, const void* q, int nq, int k,
                                    int chunk_rows, const void* scores, const void* index, const void* workspace,
                                    size_t workspace_bytes) {
    if (const char* bad = yh_reid_dim_check(dim)) return bad;
    if (k < 1 || k > YH_GALLERY_MAX_K) return "k must be in [1, YH_GALLERY_MAX_K (" YH_STR(YH_GALLERY_MAX_K) ")]";
    if (capacity < 0 || nq < 0) return "capacity and nq must be >= 0";
    if (capacity > YH_GALLERY_MAX_CAPACITY) return "capacity exceeds YH_GALLERY_MAX_CAPACITY (2^31 - 1024)";
    if (chunk_rows < 0 || chunk_rows % 64) return "chunk_rows must be 0 or a positive multiple of 64";
    if (yh_gal_chunks(capacity, nq, chunk_rows) * (((long long)nq + 63) / 64) > (1ll << 30))
        return "chunk_rows gives more than 2^30 (chunk, query tile) pairs";
    if (nq > 0 && (!scores || !index)) return "null scores / index";
    if (nq > 0 && !q) return "null q";
    if (nq > 0 && capacity > 0 && !gallery) return "null gallery";
    const size_t need = yh_gal_ws_bytes(capacity, nq, k, chunk_rows);
    if (need > 0 && !workspace) return "null workspace";
    if (workspace_bytes < need) return "gallery workspace too small";
    return nullptr;
}

const char* yh_gallery_enrol_check(const void* gallery, const void* labels, const void* size, int capacity, int dim,
                                   const void* q, int nq, const void* labels_in, const void* next_label,
                                   const void* rows_out) {
    if (const char* bad = yh_reid_dim_check(dim)) return bad;
    if (capacity < 0 || nq < 0) return "capacity and nq must be >= 0";
    if (!size) return "null size";
    if (capacity > 0 && (!gallery || !labels)) return "null gallery / labels";
    if (nq > 0 && (!q || !rows_out)) return "null q / rows_out";
    if (!labels_in && !next_label) return "null next_label without labels_in";
    return nullptr;
}

namespace {

bool nonzero_row(const int8_t* r, int dim) {
    for (int i = 0; i < dim; ++i)
        if (r[i]) return true;
    return false;
}

}  // namespace

int yh_gallery_search_host_run(const int8_t* gallery, const int32_t* labels, const int32_t* size, int capacity, int dim,
                               const int8_t* q, int nq, const int32_t* nq_count, int k, int32_t* scores,
                               int32_t* index, int threads) {
    const int n = yh_gal_clamp(size, capacity), m = yh_gal_clamp(nq_count, nq);
    yh::parallel_strided(nq, threads, [&](int i) {
        uint64_t best[YH_GALLERY_MAX_K] = {};   // descending; 0: no candidate
        const int8_t* qr = q + (size_t)i * dim;
        if (i < m && nonzero_row(qr, dim)) {
            for (int g = 0; g < n; ++g) {
                if (labels && labels[g] < 0) continue;
                const int8_t* gr = gallery + (size_t)g * dim;
                int32_t acc = 0;
                for (int e = 0; e < dim; ++e) acc += (int32_t)qr[e] * (int32_t)gr[e];
                const uint64_t key = yh_gal_key(acc, g);
                if (key <= best[k - 1]) continue;
                int j = k - 1;
                for (; j > 0 && best[j - 1] < key; --j) best[j] = best[j - 1];
                best[j] = key;
            }
        }
        for (int j = 0; j < k; ++j) {
            scores[(size_t)i * k + j] = yh_gal_key_score(best[j]);
            index[(size_t)i * k + j] = yh_gal_key_row(best[j]);
        }
    });
    return 0;
}

int yh_gallery_enrol_host_run(int8_t* gallery, int32_t* labels, int32_t* size, int capacity, int dim, const int8_t* q,
                              int nq, const int32_t* nq_count, const int32_t* take, const int32_t* labels_in,
                              int32_t* next_label, int32_t* rows_out) {
    const int m = yh_gal_clamp(nq_count, nq);
    int n = yh_gal_clamp(size, capacity);
    int32_t next = labels_in ? 0 : *next_label;
    for (int i = 0; i < nq; ++i) {
        const int8_t* qr = q + (size_t)i * dim;
        rows_out[i] = -1;
        if (i >= m || (take && !take[i]) || !nonzero_row(qr, dim) || n >= capacity) continue;
        std::memcpy(gallery + (size_t)n * dim, qr, dim);
        labels[n] = labels_in ? labels_in[i] : next++;
        rows_out[i] = n++;
    }
    *size = n;
    if (!labels_in) *next_label = next;
    return 0;
}
