// Host (CPU) twin of the tracker (csrc/track.hip), and the argument check both entry points
// share. HIP-free on purpose: this file compiles alone with any C++17 compiler (build it with
// -ffp-contract=off, as the device file is). The arithmetic of a track and the state layout are
// in csrc/track_host.h, shared with the kernel.
//
// Semantics: the six steps stated at yh_track in include/yolo_hip.h. Where the kernel finds the
// association by rounds of mutual best matching, this file does what the text says: it lists the
// candidate pairs, sorts them (iou descending, then slot, then row) and walks them. Both give
// the same matching: a pair that is the best of its slot and of its row under that strict order
// is preceded by no pair that shares a side with it, so the walk takes it; removing it and
// repeating is the walk.
//
// In YH_ASSIGN_OPTIMAL mode (yh_track2 / yh_track_reid2) the same candidate pairs go, as weights,
// through csrc/assign_host.h's solver instead of the walk.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "assign_host.h"
#include "host_parallel.h"
#include "track_host.h"

namespace {

struct Pair {
    uint32_t ord;   // yh::float_order(sort value)
    int t, d;
};

struct Frame {
    const float* dets;   // (n, 6)
    int n;
    std::vector<yh_track_box> tbox;   // predicted box per slot
    std::vector<float> tcls;
    std::vector<int> status;          // as stored, before this frame
    std::vector<int> mrow;            // slot -> row or -1
    std::vector<int> mslot;           // row -> slot or -1
};

yh_track_box row_box(const float* d) { return yh_track_box{d[0], d[1], d[2], d[3]}; }

// pair(t, d, val): is (slot t, row d) a candidate, and with which sort value?
template <class FS, class FR, class FP>
void assoc(Frame& fr, FS slot_live, FR row_live, int class_aware, FP pair, int mode) {
    std::vector<Pair> pairs;
    const int T = (int)fr.status.size();
    if (mode == YH_ASSIGN_OPTIMAL) {
        // the live slots and rows in ascending order, the candidates' weights between them
        std::vector<int> ts, ds;
        for (int t = 0; t < T; ++t)
            if (slot_live(t)) ts.push_back(t);
        for (int d = 0; d < fr.n; ++d)
            if (row_live(d)) ds.push_back(d);
        const int nt = (int)ts.size(), nd = (int)ds.size();
        if (nt == 0 || nd == 0) return;
        std::vector<int> w((size_t)nt * nd, 0);
        for (int a = 0; a < nt; ++a)
            for (int c = 0; c < nd; ++c) {
                if (class_aware && !(fr.tcls[ts[a]] == fr.dets[6 * (size_t)ds[c] + 5])) continue;
                float val;
                if (pair(ts[a], ds[c], val)) w[(size_t)a * nd + c] = yh_trk_weight(val);
            }
        std::vector<int> ros(nt), sor(nd);
        yh_assign_solve(nt, nd, [&](int a, int c) { return w[(size_t)a * nd + c]; }, ros.data(), sor.data());
        for (int a = 0; a < nt; ++a) {
            if (ros[a] < 0) continue;
            fr.mrow[ts[a]] = ds[ros[a]];
            fr.mslot[ds[ros[a]]] = ts[a];
        }
        return;
    }
    for (int t = 0; t < T; ++t) {
        if (!slot_live(t)) continue;
        for (int d = 0; d < fr.n; ++d) {
            if (!row_live(d)) continue;
            const float* r = fr.dets + 6 * (size_t)d;
            if (class_aware && !(fr.tcls[t] == r[5])) continue;
            float val;
            if (!pair(t, d, val)) continue;
            pairs.push_back({yh::float_order(val), t, d});
        }
    }
    std::sort(pairs.begin(), pairs.end(), [](const Pair& p, const Pair& q) {
        if (p.ord != q.ord) return p.ord > q.ord;
        if (p.t != q.t) return p.t < q.t;
        return p.d < q.d;
    });
    for (const Pair& p : pairs) {
        if (fr.mrow[p.t] >= 0 || fr.mslot[p.d] >= 0) continue;
        fr.mrow[p.t] = p.d;
        fr.mslot[p.d] = p.t;
    }
}

void load_kal(const uint32_t* w, int T, int t, yh_track_kal& k) {
    for (int i = 0; i < 4; ++i) {
        std::memcpy(&k.x[i], w + YH_TRACK_HDR + (size_t)(YH_TRK_X + i) * T + t, 4);
        std::memcpy(&k.v[i], w + YH_TRACK_HDR + (size_t)(YH_TRK_V + i) * T + t, 4);
        std::memcpy(&k.a[i], w + YH_TRACK_HDR + (size_t)(YH_TRK_A + i) * T + t, 4);
        std::memcpy(&k.b[i], w + YH_TRACK_HDR + (size_t)(YH_TRK_B + i) * T + t, 4);
        std::memcpy(&k.c[i], w + YH_TRACK_HDR + (size_t)(YH_TRK_C + i) * T + t, 4);
    }
}

void store_kal(uint32_t* w, int T, int t, const yh_track_kal& k) {
    for (int i = 0; i < 4; ++i) {
        std::memcpy(w + YH_TRACK_HDR + (size_t)(YH_TRK_X + i) * T + t, &k.x[i], 4);
        std::memcpy(w + YH_TRACK_HDR + (size_t)(YH_TRK_V + i) * T + t, &k.v[i], 4);
        std::memcpy(w + YH_TRACK_HDR + (size_t)(YH_TRK_A + i) * T + t, &k.a[i], 4);
        std::memcpy(w + YH_TRACK_HDR + (size_t)(YH_TRK_B + i) * T + t, &k.b[i], 4);
        std::memcpy(w + YH_TRACK_HDR + (size_t)(YH_TRK_C + i) * T + t, &k.c[i], 4);
    }
}

// The appearance side of one frame of one stream (yh_track_reid): the rows' quantised features
// and flags in the workspace, the stream's gallery.
struct Reid {
    const int8_t* q;      // (max_det, dim)
    const int* flags;     // (max_det): bit 0 the row has a feature, bit 1 its q is non-zero
    int8_t* gallery;      // (T, dim)
    int dim;
    yh_reid_params rp;
};

bool nonzero(const int8_t* v, int dim) {
    for (int i = 0; i < dim; ++i)
        if (v[i]) return true;
    return false;
}

// the gallery update of slot t with row d (born: the slot was born in this frame)
void gallery_update(const Reid& r, int t, int d, bool born) {
    int8_t* g = r.gallery + (size_t)t * r.dim;
    if (!(r.flags[d] & 1)) {
        if (born) std::memset(g, 0, r.dim);
        return;
    }
    const int8_t* q = r.q + (size_t)d * r.dim;
    if (born || !nonzero(g, r.dim)) {
        std::memcpy(g, q, r.dim);
        return;
    }
    int64_t S = 0;
    for (int i = 0; i < r.dim; ++i) {
        const int v = 7 * (int)g[i] + (int)q[i];
        S += (int64_t)v * v;
    }
    if (S == 0) {
        std::memset(g, 0, r.dim);
        return;
    }
    const double scale = yh_reid_scale(S);
    for (int i = 0; i < r.dim; ++i) g[i] = (int8_t)yh_reid_round(7 * (int)g[i] + (int)q[i], scale);
}

// one frame of one stream; w: the stream's state words; reid: NULL for yh_track
void track_stream(const float* dets, int count, int max_det, uint32_t* w, int T, const yh_track_params& p,
                  int max_out, float* out, int* ids, int* det_index, int* out_count, const Reid* reid, int mode) {
    std::fill(out, out + (size_t)max_out * 6, 0.0f);
    std::fill(ids, ids + max_out, 0);
    std::fill(det_index, det_index + max_out, 0);
    int* st = reinterpret_cast<int*>(w) + YH_TRACK_HDR + (size_t)YH_TRK_STATUS * T;
    int* id = reinterpret_cast<int*>(w) + YH_TRACK_HDR + (size_t)YH_TRK_ID * T;
    int* last = reinterpret_cast<int*>(w) + YH_TRACK_HDR + (size_t)YH_TRK_LAST * T;
    float* cls = reinterpret_cast<float*>(w) + YH_TRACK_HDR + (size_t)YH_TRK_CLS * T;

    // step 1
    const int f = (int)w[0] + 1;
    w[0] = (uint32_t)f;
    Frame fr;
    fr.dets = dets;
    fr.n = std::min(std::max(count, 0), max_det);
    fr.tbox.assign(T, yh_track_box{0.0f, 0.0f, 0.0f, 0.0f});
    fr.tcls.assign(cls, cls + T);
    fr.status.assign(st, st + T);
    fr.mrow.assign(T, -1);
    fr.mslot.assign(fr.n, -1);
    std::vector<yh_track_kal> kal(T);
    for (int t = 0; t < T; ++t) {
        if (st[t] == 0) continue;
        load_kal(w, T, t, kal[t]);
        yh_trk_predict(kal[t], st[t]);
        fr.tbox[t] = yh_trk_box(kal[t]);
    }
    // step 2
    auto score = [&](int d) { return dets[6 * (size_t)d + 4]; };
    auto high = [&](int d) { return score(d) >= p.track_high; };
    auto low = [&](int d) { return score(d) >= p.track_low && score(d) < p.track_high; };
    // step 3
    auto by_iou = [&](float thr) {
        return [&fr, dets, thr](int t, int d, float& val) {
            return yh_trk_pair(fr.tbox[t], row_box(dets + 6 * (size_t)d), thr, val);
        };
    };
    auto first = [&](int t) { return fr.status[t] == 2 || fr.status[t] == 3; };
    if (reid) {
        std::vector<char> gnz(T, 0);
        for (int t = 0; t < T; ++t) gnz[t] = first(t) && nonzero(reid->gallery + (size_t)t * reid->dim, reid->dim);
        assoc(fr, first, high, p.class_aware, [&](int t, int d, float& val) {
            const bool feat = gnz[t] && (reid->flags[d] & 2);
            int dot = 0;
            if (feat) {
                const int8_t* g = reid->gallery + (size_t)t * reid->dim;
                const int8_t* q = reid->q + (size_t)d * reid->dim;
                for (int i = 0; i < reid->dim; ++i) dot += (int)g[i] * (int)q[i];
            }
            return yh_trk_pair_reid(fr.tbox[t], row_box(dets + 6 * (size_t)d), p.iou_first, feat, dot,
                                    reid->rp.cos_min, reid->rp.iou_min, val);
        }, mode);
    } else {
        assoc(fr, first, high, p.class_aware, by_iou(p.iou_first), mode);
    }
    assoc(fr, [&](int t) { return fr.status[t] == 2 && fr.mrow[t] < 0; }, low, p.class_aware, by_iou(p.iou_second),
          mode);
    assoc(fr, [&](int t) { return fr.status[t] == 1; }, [&](int d) { return high(d) && fr.mslot[d] < 0; },
          p.class_aware, by_iou(p.iou_tentative), mode);
    std::vector<int> grow;   // the gallery's work: slot -> its row of this frame, born ones tagged
    if (reid) {
        grow.assign(T, -1);
        for (int t = 0; t < T; ++t)
            if (st[t] != 0 && fr.mrow[t] >= 0) grow[t] = fr.mrow[t];
    }
    // step 4
    for (int t = 0; t < T; ++t) {
        if (st[t] == 0) continue;
        const int d = fr.mrow[t];
        if (d >= 0) {
            yh_trk_update(kal[t], row_box(dets + 6 * (size_t)d));
            st[t] = 2;
            last[t] = f;
            cls[t] = dets[6 * (size_t)d + 5];
        } else if (st[t] == 2) {
            st[t] = 3;
        } else if (st[t] == 1) {
            st[t] = 0;
        }
        if (st[t] == 3 && f - last[t] > p.max_age) st[t] = 0;
        store_kal(w, T, t, kal[t]);
    }
    // step 5
    int t = 0;
    for (int d = 0; d < fr.n; ++d) {
        if (!(high(d) && fr.mslot[d] < 0 && score(d) >= p.track_new)) continue;
        while (t < T && st[t] != 0) ++t;
        if (t == T) break;
        yh_trk_birth(kal[t], row_box(dets + 6 * (size_t)d));
        store_kal(w, T, t, kal[t]);
        w[1] += 1;
        id[t] = (int)w[1];
        last[t] = f;
        cls[t] = dets[6 * (size_t)d + 5];
        st[t] = f == 1 ? 2 : 1;
        if (f == 1) {   // only these births are output: the others are tentative
            fr.mrow[t] = d;
            fr.mslot[d] = t;
        }
        if (reid) grow[t] = d | (1 << 30);
    }
    if (reid)
        for (int s = 0; s < T; ++s)
            if (grow[s] >= 0) gallery_update(*reid, s, grow[s] & ~(1 << 30), (grow[s] >> 30) != 0);
    // step 6
    int k = 0;
    for (int d = 0; d < fr.n && k < max_out; ++d) {
        const int s = fr.mslot[d];
        if (s < 0) continue;              // every matched slot has status 2 and last frame f
        const yh_track_box b = yh_trk_box(kal[s]);
        float* o = out + 6 * (size_t)k;
        o[0] = b.x1; o[1] = b.y1; o[2] = b.x2; o[3] = b.y2;
        o[4] = score(d); o[5] = dets[6 * (size_t)d + 5];
        ids[k] = id[s];
        det_index[k] = d;
        ++k;
    }
    *out_count = k;
}

}  // namespace

const char* yh_track_check(const void* dets, const void* counts, int batch, int max_det, const void* state,
                           int streams, int max_tracks, const yh_track_params* p, int max_out, const void* out,
                           const void* ids, const void* det_index, const void* out_counts) {
    if (batch < 0) return "batch must be >= 0";
    if (max_det < 0) return "max_det must be >= 0";
    if (streams < 0) return "streams must be >= 0";
    if (max_out < 0) return "max_out must be >= 0";
    if (max_tracks < 1) return "max_tracks must be >= 1";
    if (max_tracks > YH_TRACK_MAX_TRACKS) return "max_tracks exceeds YH_TRACK_MAX_TRACKS (" YH_STR(YH_TRACK_MAX_TRACKS) ")";
    if (max_det > YH_TRACK_MAX_DET) return "max_det exceeds YH_TRACK_MAX_DET (" YH_STR(YH_TRACK_MAX_DET) ")";
    if (!p) return "null params";
    if (p->track_low > p->track_high) return "track_low must be <= track_high";
    if (p->max_age < 0) return "max_age must be >= 0";
    if (batch > 0 && (!counts || !out_counts)) return "null counts / out_counts";
    if (batch > 0 && max_out > 0 && (!out || !ids || !det_index)) return "null out / ids / det_index";
    if (batch > 0 && max_det > 0 && !dets) return "null dets";
    if (batch > 0 && streams > 0 && !state) return "null state";
    return nullptr;
}

const char* yh_reid_dim_check(int dim) {
    if (dim < 64 || dim > YH_REID_MAX_DIM || dim % 64) return "dim must be a multiple of 64 in [64, " YH_STR(YH_REID_MAX_DIM) "]";
    return nullptr;
}

const char* yh_track_reid_check(int batch, int max_det, int max_tracks, int capacity, int dim, const yh_reid_params* rp,
                                const void* workspace, size_t workspace_bytes) {
    if (const char* bad = yh_reid_dim_check(dim)) return bad;
    if (capacity < 0) return "capacity must be >= 0";
    if (!rp) return "null reid params";
    if (!std::isfinite(rp->cos_min) || !std::isfinite(rp->iou_min)) return "cos_min / iou_min must be finite";
    if (batch > 0 && !workspace) return "null workspace";
    if (batch > 0 && workspace_bytes < yh_reid_ws_bytes(batch, max_det, max_tracks, dim)) return "reid workspace too small";
    return nullptr;
}

const char* yh_embed_quantize_check(const void* e, int rows, int dim, const void* q) {
    if (const char* bad = yh_reid_dim_check(dim)) return bad;
    if (rows < 0) return "rows must be >= 0";
    if (rows > 0 && (!e || !q)) return "null e / q";
    return nullptr;
}

const char* yh_embed_similarity_check(const void* a, size_t a_block_stride, int nblocks, const void* b, int batch,
                                      int ra, int rb, int dim, const void* out) {
    if (const char* bad = yh_reid_dim_check(dim)) return bad;
    if (batch < 0 || ra < 0 || rb < 0 || nblocks < 0) return "batch, ra, rb and nblocks must be >= 0";
    if (a_block_stride < (size_t)ra * dim) return "a_block_stride is smaller than a block (ra * dim)";
    if (batch > 0 && ra > 0 && rb > 0 && !out) return "null out";
    if (batch > 0 && ra > 0 && rb > 0 && !b) return "null b";
    if (batch > 0 && ra > 0 && rb > 0 && nblocks > 0 && !a) return "null a";
    return nullptr;
}

void yh_embed_quantize_row(const float* e, int dim, int8_t* q) {
    std::memset(q, 0, dim);
    if (!e) return;
    float m = 0.0f;
    for (int i = 0; i < dim; ++i) {
        if (!std::isfinite(e[i])) return;
        const float a = std::fabs(e[i]);
        if (a > m) m = a;
    }
    if (m == 0.0f) return;
    const double r = 16384.0 / (double)m;
    std::vector<int> pv(dim);
    int64_t S = 0;
    for (int i = 0; i < dim; ++i) {
        pv[i] = (int)rint((double)e[i] * r);
        S += (int64_t)pv[i] * pv[i];
    }
    const double scale = yh_reid_scale(S);   // S >= 16384^2: the largest element
    for (int i = 0; i < dim; ++i) q[i] = (int8_t)yh_reid_round(pv[i], scale);
}

int yh_embed_quantize_host_run(const float* e, int rows, int dim, const int* count, int8_t* q, int threads) {
    const int n = count ? std::min(std::max(*count, 0), rows) : rows;
    yh::parallel_strided(rows, threads, [&](int r) {
        yh_embed_quantize_row(r < n ? e + (size_t)r * dim : nullptr, dim, q + (size_t)r * dim);
    });
    return 0;
}

int yh_embed_similarity_host_run(const int8_t* a, size_t a_block_stride, int nblocks, const int* a_index,
                                 const int8_t* b, int batch, int ra, int rb, int dim, int32_t* out, int threads) {
    yh::parallel_strided(batch * ra, threads, [&](int job) {
        const int bz = job / ra, m = job % ra;
        const int k = a_index ? a_index[bz] : bz;
        int32_t* o = out + ((size_t)bz * ra + m) * rb;
        if (k < 0 || k >= nblocks) {
            std::fill(o, o + rb, 0);
            return;
        }
        const int8_t* ar = a + (size_t)k * a_block_stride + (size_t)m * dim;
        for (int n = 0; n < rb; ++n) {
            const int8_t* br = b + ((size_t)bz * rb + n) * dim;
            int32_t acc = 0;
            for (int i = 0; i < dim; ++i) acc += (int32_t)ar[i] * (int32_t)br[i];
            o[n] = acc;
        }
    });
    return 0;
}

int yh_track_host_run(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                      void* state, int streams, int max_tracks, const yh_track_params* p, int max_out, float* out,
                      int* ids, int* det_index, int* out_counts, int threads, const yh_track_reid_args* ra,
                      int assign_mode) {
    const size_t words = yh_track_stream_words(max_tracks);
    const size_t stride = ra ? yh_track_reid_stream_bytes(max_tracks, ra->dim) : words * 4;
    int8_t* wq = nullptr;
    int* wflags = nullptr;
    if (ra && batch > 0) {
        // the rows' features: yh_crop_rois' compaction, then the quantisation into the workspace
        wq = static_cast<int8_t*>(ra->workspace);
        wflags = reinterpret_cast<int*>(static_cast<char*>(ra->workspace) + yh_reid_ws_flags(batch, max_det, ra->dim));
        long long limit = ra->embed ? ra->capacity : 0;
        if (ra->embed && ra->embed_total) limit = std::min<long long>(limit, *ra->embed_total);
        std::vector<long long> base(batch + 1, 0);
        std::vector<int> nf(batch);
        for (int b = 0; b < batch; ++b) {
            const int c = std::min(std::max(counts[b], 0), max_det);
            nf[b] = ra->feat_counts ? std::min(std::max(ra->feat_counts[b], 0), c) : c;
            base[b + 1] = base[b] + nf[b];
        }
        yh::parallel_strided(batch * max_det, threads, [&](int job) {
            const int b = job / max_det, r = job % max_det;
            const long long s = base[b] + r;
            const bool has = r < nf[b] && s < limit;
            int8_t* q = wq + (size_t)job * ra->dim;
            yh_embed_quantize_row(has ? ra->embed + (size_t)s * ra->dim : nullptr, ra->dim, q);
            wflags[job] = has ? 1 | (nonzero(q, ra->dim) ? 2 : 0) : 0;
        });
    }
    auto run = [&](int b) {
        const int s = stream_ids ? stream_ids[b] : b;
        float* o = out + (size_t)b * max_out * 6;
        int* oi = ids + (size_t)b * max_out;
        int* od = det_index + (size_t)b * max_out;
        if (s < 0 || s >= streams) {
            std::fill(o, o + (size_t)max_out * 6, 0.0f);
            std::fill(oi, oi + max_out, 0);
            std::fill(od, od + max_out, 0);
            out_counts[b] = 0;
            return;
        }
        char* w = static_cast<char*>(state) + (size_t)s * stride;
        Reid reid{};
        if (ra) {
            reid.q = wq + (size_t)b * max_det * ra->dim;
            reid.flags = wflags + (size_t)b * max_det;
            reid.gallery = reinterpret_cast<int8_t*>(w + words * 4);
            reid.dim = ra->dim;
            reid.rp = ra->rp;
        }
        track_stream(dets + (size_t)b * max_det * 6, counts[b], max_det, reinterpret_cast<uint32_t*>(w), max_tracks,
                     *p, max_out, o, oi, od, out_counts + b, ra ? &reid : nullptr, assign_mode);
    };
    yh::parallel_strided(batch, threads, run);
    return 0;
}

const char* yh_track_warp_check(const void* state, int streams, int max_tracks, int reid_dim, const void* motion,
                                int batch) {
    if (batch < 0) return "batch must be >= 0";
    if (streams < 0) return "streams must be >= 0";
    if (max_tracks < 1) return "max_tracks must be >= 1";
    if (max_tracks > YH_TRACK_MAX_TRACKS) return "max_tracks exceeds YH_TRACK_MAX_TRACKS (" YH_STR(YH_TRACK_MAX_TRACKS) ")";
    if (reid_dim != 0)
        if (const char* bad = yh_reid_dim_check(reid_dim)) return bad;
    if (batch > 0 && !motion) return "null motion";
    if (batch > 0 && streams > 0 && !state) return "null state";
    return nullptr;
}

int yh_track_warp_host_run(void* state, int streams, int max_tracks, int reid_dim, const float* motion,
                           const int* stream_ids, int batch, int threads) {
    const size_t stride = yh_track_warp_stride(max_tracks, reid_dim);
    const int T = max_tracks;
    yh::parallel_strided(batch, threads, [&](int b) {
        const int s = stream_ids ? stream_ids[b] : b;
        const float* m = motion + (size_t)b * 3;
        if (s < 0 || s >= streams || !yh_trk_warp_valid(m)) return;
        uint32_t* w = reinterpret_cast<uint32_t*>(static_cast<char*>(state) + (size_t)s * stride);
        const int* st = reinterpret_cast<const int*>(w) + YH_TRACK_HDR + (size_t)YH_TRK_STATUS * T;
        for (int t = 0; t < T; ++t) {
            if (st[t] == 0) continue;
            yh_track_kal k;
            load_kal(w, T, t, k);
            yh_trk_warp(k, m[0], m[1], m[2]);
            store_kal(w, T, t, k);
        }
    });
    return 0;
}
