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
#include <algorithm>
#include <cstring>
#include <vector>

#include "host_parallel.h"
#include "track_host.h"

namespace {

struct Pair {
    uint32_t ord;   // yh::float_order(iou)
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

template <class FS, class FR>
void assoc(Frame& fr, FS slot_live, FR row_live, float thr, int class_aware) {
    std::vector<Pair> pairs;
    const int T = (int)fr.status.size();
    for (int t = 0; t < T; ++t) {
        if (!slot_live(t)) continue;
        for (int d = 0; d < fr.n; ++d) {
            if (!row_live(d)) continue;
            const float* r = fr.dets + 6 * (size_t)d;
            if (class_aware && !(fr.tcls[t] == r[5])) continue;
            float iou;
            if (!yh_trk_pair(fr.tbox[t], row_box(r), thr, iou)) continue;
            pairs.push_back({yh::float_order(iou), t, d});
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

// one frame of one stream; w: the stream's state words
void track_stream(const float* dets, int count, int max_det, uint32_t* w, int T, const yh_track_params& p,
                  int max_out, float* out, int* ids, int* det_index, int* out_count) {
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
    assoc(fr, [&](int t) { return fr.status[t] == 2 || fr.status[t] == 3; }, high, p.iou_first, p.class_aware);
    assoc(fr, [&](int t) { return fr.status[t] == 2 && fr.mrow[t] < 0; }, low, p.iou_second, p.class_aware);
    assoc(fr, [&](int t) { return fr.status[t] == 1; }, [&](int d) { return high(d) && fr.mslot[d] < 0; },
          p.iou_tentative, p.class_aware);
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
    }
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

int yh_track_host_run(const float* dets, const int* counts, int batch, int max_det, const int* stream_ids,
                      void* state, int streams, int max_tracks, const yh_track_params* p, int max_out, float* out,
                      int* ids, int* det_index, int* out_counts, int threads) {
    const size_t words = yh_track_stream_words(max_tracks);
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
        track_stream(dets + (size_t)b * max_det * 6, counts[b], max_det,
                     static_cast<uint32_t*>(state) + (size_t)s * words, max_tracks, *p, max_out, o, oi, od,
                     out_counts + b);
    };
    yh::parallel_strided(batch, threads, run);
    return 0;
}
