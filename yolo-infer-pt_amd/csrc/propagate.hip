// Track propagation over the frames the detector skips (yh_propagate, yh_propagate_remember): a
// template search per remembered track, at the track's own scale, in the full-resolution frame. The
// semantics are stated in include/yolo_hip.h; the host twin is csrc/propagate_host.cpp, and the state
// layout, the geometry and the result arithmetic are shared with it through csrc/propagate_host.h.
// Everything but the last few fp32 operations is integer arithmetic, so no summation order needs
// fixing. No atomics, no allocation; the frame descriptors of up to YH_PROP_LAUNCH batch rows travel
// as kernel arguments.
//
// build_cells    the part both kernels share: a square of cells - box means of cw x ch luma bytes,
//                pixel coordinates clamped into the frame - into LDS. A wave owns a row of cells; a
//                lane owns 4 consecutive source pixels at a frame column that is a multiple of 4 (one
//                dword of an NV12 row, three of a BGR row, unpacked in registers; byte loads with
//                clamped coordinates where the group crosses the frame's edge or the rows are not
//                dword aligned) and adds their lumas down the cell's ch source rows in registers. The
//                column sums go to the wave's strip of LDS as 16-bit values (32 rows of 255 fit), and
//                after a barrier lane j adds the cw columns of cell j. Every source byte of the
//                footprint is read once.
// propagate_remember  grid (max_tracks, rows), 256 threads: a workgroup beyond the row's count exits
//                at once; the others build the P x P template of their entry and store the entry's 64
//                header bytes and the template as 256 packed dwords.
// propagate_search    grid (max_tracks, rows), 256 threads: the window of (P + 2 R)^2 cells at a row
//                pitch of 68 bytes (17 dwords: odd, so that the rows of neighbouring dy fall on
//                different banks) and the template (1 KB) in LDS. A lane takes an item (part, dy, c):
//                8 template rows, one dy, the four dx whose window column offset dx + R is 4 c + 0 .. 3.
//                Per template dword: one template read (a broadcast), one new window dword (the pair's
//                other half is the previous step's), three v_alignbyte_b32 and four v_sad_u8. The four
//                parts keep all four waves busy at R = 8 (340 items) and write partial tables, which
//                alias the column sums; their sum is the SAD table. Every thread folds its share of
//                the table into the smallest key (SAD, |dy| + |dx|, dy, dx) - a total order, so the
//                spread over lanes and waves cannot matter -, lane exchanges within a wave, LDS across
//                the four; thread 0 refines, moves the box, applies the gate and leaves a 32-byte
//                record in the workspace.
// propagate_emit      one workgroup of 1024 threads per batch row: a ballot and prefix count over the
//                records in table order, the outputs of the survivors, then the table's compaction in
//                place. An entry only ever moves down, so a chunk of 15 entries is read into registers
//                (4 dwords a thread), and stored behind a barrier: a chunk's stores land on slots whose
//                contents this chunk or an earlier one has already read. Nothing moves when nothing was
//                dropped. Then the new origins, zeros over the vacated slots, the header.
// Built with -ffp-contract=off and without packed fp32: the refinement must round as in the host twin.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "propagate_host.h"
#include "yolo_hip.h"

namespace yh {

namespace {

constexpr int P = YH_PROP_P;
constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_PITCH = 68;                         // window row pitch, bytes
constexpr int PR_SIDE = P + 2 * YH_PROPAGATE_MAX_RADIUS;
constexpr int PR_COLS = PR_SIDE * YH_PROP_CMAX + 16; // column sums of a wave: the widest row and the alignment's slack
constexpr int PR_PARTS = 4;                          // template row groups of a search item
constexpr int PR_TABLE = (2 * YH_PROPAGATE_MAX_RADIUS + 1) * (2 * YH_PROPAGATE_MAX_RADIUS + 1);
constexpr int PE_THREADS = 1024;
constexpr int PE_DWORDS = YH_PROP_ENTRY / 4;         // 272
constexpr int PE_PER = 4;                            // dwords a thread carries per chunk
constexpr int PE_CHUNK = PE_THREADS * PE_PER / PE_DWORDS;   // 15 entries
static_assert(PR_WAVES * PR_COLS * 2 <= PR_PARTS * PR_TABLE * 4, "the column sums fit the partial tables' bytes");
static_assert(P * P / 4 == PR_THREADS, "a thread per template dword");
static_assert(YH_PROPAGATE_MAX_TRACKS <= PR_THREADS, "propagate_emit ranks the entries with its first four waves");

struct PropFrame {
    const unsigned char* p0;
    int h, w, stride0, format;
    int aligned;   // p0 and stride0 are multiples of 4: whole groups take the dword loads
};

struct PropBatch {
    PropFrame fr[YH_PROP_LAUNCH];
    const int* stream_ids;   // the launch's first row (or NULL)
    unsigned char* state;
    int b0, streams, max_tracks;
};

__device__ inline unsigned byte_of(unsigned v, int k) { return (v >> (8 * k)) & 0xffu; }

// Cells (i, j) in [-R, P + R)^2 relative to (oy, ox) -> win[(i + R) * pitch + (j + R)]. Called by all
// PR_THREADS threads with uniform arguments; ends with a barrier. colsum: PR_WAVES * PR_COLS values.
__device__ void build_cells(const PropFrame& f, int oy, int ox, int ch, int cw, int R, unsigned char* win, int pitch,
                            uint16_t* colsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = P + 2 * R;
    const int xw0 = ox - R * cw;                     // the first column of the footprint, unclamped
    const int xa = xw0 & ~3;                         // the multiple of 4 at or below it
    const int groups = (xw0 + S * cw - xa + 3) >> 2; // <= (3 + 2048 + 3) / 4: 4 * groups <= PR_COLS
    uint16_t* cs = colsum + wave * PR_COLS;
    const bool nv12 = f.format == YH_PIX_NV12;
    for (int it = 0; it < (S + PR_WAVES - 1) / PR_WAVES; ++it) {
        const int wi = it * PR_WAVES + wave;         // the wave's row of cells
        if (wi < S) {
            const int y0 = oy + (wi - R) * ch;
            for (int g = lane; g < groups; g += 64) {
                const int x0 = xa + 4 * g;
                unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                const bool whole = f.aligned && x0 >= 0 && x0 + 4 <= f.w;
                for (int t = 0; t < ch; ++t) {
                    const unsigned char* row = f.p0 + (size_t)yh_prop_clamp(y0 + t, f.h) * f.stride0;
                    if (whole && nv12) {
                        const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x0);
                        a0 += byte_of(v, 0); a1 += byte_of(v, 1); a2 += byte_of(v, 2); a3 += byte_of(v, 3);
                    } else if (whole) {
                        const uint32_t* p = reinterpret_cast<const uint32_t*>(row + (size_t)x0 * 3);
                        const uint32_t u = p[0], v = p[1], w = p[2];
                        a0 += yh_motion_luma(byte_of(u, 0), byte_of(u, 1), byte_of(u, 2));
                        a1 += yh_motion_luma(byte_of(u, 3), byte_of(v, 0), byte_of(v, 1));
                        a2 += yh_motion_luma(byte_of(v, 2), byte_of(v, 3), byte_of(w, 0));
                        a3 += yh_motion_luma(byte_of(w, 1), byte_of(w, 2), byte_of(w, 3));
                    } else {
                        unsigned l[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int x = yh_prop_clamp(x0 + q, f.w);
                            if (nv12) {
                                l[q] = row[x];
                            } else {
                                const unsigned char* p = row + (size_t)x * 3;
                                l[q] = yh_motion_luma(p[0], p[1], p[2]);
                            }
                        }
                        a0 += l[0]; a1 += l[1]; a2 += l[2]; a3 += l[3];
                    }
                }
                cs[4 * g] = (uint16_t)a0; cs[4 * g + 1] = (uint16_t)a1; cs[4 * g + 2] = (uint16_t)a2; cs[4 * g + 3] = (uint16_t)a3;
            }
        }
        __syncthreads();
        if (wi < S && lane < S) {
            const uint16_t* c = cs + (xw0 - xa) + lane * cw;
            unsigned sum = 0;
            for (int u = 0; u < cw; ++u) sum += c[u];
            win[wi * pitch + lane] = (unsigned char)yh_motion_mean(sum, (unsigned)(cw * ch));
        }
        __syncthreads();
    }
}

struct PropRemember {
    PropBatch pb;
    const float* dets;       // the launch's first row
    const int32_t* ids;
    const int* counts;
    int max_det;
};

__global__ __launch_bounds__(PR_THREADS) void propagate_remember(const PropRemember a) {
    __shared__ uint16_t colsum[PR_WAVES * PR_COLS];
    __shared__ __attribute__((aligned(16))) unsigned char cells[P * P];
    const int r = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int s = a.pb.stream_ids ? a.pb.stream_ids[k] : a.pb.b0 + k;   // one address for the workgroup: uniform
    if (s < 0 || s >= a.pb.streams) return;
    const int n = yh_prop_rows(a.counts[k], a.max_det, a.pb.max_tracks);
    unsigned char* blk = a.pb.state + (size_t)s * yh_prop_stream_bytes(a.pb.max_tracks);
    if (r == 0 && tid < 4) reinterpret_cast<uint32_t*>(blk)[tid] = tid == 0 ? (uint32_t)n : 0u;
    if (r >= n) return;
    const float* d = a.dets + ((size_t)k * a.max_det + r) * 6;
    int32_t cw, ch, ox, oy;
    yh_prop_axis(d[0], d[2], &cw, &ox);
    yh_prop_axis(d[1], d[3], &ch, &oy);
    build_cells(a.pb.fr[k], oy, ox, ch, cw, 0, cells, P, colsum);
    unsigned char* slot = blk + YH_PROP_HDR + (size_t)r * YH_PROP_ENTRY;
    if (tid == 0)
        *reinterpret_cast<yh_prop_entry*>(slot) = yh_prop_entry{a.ids[(size_t)k * a.max_det + r], {d[0], d[1], d[2], d[3]}, d[4], d[5],
                                                                cw, ch, ox, oy, ox, oy, {0, 0, 0}};
    reinterpret_cast<uint32_t*>(slot + YH_PROP_ENTRY_HDR)[tid] = reinterpret_cast<const uint32_t*>(cells)[tid];
}

// the smallest 64-bit key of a wave's lanes, in every lane
__device__ inline uint64_t wave_min_key(uint64_t best) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)best, d);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(best >> 32), d);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        if (o < best) best = o;
    }
    return best;
}

struct PropSearch {
    PropBatch pb;
    unsigned char* ws;       // YH_PROP_REC bytes per entry, max_tracks entries per row of the launch
    int R, max_mad;
};

__global__ __launch_bounds__(PR_THREADS) void propagate_search(const PropSearch a) {
    __shared__ __attribute__((aligned(16))) uint32_t scratch[PR_PARTS * PR_TABLE];   // column sums, then partial tables
    __shared__ __attribute__((aligned(16))) unsigned char win[PR_SIDE * PR_PITCH + 8];
    __shared__ uint32_t tmpl[P * P / 4];
    __shared__ int32_t table[PR_TABLE];
    __shared__ uint64_t wkey[PR_WAVES];
    const int r = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, n1 = 2 * R + 1;
    const int s = a.pb.stream_ids ? a.pb.stream_ids[k] : a.pb.b0 + k;   // uniform
    if (s < 0 || s >= a.pb.streams) return;
    const unsigned char* blk = a.pb.state + (size_t)s * yh_prop_stream_bytes(a.pb.max_tracks);
    const uint32_t stored = *reinterpret_cast<const uint32_t*>(blk);
    if ((uint32_t)r >= stored) return;               // r < max_tracks: the grid
    const unsigned char* slot = blk + YH_PROP_HDR + (size_t)r * YH_PROP_ENTRY;
    yh_prop_entry e = *reinterpret_cast<const yh_prop_entry*>(slot);
    yh_prop_sanitize(&e);                            // a state from elsewhere must not index past the LDS or the frame
    // the bytes between and behind the rows: a pair's second dword reaches into them; what it reads
    // there belongs to candidates beyond the radius, which are not stored, but the bytes are defined
    for (int q = tid; q < (PR_SIDE * PR_PITCH + 8) / 4; q += PR_THREADS) reinterpret_cast<uint32_t*>(win)[q] = 0u;
    tmpl[tid] = reinterpret_cast<const uint32_t*>(slot + YH_PROP_ENTRY_HDR)[tid];
    __syncthreads();
    build_cells(a.pb.fr[k], e.oy, e.ox, e.ch, e.cw, R, win, PR_PITCH, reinterpret_cast<uint16_t*>(scratch));
    // A lane takes an item (part, dy, c). Neighbouring lanes differ in c, then dy: one template dword
    // for all of them, window dwords 1 and 17 apart.
    const int cch = ((2 * R) >> 2) + 1, per = n1 * cch;
    const uint32_t* wdw = reinterpret_cast<const uint32_t*>(win);
    for (int item = tid; item < PR_PARTS * per; item += PR_THREADS) {
        const int part = item / per, rest = item - part * per;
        const int dyi = rest / cch, c = rest - dyi * cch;
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int i = part * (P / PR_PARTS); i < (part + 1) * (P / PR_PARTS); ++i) {
            const uint32_t* wr = wdw + (i + dyi) * (PR_PITCH / 4) + c;   // row <= P - 1 + 2 R, dword <= 8 + 8
            const uint32_t* tr = tmpl + i * (P / 4);
            uint32_t lo = wr[0];
#pragma unroll
            for (int q = 0; q < P / 4; ++q) {
                const uint32_t hi = wr[q + 1], t = tr[q];
                a0 = __builtin_amdgcn_sad_u8(t, lo, a0);
                a1 = __builtin_amdgcn_sad_u8(t, __builtin_amdgcn_alignbyte(hi, lo, 1), a1);
                a2 = __builtin_amdgcn_sad_u8(t, __builtin_amdgcn_alignbyte(hi, lo, 2), a2);
                a3 = __builtin_amdgcn_sad_u8(t, __builtin_amdgcn_alignbyte(hi, lo, 3), a3);
                lo = hi;
            }
        }
        uint32_t* t = scratch + part * n1 * n1 + dyi * n1;
        const int o = 4 * c;                         // o + j = dx + R
        t[o] = a0;
        if (o + 1 <= 2 * R) t[o + 1] = a1;
        if (o + 2 <= 2 * R) t[o + 2] = a2;
        if (o + 3 <= 2 * R) t[o + 3] = a3;
    }
    __syncthreads();
    uint64_t best = ~(uint64_t)0;
    for (int q = tid; q < n1 * n1; q += PR_THREADS) {
        uint32_t sum = 0;
#pragma unroll
        for (int part = 0; part < PR_PARTS; ++part) sum += scratch[part * n1 * n1 + q];
        table[q] = (int32_t)sum;
        const int dyi = q / n1, dxi = q - dyi * n1;
        const uint64_t key = yh_motion_key(sum, dyi - R, dxi - R);
        if (key < best) best = key;
    }
    best = wave_min_key(best);
    if (lane == 0) wkey[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PR_WAVES; ++w)
            if (wkey[w] < best) best = wkey[w];
        yh_prop_rec rec;
        yh_prop_result(table, R, best, e, a.pb.fr[k].h, a.pb.fr[k].w, a.max_mad, &rec);
        *reinterpret_cast<yh_prop_rec*>(a.ws + ((size_t)k * a.pb.max_tracks + r) * YH_PROP_REC) = rec;
    }
}

struct PropEmit {
    const int* stream_ids;   // the launch's first row (or NULL)
    unsigned char* state;
    const unsigned char* ws;
    float* dets;             // the launch's first row
    int32_t* ids;
    int32_t* sad;
    int* counts;
    int b0, streams, max_tracks, max_out;
};

__global__ __launch_bounds__(PE_THREADS) void propagate_emit(const PropEmit a) {
    __shared__ int src_of[YH_PROPAGATE_MAX_TRACKS];
    __shared__ int wcount[PR_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = a.stream_ids ? a.stream_ids[k] : a.b0 + k;   // uniform
    const bool valid = s >= 0 && s < a.streams;
    unsigned char* blk = a.state + (size_t)(valid ? s : 0) * yh_prop_stream_bytes(a.max_tracks);
    int n = 0;
    if (valid) {
        const uint32_t stored = *reinterpret_cast<const uint32_t*>(blk);
        n = stored > (uint32_t)a.max_tracks ? a.max_tracks : (int)stored;
    }
    const yh_prop_rec* recs = reinterpret_cast<const yh_prop_rec*>(a.ws) + (size_t)k * a.max_tracks;
    // the survivors in table order: entry t is thread t's, the first four waves hold them all
    const bool ok = tid < n && recs[tid].ok != 0;
    const unsigned long long mask = __ballot(ok);
    if (wave < PR_WAVES && lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, kept = 0;
    for (int w = 0; w < PR_WAVES; ++w) {
        base += w < wave ? wcount[w] : 0;
        kept += wcount[w];
    }
    if (ok) src_of[base + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    float* od = a.dets + (size_t)k * a.max_out * 6;
    int32_t* oi = a.ids + (size_t)k * a.max_out;
    int32_t* os = a.sad + (size_t)k * a.max_out;
    for (int q = tid; q < a.max_out; q += PE_THREADS) {
        float row[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int32_t id = 0, s0 = 0;
        if (q < kept) {
            const int src = src_of[q];
            const yh_prop_entry* e = reinterpret_cast<const yh_prop_entry*>(blk + YH_PROP_HDR + (size_t)src * YH_PROP_ENTRY);
            for (int c = 0; c < 4; ++c) row[c] = recs[src].box[c];
            row[4] = e->score;
            row[5] = e->cls;
            id = e->id;
            s0 = recs[src].s0;
        }
        for (int c = 0; c < 6; ++c) od[(size_t)q * 6 + c] = row[c];
        oi[q] = id;
        os[q] = s0;
    }
    if (tid == 0) a.counts[k] = kept < a.max_out ? kept : a.max_out;
    if (!valid) return;
    __syncthreads();                                 // the outputs have read the entries' old places
    uint32_t* tab = reinterpret_cast<uint32_t*>(blk + YH_PROP_HDR);
    if (kept != n) {
        for (int kb = 0; kb < kept; kb += PE_CHUNK) {
            uint32_t v[PE_PER];
            int dst[PE_PER];
#pragma unroll
            for (int u = 0; u < PE_PER; ++u) {
                const int q = tid + PE_THREADS * u, kk = kb + q / PE_DWORDS, dw = q % PE_DWORDS;
                dst[u] = -1;
                if (q < PE_CHUNK * PE_DWORDS && kk < kept && src_of[kk] != kk) {
                    v[u] = tab[(size_t)src_of[kk] * PE_DWORDS + dw];
                    dst[u] = kk * PE_DWORDS + dw;
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PE_PER; ++u)
                if (dst[u] >= 0) tab[dst[u]] = v[u];
        }
        __syncthreads();
    }
    if (tid < kept) {
        yh_prop_entry* e = reinterpret_cast<yh_prop_entry*>(blk + YH_PROP_HDR + (size_t)tid * YH_PROP_ENTRY);
        e->ox = recs[src_of[tid]].ox;
        e->oy = recs[src_of[tid]].oy;
    }
    for (int q = kept * PE_DWORDS + tid; q < n * PE_DWORDS; q += PE_THREADS) tab[q] = 0u;
    if (tid < 4) reinterpret_cast<uint32_t*>(blk)[tid] = tid == 0 ? (uint32_t)kept : 0u;
}

PropBatch describe_rows(const yh_motion_src* src, int b0, int nb, const int* stream_ids, void* state, int streams,
                        int max_tracks) {
    PropBatch pb{};
    for (int k = 0; k < nb; ++k) {
        const yh_motion_src& f = src[b0 + k];
        pb.fr[k] = PropFrame{f.p0, f.h, f.w, f.stride0, f.format,
                             (reinterpret_cast<uintptr_t>(f.p0) | (uintptr_t)f.stride0) % 4 == 0 ? 1 : 0};
    }
    pb.stream_ids = stream_ids ? stream_ids + b0 : nullptr;
    pb.state = static_cast<unsigned char*>(state);
    pb.b0 = b0; pb.streams = streams; pb.max_tracks = max_tracks;
    return pb;
}

}  // namespace

int launch_propagate_remember(const yh_motion_src* src, int batch, const int* stream_ids, const float* dets,
                              const int32_t* ids, const int* counts, int max_det, void* state, int streams,
                              int max_tracks, hipStream_t s) {
    // arguments were checked by yh_propagate_remember
    for (int b0 = 0; b0 < batch; b0 += YH_PROP_LAUNCH) {
        const int nb = batch - b0 < YH_PROP_LAUNCH ? batch - b0 : YH_PROP_LAUNCH;
        PropRemember a{};
        a.pb = describe_rows(src, b0, nb, stream_ids, state, streams, max_tracks);
        a.dets = dets + (size_t)b0 * max_det * 6;
        a.ids = ids + (size_t)b0 * max_det;
        a.counts = counts + b0;
        a.max_det = max_det;
        hipLaunchKernelGGL(propagate_remember, dim3((unsigned)max_tracks, (unsigned)nb), dim3(PR_THREADS), 0, s, a);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

int launch_propagate(const yh_motion_src* src, int batch, const int* stream_ids, void* state, int streams,
                     int max_tracks, int radius, int max_mad, int max_out, float* dets, int32_t* ids, int32_t* sad,
                     int* counts, void* workspace, hipStream_t s) {
    // arguments were checked by yh_propagate; the launches of a call follow each other on one stream,
    // so the rows of every launch use the same workspace records
    for (int b0 = 0; b0 < batch; b0 += YH_PROP_LAUNCH) {
        const int nb = batch - b0 < YH_PROP_LAUNCH ? batch - b0 : YH_PROP_LAUNCH;
        PropSearch a{};
        a.pb = describe_rows(src, b0, nb, stream_ids, state, streams, max_tracks);
        a.ws = static_cast<unsigned char*>(workspace);
        a.R = radius; a.max_mad = max_mad;
        hipLaunchKernelGGL(propagate_search, dim3((unsigned)max_tracks, (unsigned)nb), dim3(PR_THREADS), 0, s, a);
        if (hipError_t e = hipGetLastError()) return (int)e;
        PropEmit m{};
        m.stream_ids = a.pb.stream_ids;
        m.state = a.pb.state;
        m.ws = a.ws;
        m.dets = dets + (size_t)b0 * max_out * 6;
        m.ids = ids + (size_t)b0 * max_out;
        m.sad = sad + (size_t)b0 * max_out;
        m.counts = counts + b0;
        m.b0 = b0; m.streams = streams; m.max_tracks = max_tracks; m.max_out = max_out;
        hipLaunchKernelGGL(propagate_emit, dim3((unsigned)nb), dim3(PE_THREADS), 0, s, m);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

}  // namespace yh
