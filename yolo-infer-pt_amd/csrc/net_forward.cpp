// Workspace, per-shape plans and captured graphs: where the activations live, which ops a forward
// at (B, H, W) launches, and the forward itself (eager, profiled or as one replayed HIP graph).
#include "net.h"

namespace yh {

size_t Net::tensor_bytes(const Tensor& t, int B, int H, int W) const {
    if (t.level < 0) return (size_t)B * t.C * 4;   // one fp32 vector per image
    return (size_t)B * (H >> t.level) * (W >> t.level) * t.C * es;
}
// Tensors are laid out coarsest level first (a classifier's per-image vectors after the maps).
size_t Net::ws_bytes_for(int B, int H, int W, std::vector<size_t>* offs) const {
    size_t total = 0;
    if (offs) offs->assign(tensors.size(), 0);
    for (int lvl = 5; lvl >= -1; --lvl)
        for (size_t i = 0; i < tensors.size(); ++i) {
            const Tensor& t = tensors[i];
            if (t.level != lvl) continue;
            const size_t b = tensor_bytes(t, B, H, W);
            if (offs) (*offs)[i] = total;
            total += (b + 255) & ~(size_t)255;
        }
    return total;
}
void Net::reserve(int B, int H, int W) {
    require(B > 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "input height/width must be positive multiples of 32");
    // the fused stem has no per-layer launch to fall back to: refuse the shape here, before
    // anything is allocated, not at its launch
    for (const Op& op : ops)
        require(op.kind != OP_STEM2 || stem2_size_ok(H, W),
                "input image too large for the fused stem (3 * height * width must be below 2^32); set YH_FUSE=0");
    if (task == 1) check_shape(B, H, W);
    if (ws.base && ws.B == B && ws.H == H && ws.W == W) return;
    std::vector<size_t> offs;
    const size_t need = ws_bytes_for(B, H, W, &offs);
    if (!ws.base || need > ws.bytes) {
        drop_graphs();
        if (ws.base) HIPCHECK(hipFree(ws.base));
        ws.base = nullptr;
        const hipError_t e = hipMalloc(&ws.base, need);
        if (e != hipSuccess) throw Fail(YH_ENOMEM, "workspace allocation failed");
        ws.bytes = need;
    } else if (ws.B != B || ws.H != H || ws.W != W) {
        drop_graphs();
    }
    ws.off = offs;
    ws.B = B;
    ws.H = H;
    ws.W = W;
}

// A classifier handle meets maps down to 1 x 1 (32 x 32 crops): every op without a per-layer
// alternative must have a plan at the shape, or the shape is refused here, before any launch.
void Net::check_shape(int B, int H, int W) const {
    for (const Op& op : ops) {
        if (op.kind == OP_CSP) {
            const int lv = tensors[op.out.t].level;
            int th, tw;
            require(csp_tile(opt.tune, op.cs[0] >= 0 ? convs[op.cs[0]].cin / 16 : 0, convs[op.cs[1]].cin / 16, convs[op.cs[3]].cout / 32,
                             B, H >> lv, W >> lv, 256, th, tw),
                    op.label + ": no tile for a " + std::to_string(H >> lv) + " x " + std::to_string(W >> lv) + " map");
        }
        // cls_pool's grid has one row of workgroups per image
        if (op.kind == OP_CLSPOOL) require(B <= 65535, "classifier batch above 65535");
    }
}

void Net::drop_graphs() {
    // A graph exec (and the plans / workspace it points into) must not be destroyed
    // while a replay is still in flight; a multi-branch exec destroyed mid-replay
    // left libamdhip64 to segfault in a later hipGraphLaunch.
    if (!graphs.empty() || !plans.empty()) {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
    plans.clear();
    cur_plan = nullptr;
}

Net::~Net() {
    drop_graphs();
    for (auto& d : convs) free_conv(d);
    if (ws.base) (void)hipFree(ws.base);
    if (io_dev) (void)hipFree(io_dev);
    if (zero_dev) (void)hipFree(zero_dev);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    for (auto e : ev) (void)hipEventDestroy(e);
}

// whether a fused op with per-layer alternatives (Op::alts) runs at this shape
bool Net::fused_fits(const Op& op, int B, int H, int W) const {
    switch (op.kind) {
        case OP_PWCHAIN: {
            const int lv = tensors[op.out.t].level;
            // a pointwise chain reads every stage's weights once per workgroup: kept where that is at
            // most 160 MB per launch (v11_n b32: 52-90 MB, 104 -> 77 us for its three chains),
            // per-layer launches above (v11_s b64 1.4 GB: the chains ran 2.2x slower,
            // profiles/r05_pw_chain_configs.txt)
            const long long M = (long long)B * (H >> lv) * (W >> lv);
            const double grid = (double)((M + op.pwP - 1) / op.pwP);
            double wb = 0;
            for (int k : op.alts) wb += (double)convs[ops[k].conv].cout * convs[ops[k].conv].K * es;
            return wb * grid <= 160e6;
        }
        case OP_C3K: {
            // a fused C3k block runs where bands of its map fit a workgroup's LDS (c3k_lds), its
            // seven per-layer launches everywhere else
            const int lv = tensors[op.out.t].level;
            return c3k_lds(H >> lv, W >> lv, convs[op.ck[0]].cout) > 0;
        }
        case OP_CLSHEAD:
            // where a workgroup holds at least one whole image's map (cls_head_group; a function
            // of the map and the channels only, never of the batch)
            return cls_head_group(convs[op.conv].K, (H >> 5) * (W >> 5)) > 0;
        default: return true;
    }
}
void Net::ensure_plan(int B, int H, int W) {
    const GraphKey key{B, H, W};
    auto it = plans.find(key);
    if (it != plans.end()) { cur_plan = &it->second; return; }
    Plan pl;
    pl.active.assign(ops.size(), 1);
    // Either a fused op or its alternatives run. The order of the decisions cannot matter: the
    // alternative sets are disjoint and hold no op that has alternatives itself (build(): a C3k
    // op's are its own block's seven convs, and fuse_pw_chains takes only plain convs that are in
    // no other op's set, each for one chain), so every entry of `active` is cleared by at most one op
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].alts.empty()) continue;
        if (fused_fits(ops[i], B, H, W))
            for (int k : ops[i].alts) pl.active[k] = 0;
        else
            pl.active[i] = 0;
    }
    for (size_t i = 0; i < ops.size(); ++i)
        if (pl.active[i]) pl.order.push_back((int)i);
    cur_plan = &plans.emplace(key, std::move(pl)).first->second;
}

void Net::run_ops(int B, int H, int W, hipStream_t s) {
    for (int i : cur_plan->order) launch_op((size_t)i, B, H, W, s);
}

void Net::forward(const void* x, int B, int H, int W, void* y, hipStream_t s, int x_u8) {
    in_u8 = x_u8;
    for (auto& d : convs) require(d.loaded, "weights of " + d.name + " not loaded", YH_ESTATE);
    reserve(B, H, W);
    HIPCHECK(hipSetDevice(device));
    require(launch_set_io(io_dev, x, y, s) == 0, "set_io launch failed", YH_EHIP);
    launch_plan(B, H, W, s);
}

// The classifier's forward (yh_classify): the same plan / tuner / graph machinery; the outputs and
// the count are reached through io_dev, so a replayed graph serves any set of pointers.
void Net::classify(const void* x, int x_u8, int B, int H, int W, const int* count, float* probs, float* logits,
                   float* embed, hipStream_t s) {
    in_u8 = x_u8;
    for (auto& d : convs) require(d.loaded, "weights of " + d.name + " not loaded", YH_ESTATE);
    reserve(B, H, W);
    HIPCHECK(hipSetDevice(device));
    require(launch_set_io_cls(io_dev, x, probs, logits, embed, count, s) == 0, "set_io launch failed", YH_EHIP);
    launch_plan(B, H, W, s);
}

// the plan of (B, H, W) on stream s: profiled, eager or as one replayed graph
void Net::launch_plan(int B, int H, int W, hipStream_t s) {
    ensure_plan(B, H, W);
    ensure_tuned(B, H, W, s);
    if (profile) {   // HIP events around every launch, on the caller's stream
        const std::vector<int>& order = cur_plan->order;
        const size_t nu = order.size();
        if (ev.size() < 2 * nu) {
            for (auto e : ev) (void)hipEventDestroy(e);
            ev.assign(2 * nu, nullptr);
            for (auto& e : ev) HIPCHECK(hipEventCreate(&e));
        }
        if (prof_key.B != B || prof_key.H != H || prof_key.W != W) {
            prof_ms.assign(nu, 0.0);
            prof_calls.assign(nu, 0);
            prof_key = GraphKey{B, H, W};
        }
        for (size_t i = 0; i < nu; ++i) {
            HIPCHECK(hipEventRecord(ev[2 * i], s));
            launch_op((size_t)order[i], B, H, W, s);
            HIPCHECK(hipEventRecord(ev[2 * i + 1], s));
        }
        HIPCHECK(hipEventSynchronize(ev[2 * nu - 1]));
        for (size_t i = 0; i < nu; ++i) {
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            prof_ms[i] += ms;
            prof_calls[i] += 1;
        }
        return;
    }
    if (!use_graph) {
        run_ops(B, H, W, s);
        return;
    }
    const GraphKey key{B, H, W, in_u8};
    auto it = graphs.find(key);
    if (it == graphs.end()) {
        // one eager pass first: every kernel of the plan is then loaded and has its
        // function attributes (dynamic-LDS limits) set outside any stream capture
        run_ops(B, H, W, s);
        if (!cap_stream) HIPCHECK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        hipGraph_t g = nullptr;
        HIPCHECK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
        try {
            run_ops(B, H, W, cap_stream);
        } catch (...) {
            (void)hipStreamEndCapture(cap_stream, &g);
            if (g) (void)hipGraphDestroy(g);
            throw;
        }
        HIPCHECK(hipStreamEndCapture(cap_stream, &g));
        hipGraphExec_t ex = nullptr;
        HIPCHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        it = graphs.emplace(key, ex).first;
    }
    HIPCHECK(hipGraphLaunch(it->second, s));
}

}  // namespace yh
