// Launch arguments, launch_op and the autotuner: every op kind's kernel arguments at a shape, the
// tile choices they depend on, and the per-shape choice of each 16-bit dense conv's conv_mx plan.
#include <algorithm>
#include <cstdio>

#include "net.h"

namespace yh {

// first anchor of detect level l (0..2) for an H x W input (make_anchors order)
int Net::anchor_off(int l, int H, int W) {
    int a = 0;
    for (int k = 0; k < l; ++k) a += (H >> (3 + k)) * (W >> (3 + k));
    return a;
}

// ---------------------------------------------------------- dense convs
static void pick_tile(long long M, int cout, int& BM, int& BN) {
    BN = cout <= 16 ? 16 : cout <= 32 ? 32 : cout <= 64 ? 64 : 128;
    const long long gn = (cout + BN - 1) / BN;
    BM = 64;
    for (int bm : {256, 128}) {
        if (((M + bm - 1) / bm) * gn >= 1024) { BM = bm; break; }
    }
}

void Net::conv_args(const Op& op, int B, int H, int W, ConvArgs& a, int& BM, int& BN) const {
    const ConvDesc& d = convs[op.conv];
    const Tensor& to = tensors[op.out.t];
    const int lvl_in = tensors[op.in[0].v.t].level - op.in[0].up;
    a.Hi = H >> lvl_in; a.Wi = W >> lvl_in;
    a.Ho = H >> to.level; a.Wo = W >> to.level;
    a.stride = d.stride; a.pad = d.k / 2; a.KH = d.k; a.KW = d.k;
    for (size_t si = 0; si < op.in.size(); ++si) {
        const Seg& sg = op.in[si];
        const Tensor& ts = tensors[sg.v.t];
        const int hh = H >> ts.level, ww = W >> ts.level;
        if (si == 0) { a.in0 = ptr(sg.v); a.ldc0 = ts.C; a.c0 = sg.v.C; a.up0 = sg.up; a.h0 = hh; a.w0 = ww; }
        else { a.in1 = ptr(sg.v); a.ldc1 = ts.C; a.c1 = sg.v.C; a.up1 = sg.up; a.h1 = hh; a.w1 = ww; }
    }
    if (op.in.size() == 1) { a.in1 = a.in0; a.ldc1 = a.ldc0; a.c1 = 0; a.up1 = 0; a.h1 = a.h0; a.w1 = a.w0; }
    a.Cin = d.cin_p; a.K = d.K; a.Kp = d.Kp;
    a.M = B * a.Ho * a.Wo;
    a.w = d.w_dev; a.bias = d.b_dev; a.ktab = d.ktab_dev;
    a.out = ptr(op.out); a.ldo = to.C;
    if (op.has_res) { a.res = ptr(op.res); a.ldr = ldc(op.res); }
    a.Cout = d.cout_p;
    a.act = d.act;
    pick_tile(a.M, a.Cout, BM, BN);
    if (a.act == ACT_SILU_F64 && BM > 128) BM = 128;   // conv_gemm's fp64-epilogue instances (conv.hip)
    a.gm = (a.M + BM - 1) / BM;
    a.gn = (a.Cout + BN - 1) / BN;
    a.zero = zero_dev;
    a.ks = 1;
}

// conv_mx (16-bit dense convs)
MxShape Net::mx_shape(const ConvArgs& a, int B) const {
    MxShape sh{};
    sh.ks = a.KH; sh.s = a.stride; sh.cin = a.Cin; sh.cout = a.Cout;
    sh.Hi = a.Hi; sh.Wi = a.Wi; sh.Ho = a.Ho; sh.Wo = a.Wo; sh.B = B;
    sh.c0 = a.c1 ? a.c0 : a.Cin; sh.c1 = a.c1; sh.up0 = a.up0; sh.up1 = a.up1;
    sh.ldo = a.ldo; sh.ldr = a.res ? a.ldr : 0;
    return sh;
}
static std::string mx_name(const MxPlan& p) {
    char b[96];
    if (p.cfg.kind == 2)
        snprintf(b, sizeof(b), "rw_g%d_p%d_mb%d_ns%d_t%dx%d%s", p.cfg.na, p.cfg.wm, p.cfg.mb, p.cfg.nbuf, p.TH, p.TW,
                 p.cfg.gdiv == 2 ? "_d2" : p.cfg.gdiv == 4 ? "_d4" : "");
    else
        snprintf(b, sizeof(b), "%s_na%d_mb%d_w%dx%d_ncb%d_t%dx%d", p.cfg.kind ? "mxr" : "mx", p.cfg.na, p.cfg.mb,
                 p.cfg.wn, p.cfg.wm, p.cfg.ncb, p.TH, p.TW);
    return b;
}
int Net::launch_mx_op(const Op& op, const MxPlan& pl, int B, int H, int W, hipStream_t s) {
    ConvArgs a{};
    int BM, BN;
    conv_args(op, B, H, W, a, BM, BN);
    const MxShape sh = mx_shape(a, B);
    MxArgs m{};
    mx_fill_args(pl, sh, m);
    m.in0 = (const char*)a.in0;
    m.in1 = a.c1 ? (const char*)a.in1 : nullptr;
    m.ldc0 = a.ldc0; m.ldc1 = a.ldc1;
    m.hs0 = a.h0; m.ws0 = a.w0; m.hs1 = a.h1; m.ws1 = a.w1;
    m.w = mx_weights(op.conv, pl, sh);
    m.bias = a.bias;
    m.out = (char*)a.out; m.ldo = a.ldo;
    m.res = (const char*)a.res; m.ldr = a.ldr;
    m.act = a.act;
    m.zero = (const char*)zero_dev;
    return launch_mx(dtype, pl, m, s);
}

// input bytes a plan stages per output pixel and cout slice, relative to one read of the
// input: the tile's patch over its outputs (halo, stride) times the cout slices
static double patch_reads(const MxPlan& pl) {
    const double out = (double)pl.TH * pl.TW;
    const double in = (double)pl.PR * pl.PC / (pl.cfg.ks == 3 && pl.cfg.s == 2 ? 4.0 : 1.0);
    return in / out * pl.nslices;
}

// Pick the conv_mx plan of every dense conv for this shape: one plain forward with
// each layer's default plan (realistic activations in the workspace), then every
// candidate plan of every layer timed over 3 launches after a warm-up launch, each
// right after the forward's preceding op (in situ; the input's cache state of the
// forward: back-to-back launches of one layer favoured plans that re-read a
// MALL-resident input, e.g. net.p3.0's 32-B-per-stage plan at 2x HBM traffic). The
// candidates are bit-identical (one reduction order), so the choice only changes
// speed. Runs outside any graph capture; the next forward recomputes everything.
void Net::ensure_tuned(int B, int H, int W, hipStream_t s) {
    if (dtype == F32) return;   // conv_gemm only
    const GraphKey key{B, H, W};
    auto it = conv_kern.find(key);
    if (it != conv_kern.end()) { cur_kern = &it->second; return; }
    const int forced = force_kern >= 0 ? force_kern : opt.conv_force;
    std::vector<MxChoice> ch(ops.size());
    std::vector<std::vector<MxPlan>> cands(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].kind != OP_CONV) continue;
        ConvArgs a{};
        int BM, BN;
        conv_args(ops[i], B, H, W, a, BM, BN);
        cands[i] = mx_candidates(mx_shape(a, B), num_cus);
        require(!cands[i].empty(), "no conv_mx plan for " + ops[i].label);
        const int pick = forced >= 0 ? std::min(forced, (int)cands[i].size() - 1) : 0;
        ch[i].plan = cands[i][pick];
        ch[i].name = mx_name(ch[i].plan);
    }
    auto& slot = conv_kern[key];
    slot = ch;
    cur_kern = &slot;
    if (forced >= 0) return;
    run_ops(B, H, W, s);
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    const std::vector<char>& act = cur_plan->active;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].kind != OP_CONV || cands[i].size() < 2 || !act[i]) continue;
        int prev = (int)i - 1;
        while (prev >= 0 && !act[prev]) --prev;
        // two interleaved rounds over the candidates, each candidate's faster round kept: one
        // disturbed measurement (another lane's kernels, a clock step) no longer decides a
        // layer's plan for the life of the engine (a bench's roofline forward once read its
        // 3x3 family 17 % slower than the same library's next run)
        std::vector<float> t_ms(cands[i].size(), 3.0e38f);
        for (int round = 0; round < 2; ++round)
        for (size_t c = 0; c < cands[i].size(); ++c) {
            const MxPlan& pl = cands[i][c];
            int rc = launch_mx_op(ops[i], pl, B, H, W, s);
            float ms = 0.f;
            if (prev >= 0) {
                // in situ: each timed launch right after the op that precedes it in the
                // forward, so the input's cache state (just written, L2 / MALL warm, the
                // layer's other operands cold) is the forward's, not a back-to-back loop's
                for (int r = 0; r < 3 && rc == 0; ++r) {
                    launch_op((size_t)prev, B, H, W, s);
                    HIPCHECK(hipEventRecord(e0, s));
                    rc = launch_mx_op(ops[i], pl, B, H, W, s);
                    HIPCHECK(hipEventRecord(e1, s));
                    HIPCHECK(hipEventSynchronize(e1));
                    float t = 0.f;
                    HIPCHECK(hipEventElapsedTime(&t, e0, e1));
                    ms += t;
                }
            } else {
                HIPCHECK(hipEventRecord(e0, s));
                for (int r = 0; r < 3 && rc == 0; ++r) rc = launch_mx_op(ops[i], pl, B, H, W, s);
                HIPCHECK(hipEventRecord(e1, s));
                HIPCHECK(hipEventSynchronize(e1));
                HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
            }
            if (rc != 0) throw Fail(YH_EHIP, "tuning launch of " + ops[i].label + " failed");
            if (opt.tune_log)
                fprintf(stderr, "[yh tune] %-36s %-40s %8.2f us\n", ops[i].label.c_str(), mx_name(pl).c_str(),
                        ms * 1e3f / 3);
            t_ms[c] = std::min(t_ms[c], ms);
        }
        // pick after every candidate is timed: the fastest, except that for 3x3 layers a plan
        // within 3 % of the fastest that re-reads fewer input bytes (halo and cout-slice
        // re-reads) wins - stable choices, less HBM pressure beside the other lanes
        const float best = *std::min_element(t_ms.begin(), t_ms.end());
        size_t pick = 0;
        for (size_t c = 0; c < cands[i].size(); ++c) {
            const MxPlan &pc = cands[i][c], &pp = cands[i][pick];
            const bool near = pc.cfg.ks == 3 && t_ms[c] <= best * 1.03f;
            const bool near_p = pp.cfg.ks == 3 && t_ms[pick] <= best * 1.03f;
            bool better;
            if (near && near_p) {
                const double rc_ = patch_reads(pc), rp = patch_reads(pp);
                better = rc_ < rp || (rc_ == rp && t_ms[c] < t_ms[pick]);
            } else {
                better = (near && !near_p) || (!near_p && t_ms[c] < t_ms[pick]);
            }
            if (better) pick = c;
        }
        slot[i].plan = cands[i][pick];
        slot[i].name = mx_name(cands[i][pick]);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}

// ---------------------------------------------------------- the other per-layer ops
FirstConvArgs Net::first_args(const Op& op, int B, int H, int W) const {
    const ConvDesc& d = convs[op.conv];
    FirstConvArgs a{};
    a.io = (const void* const*)io_dev; a.in_u8 = in_u8;
    a.H = H; a.W = W; a.Ho = H >> 1; a.Wo = W >> 1; a.Cout = d.cout_p; a.M = B * a.Ho * a.Wo;
    a.w = (const float*)d.w_dev; a.bias = d.b_dev;
    a.out = ptr(op.out); a.ldo = ldc(op.out); a.act = d.act;
    return a;
}
DwArgs Net::dw_args(const Op& op, int B, int H, int W) const {
    const ConvDesc& d = convs[op.conv];
    const Tensor& ti = tensors[op.in[0].v.t];
    DwArgs a{};
    a.in = ptr(op.in[0].v); a.ldi = ti.C;
    a.H = H >> ti.level; a.W = W >> ti.level; a.C = d.cout_p; a.M = B * a.H * a.W;
    a.w = (const float*)d.w_dev; a.bias = d.b_dev;
    a.out = ptr(op.out); a.ldo = ldc(op.out); a.act = d.act;
    return a;
}
PoolArgs Net::pool_args(const Op& op, int B, int H, int W) const {
    const Tensor& t = tensors[op.out.t];
    PoolArgs a{};
    a.buf = ptr(op.out); a.ldc = t.C; a.C = op.out.C; a.H = H >> t.level; a.W = W >> t.level; a.B = B;
    return a;
}
AttnArgs Net::attn_args(const Op& op, int H, int W) const {
    const ConvDesc& d = convs[op.conv];
    const Tensor& tq = tensors[op.in[0].v.t];
    AttnArgs a{};
    a.qkv = ptr(op.in[0].v); a.ldq = tq.C;
    a.Hs = H >> tq.level; a.Ws = W >> tq.level; a.T = a.Hs * a.Ws;
    a.heads = op.heads; a.dk = 32; a.dh = 64;
    a.scale = (float)std::pow(32.0, -0.5);
    a.pe_w = (const float*)d.w_dev; a.pe_b = d.b_dev;
    a.out = ptr(op.out); a.ldo = ldc(op.out);
    return a;
}
DecodeArgs Net::decode_args(const Op& op, int B, int H, int W) const {
    DecodeArgs a{};
    for (int l = 0; l < 3; ++l) {
        const Tensor& t = tensors[op.lvl[l].t];
        a.lvl[l] = ptr(op.lvl[l]);
        a.H[l] = H >> t.level; a.W[l] = W >> t.level;
        a.stride[l] = (float)(1 << t.level);
        a.ldc = t.C;
    }
    a.nc = var.num_classes; a.B = B;
    a.A = a.H[0] * a.W[0] + a.H[1] * a.W[1] + a.H[2] * a.W[2];
    a.io = (const void* const*)io_dev;
    a.a_lo = anchor_off(op.dlo, H, W); a.box = op.dbox ? 1 : 0;
    return a;
}

// ---------------------------------------------------------- fused ops
Stem2Args Net::stem2_args(const Op& op, int B, int H, int W) {
    const ConvDesc& d = convs[op.conv];
    Stem2Args a{};
    a.io = (const void* const*)io_dev;
    a.H = H; a.W = W; a.Hs = H >> 1; a.Ws = W >> 1; a.Ho = H >> 2; a.Wo = W >> 2; a.B = B;
    a.b1 = d.b_dev;
    a.c1 = d.cout; a.c2 = convs[op.cs[0]].cout;
    a.prm = stem2_params(op, a.prm_bias, a.prm_stem);
    a.out = ptr(op.out);
    a.ldo = ldc(op.out);
    a.in_u8 = in_u8;
    stem2_tiles(a.Ho, a.Wo, a.ntw, a.nth);
    return a;
}

PwChainArgs Net::pw_chain_args(const Op& op, int B, int H, int W) {
    PwChainArgs a{};
    const int lv = tensors[op.out.t].level;
    a.M = (long long)B * (H >> lv) * (W >> lv);
    a.P = op.pwP;
    a.nst = (int)op.pws.size();
    a.nload = (int)op.pwl.size();
    // pwc_warm off: no L2 warm-up in the prologue
    a.sink = opt.tune.pwc_warm ? op.pwLds - 1024 : -1;
    a.zero = zero_dev;
    for (int z = 0; z < a.nload; ++z) {
        PwcLoad& L = a.ld[z];
        L.g = ptr(op.pwl[z]);
        L.ldg = ldc(op.pwl[z]);
        L.lds = op.pwl_lds[z];
        L.nchunk = op.pwl[z].C / 8;
    }
    for (int k = 0; k < a.nst; ++k) {
        const Op& o = ops[op.alts[k]];
        const ConvDesc& d = convs[o.conv];
        const Op::PwStage& ps = op.pws[k];
        PwcStage& st = a.st[k];
        st.K = d.K;
        st.N = d.cout;
        st.act = d.act;
        st.nrun = (int)ps.runs.size();
        for (int r = 0; r < st.nrun; ++r) {
            const Op::PwRun& pr = ps.runs[r];
            PwcRun& R = st.run[r];
            R.nkb = pr.nch / 16;
            if (pr.stage >= 0) {
                R.lds = op.pws[pr.stage].lds + pr.coff * 2;
                R.ld = convs[ops[op.alts[pr.stage]].conv].cout + 8;
            } else {
                R.lds = op.pwl_lds[pr.load];
                R.ld = op.pwl[pr.load].C + 8;
            }
        }
        // A-fragment-ordered copy (upload: "pwfrag"); wld = Kp gives its k-blocks per A tile
        auto itw = d.mx_w.find("pwfrag");
        require(itw != d.mx_w.end(), "pw_chain: no fragment-ordered weights for " + d.name);
        st.w = itw->second;
        st.wld = d.Kp;
        st.bias = d.b_dev;
        st.res_lds = -1;
        if (o.has_res) {
            if (ps.res_stage >= 0) {
                st.res_lds = op.pws[ps.res_stage].lds + ps.res_coff * 2;
                st.res_ldl = convs[ops[op.alts[ps.res_stage]].conv].cout + 8;
            } else {
                st.res_lds = op.pwl_lds[ps.res_load];
                st.res_ldl = op.pwl[ps.res_load].C + 8;
            }
        }
        st.out = ptr(o.out);
        st.ldo = ldc(o.out);
        st.out_lds = ps.keep ? ps.lds : -1;
        st.out_ldl = d.cout + 8;
    }
    return a;
}

// output tile of one level of the fused cls branch: the largest candidate whose
// workgroup (resident weights + one tile's buffers) fits the LDS
bool Net::head_cls_tile(int C0, int c3, int nc, int H, int W, int& TH, int& TW) {
    static const int cand[][2] = {{16, 16}, {8, 32}, {8, 16}, {8, 8}, {4, 16}, {4, 8}, {8, 4}, {4, 4}, {2, 8}, {2, 4}, {2, 2}};
    for (auto& c : cand) {
        if (c[0] > H || c[1] > W) continue;
        if (head_cls_lds(c[0], c[1], C0, c3, nc) > 0) {
            TH = c[0];
            TW = c[1];
            return true;
        }
    }
    return false;
}
HeadClsArgs Net::head_cls_args(const Op& op, int B, int H, int W) {
    HeadClsArgs a{};
    a.B = B;
    a.nc = var.num_classes;
    int l0 = 0;
    while (!op.hlv[l0]) ++l0;
    a.c3 = convs[op.hc[l0][1]].cout;
    // workgroup order: levels 0, 1, 2 (issuing the 20x20 level first was 1.5-3 us slower,
    // profiles/r03_ops_hcls_order.txt)
    int lvls[3], nl = 0;
    for (int l = 0; l < 3; ++l)
        if (op.hlv[l]) lvls[nl++] = l;
    for (int k = 0; k < nl; ++k) {
        const int l = lvls[k];
        HeadClsLevel& v = a.lv[a.nlv++];
        const Tensor& t = tensors[op.hx[l].t];
        v.H = H >> t.level;
        v.W = W >> t.level;
        v.x = ptr(op.hx[l]);
        v.ldx = ldc(op.hx[l]);
        v.C0 = op.hx[l].C;
        v.y = ptr(op.hy[l]);
        v.ldy = ldc(op.hy[l]);
        v.aoff = anchor_off(l, H, W);
        const ConvDesc &d1 = convs[op.hc[l][0]], &p1 = convs[op.hc[l][1]], &d2 = convs[op.hc[l][2]],
                       &p2 = convs[op.hc[l][3]], &p3 = convs[op.hc[l][4]];
        require(d1.loaded && p1.loaded && d2.loaded && p2.loaded && p3.loaded, "head.cls weights not loaded");
        v.dw1w = (const float*)d1.w_dev; v.dw1b = d1.b_dev; v.dw1ld = d1.cout_p;
        v.pw1w = p1.w_dev; v.pw1ld = p1.Kp; v.pw1b = p1.b_dev;
        v.dw2w = (const float*)d2.w_dev; v.dw2b = d2.b_dev; v.dw2ld = d2.cout_p;
        v.pw2w = p2.w_dev; v.pw2ld = p2.Kp; v.pw2b = p2.b_dev;
        v.pw3w = p3.w_dev; v.pw3ld = p3.Kp; v.pw3b = p3.b_dev;
        require(head_cls_tile(v.C0, a.c3, a.nc, v.H, v.W, v.TH, v.TW), "head.cls: no LDS tile");
        v.ntw = (v.W + v.TW - 1) / v.TW;
        v.tiles = v.ntw * ((v.H + v.TH - 1) / v.TH);
    }
    a.zero = zero_dev;
    if (op.direct) {
        a.io = (const void* const*)io_dev;
        a.A = anchor_off(3, H, W);
    }
    // one workgroup per tile, levels in lvls order
    int wg = 0;
    for (int k = 0; k < nl; ++k) {
        a.lv[k].wg0 = wg;
        wg += B * a.lv[k].tiles;
    }
    return a;
}

BoxDflArgs Net::box_dfl_args(const Op& op, int B, int H, int W) {
    BoxDflArgs a{};
    a.B = B;
    a.nc = var.num_classes;
    a.A = anchor_off(3, H, W);
    a.io = (const void* const*)io_dev;
    a.nk = op.bx[0].C / 16;
    a.tpw = opt.tune.boxdfl_tpw ? opt.tune.boxdfl_tpw : BOX_DFL_TPW;
    int wg = 0;
    for (int l = 0; l < 3; ++l) {
        BoxDflLevel& v = a.lv[a.nlv++];
        const ConvDesc& d = convs[op.bc[l]];
        require(d.loaded, "head.box weights not loaded");
        require(d.cin == 16 * a.nk && d.cout == 64 && d.cout_p >= 64, "box_dfl: conv shape");
        const int lv = tensors[op.bx[l].t].level;
        v.x = ptr(op.bx[l]);
        v.ldx = ldc(op.bx[l]);
        v.H = H >> lv;
        v.W = W >> lv;
        v.stride = (float)(1 << lv);
        v.aoff = anchor_off(l, H, W);
        v.w = d.w_dev;
        v.wld = d.Kp;
        v.b = d.b_dev;
        v.wg0 = wg;
        const long long tiles = ((long long)B * v.H * v.W + 31) / 32;
        wg += (int)((tiles + 4 * a.tpw - 1) / (4 * a.tpw));
    }
    return a;
}

// Work items of one tile over P1-P4 (c3k2.hip cs_phase: one 32-cout A tile x one 32-pixel
// B tile each); P1 and P2 run on the tile with its 2- / 1-pixel halo.
static int csp_items(int TH, int TW, int ni, int nc, int no) {
    const auto nb = [](int px) { return (px + 31) / 32; };
    return (ni ? nc * nb((TH + 4) * (TW + 4)) : 0) + nb((TH + 2) * (TW + 2)) + ((nc + 1) / 2 + no) * nb(TH * TW);
}
// Output tile of a fused C3k2 launch over B maps of H x W on `cus` persistent workgroups.
bool Net::csp_tile(const Tuning& tune, int ni, int nc, int no, int B, int H, int W, int cus, int& TH, int& TW) {
    // Tuning::csp_th x csp_tw (YH_CSP_TILE; experiments, tests): that tile first where it fits one
    // workgroup (a tile larger than the map is clipped like any edge tile). csp_lds admits a tile
    // only if every multiply-shift quotient of the kernel's index math is exact for it, here and
    // for the default choice below.
    if (tune.csp_th > 0 && tune.csp_tw > 0 && csp_lds(tune.csp_th, tune.csp_tw, ni, nc, no) > 0) {
        TH = tune.csp_th;
        TW = tune.csp_tw;
        return true;
    }
    if (CSP_THREADS >= 1024) {
        // 16-wave workgroups, one per CU: the tile that minimises rounds x cycles per tile.
        // A tile costs CSP_TILE_FIXED cycles (the four phases' single-item latencies, paid
        // whatever the size) + CSP_TILE_ITEM per work item (LDS fragment reads and the
        // epilogues' issue slots); both fitted to the per-tile stamps of 16x20, 8x32, 8x16
        // and 4x16 tiles in profiles/cspidx_phase_stamps.txt (5.5-6.9 k and 150-160 for the
        // whole-block launches; the tail launch, whose input DMA is not overlapped, is
        // nearer 5.5 k + 270 and gets the same tile either way).
        constexpr long long CSP_TILE_FIXED = 6000, CSP_TILE_ITEM = 165;
        long long best = -1;
        H = std::min(H, 1 << 12);   // callers that only ask whether a tile exists pass huge maps
        W = std::min(W, 1 << 12);
        for (int th : {2, 4, 8, 10, 12, 16}) {
            if (th > H || (th == 2 && H >= 4)) continue;
            for (int tw = 4; tw <= W; tw += 4) {
                if (csp_lds(th, tw, ni, nc, no) <= 0) break;   // grows with tw
                const long long nt = (long long)B * ((H + th - 1) / th) * ((W + tw - 1) / tw);
                const long long cost = ((nt + cus - 1) / cus) * (CSP_TILE_FIXED + CSP_TILE_ITEM * csp_items(th, tw, ni, nc, no));
                if (best < 0 || cost < best) {
                    best = cost;
                    TH = th;
                    TW = tw;
                }
                if (nt <= cus) break;   // one round already: a wider tile only idles workgroups
            }
        }
        return best >= 0;
    }
    // 8-wave workgroups: the largest tile of >= 64 pixels that leaves room for a second
    // workgroup per CU, else the largest that fits (measured: net.p3.1 at 2x4 tiles, two per
    // CU, 263 us against 68 us at 8x16, one per CU)
    static const int cand[][2] = {{8, 16}, {8, 8}, {4, 16}, {4, 8}, {2, 8}, {2, 4}};
    for (int lim : {80 * 1024, 160 * 1024})
        for (auto& c : cand) {
            if (c[0] > H || c[1] > W || (lim == 80 * 1024 && c[0] * c[1] < 64)) continue;
            const int b = csp_lds(c[0], c[1], ni, nc, no);
            if (b > 0 && b <= lim) {
                TH = c[0];
                TW = c[1];
                return true;
            }
        }
    return false;
}

// block input, block output, map size and batch of a whole-block op (CspArgs, C3kArgs)
template <class Args>
static void block_io(const Net& n, const Op& op, int B, int H, int W, Args& a) {
    const View& xv = op.in[0].v;
    const int lv = n.tensors[xv.t].level;
    a.x = n.ptr(xv); a.ldx = n.ldc(xv);
    a.y = n.ptr(op.out); a.ldy = n.ldc(op.out);
    a.H = H >> lv; a.W = W >> lv; a.B = B;
}
// grid: persistent workgroups, as many as are resident at once
CspArgs Net::csp_args(size_t oi, int B, int H, int W, int& grid) {
    const Op& op = ops[oi];
    CspArgs a{};
    block_io(*this, op, B, H, W, a);
    a.prm = csp_params(op);
    a.ni = op.cs[0] >= 0 ? convs[op.cs[0]].cin / 16 : 0;
    a.nc = convs[op.cs[1]].cin / 16;
    a.no = convs[op.cs[3]].cout / 32;
    require(csp_tile(opt.tune, a.ni, a.nc, a.no, B, a.H, a.W, num_cus, a.TH, a.TW), op.label + ": no LDS tile");
    csp_plan[{GraphKey{B, H, W}, (int)oi}] = "c3k2_t" + std::to_string(a.TH) + "x" + std::to_string(a.TW);
    a.ntw = (a.W + a.TW - 1) / a.TW;
    // the kernel's per-lane offsets are 32-bit from the tile's origin pixel: a bound on the
    // map's width only (about 2^20 pixels at these channel counts), not on its size
    require(csp_span_ok(a.TH, a.TW, a.W, a.ldx, a.ldy), op.label + ": map too wide for 32-bit tile offsets");
    a.nth = (a.H + a.TH - 1) / a.TH;
    a.tiles = a.ntw * a.nth;
    a.ntiles = B * a.tiles;
    a.zero = zero_dev;
    // two workgroups per CU when the LDS allows (measured: net.p2.1 138 -> 103 us at b32)
    const int lds = csp_lds(a.TH, a.TW, a.ni, a.nc, a.no);
    const int per_cu = CSP_THREADS < 1024 && lds > 0 && lds <= 80 * 1024 ? 2 : 1;
    grid = std::min(a.ntiles, per_cu * num_cus);
    return a;
}
C3kArgs Net::c3k_args(const Op& op, int B, int H, int W) {
    C3kArgs a{};
    block_io(*this, op, B, H, W, a);
    a.prm = c3k_params(op);
    a.hh = convs[op.ck[0]].cout;
    return a;
}

// ---------------------------------------------------------- classifier head
ClsPoolArgs Net::cls_pool_args(const Op& op, int B, int H, int W) const {
    ClsPoolArgs a{};
    const View& v = op.in[0].v;
    a.a = ptr(v); a.lda = ldc(v);
    a.B = B; a.HW = (H >> 5) * (W >> 5); a.C = op.out.C;
    a.inv = (float)(1.0 / a.HW);
    a.e = (float*)ptr(op.out);
    return a;
}
ClsHeadArgs Net::cls_head_args(const Op& op, int B, int H, int W) const {
    const ConvDesc& d = convs[op.conv];
    ClsHeadArgs a{};
    const View& v = op.in[0].v;
    a.x = ptr(v); a.ldx = ldc(v);
    a.B = B; a.HW = (H >> 5) * (W >> 5); a.K = d.K; a.N = d.cout;
    a.G = cls_head_group(a.K, a.HW);
    require(a.G > 0 && v.C == d.K && d.Kp == d.K, op.label + ": no cls_head plan at this shape");
    auto itw = d.mx_w.find("pwfrag");
    require(itw != d.mx_w.end(), "cls_head: no fragment-ordered weights for " + d.name);
    a.w = itw->second; a.wld = d.Kp;
    a.bias = d.b_dev;
    a.act = d.act;
    a.inv = (float)(1.0 / a.HW);
    a.e = (float*)ptr(op.out);
    return a;
}
ClsFcArgs Net::cls_fc_args(const Op& op, int B) const {
    const ConvDesc& d = convs[op.conv];
    ClsFcArgs a{};
    a.e = (const float*)ptr(op.in[0].v);
    a.w = d.w_dev; a.wld = d.Kp;
    a.bias = d.b_dev;
    a.B = B; a.nc = d.cout; a.K = d.cin;
    a.z = (float*)ptr(op.out); a.ldz = ldc(op.out);
    a.io = (const void* const*)io_dev;
    return a;
}

void Net::launch_op(size_t oi, int B, int H, int W, hipStream_t s) {
    const Op& op = ops[oi];
    int rc = 0;
    switch (op.kind) {
        case OP_FIRST: rc = launch_first_conv(dtype, first_args(op, B, H, W), B, s); break;
        case OP_CONV: {
            if (dtype != F32) {
                require(cur_kern != nullptr, "conv plans not chosen", YH_ESTATE);
                rc = launch_mx_op(op, (*cur_kern)[oi].plan, B, H, W, s);
                break;
            }
            ConvArgs a{};
            int BM, BN;
            conv_args(op, B, H, W, a, BM, BN);
            rc = launch_conv(dtype, BM, BN, a, s);
            break;
        }
        case OP_DW: rc = launch_dwconv(dtype, dw_args(op, B, H, W), s); break;
        case OP_SPPF: rc = launch_sppf(dtype, pool_args(op, B, H, W), ctx(), s); break;
        case OP_ATTN: rc = launch_attention(dtype, attn_args(op, H, W), B, ctx(), s); break;
        case OP_HEADCLS: rc = launch_head_cls(dtype, head_cls_args(op, B, H, W), s); break;
        case OP_DECODE: rc = launch_decode(dtype, decode_args(op, B, H, W), s); break;
        case OP_BOXDFL: rc = launch_box_dfl(dtype, box_dfl_args(op, B, H, W), s); break;
        case OP_PWCHAIN: rc = launch_pw_chain(dtype, pw_chain_args(op, B, H, W), op.pwLds, s); break;
        case OP_STEM2: rc = launch_stem2(dtype, stem2_args(op, B, H, W), s); break;
        case OP_CSP: {
            int grid = 0;
            const CspArgs a = csp_args(oi, B, H, W, grid);
            rc = launch_csp(dtype, a, grid, s);
            break;
        }
        case OP_C3K: rc = launch_c3k(dtype, c3k_args(op, B, H, W), ctx(), s); break;
        case OP_CLSPOOL: rc = launch_cls_pool(dtype, cls_pool_args(op, B, H, W), s); break;
        case OP_CLSHEAD: rc = launch_cls_head(dtype, cls_head_args(op, B, H, W), s); break;
        case OP_CLSFC: rc = launch_cls_fc(dtype, cls_fc_args(op, B), s); break;
    }
    if (rc != 0) throw Fail(YH_EHIP, "launch of " + op.label + " failed: " + hipGetErrorString((hipError_t)rc));
}

}  // namespace yh
