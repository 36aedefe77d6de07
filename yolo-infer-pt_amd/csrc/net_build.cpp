// Graph building and fusion passes: the layer graph of a variant (nets/nn.py:28-305) as ops over
// NHWC tensors, and which layers a 16-bit handle runs as fused ops.
#include <algorithm>

#include "net.h"

namespace yh {

int Net::tensor(int level, int C) {
    tensors.push_back({level, round_up(C, 8)});
    return (int)tensors.size() - 1;
}
View Net::slice(int t, int coff, int C) const {
    require(coff % 8 == 0 && C % 8 == 0, "concat slice not a multiple of 8 channels");
    return View{t, coff, C};
}
int Net::new_conv(const std::string& name, ConvKind kind, int cin, int cout, int k, int s, int g, int has_bias, int act) {
    ConvDesc d;
    d.name = name;
    d.kind = kind;
    d.cin = cin; d.cout = cout; d.k = k; d.stride = s; d.groups = g;
    d.has_bias = has_bias; d.act = act;
    convs.push_back(std::move(d));
    return (int)convs.size() - 1;
}
// a dense conv with a single unsegmented input and no op of its own (fused ops)
int Net::new_dense_conv(const std::string& name, int cin, int cout, int k, int has_bias, int act) {
    const int ci = new_conv(name, CK_DENSE, cin, cout, k, 1, 1, has_bias, act);
    convs[ci].segs.push_back({cin, round_up(cin, 8)});
    return ci;
}
// dense conv op (k in {1,3}), input segments given as (view, logical channels, upsample)
void Net::dense(const std::string& name, const std::vector<Seg>& in, const std::vector<int>& logical, int cout, int k,
                int s, int act, View out, const View* res, int has_bias) {
    int cin = 0;
    for (int c : logical) cin += c;
    const int ci = new_conv(name, CK_DENSE, cin, cout, k, s, 1, has_bias, act);
    ConvDesc& d = convs[ci];
    for (size_t i = 0; i < in.size(); ++i) d.segs.push_back({logical[i], in[i].v.C});
    require(in.size() <= 2, "at most two concat segments");
    if (in.size() == 2) require(logical[0] == in[0].v.C && logical[0] % 8 == 0, "segment 0 must be 8-aligned");
    Op op;
    op.kind = OP_CONV;
    op.conv = ci;
    op.in = in;
    op.out = out;
    if (res) { op.res = *res; op.has_res = true; }
    op.label = name;
    ops.push_back(op);
}
View Net::conv1(const std::string& name, View x, int xc, int cout, int act, View out, const View* res) {
    dense(name, {Seg{x, 0}}, {xc}, cout, 1, 1, act, out, res);
    return out;
}
View Net::conv3(const std::string& name, View x, int xc, int cout, int s, int act, View out, const View* res) {
    dense(name, {Seg{x, 0}}, {xc}, cout, 3, s, act, out, res);
    return out;
}
void Net::dw(const std::string& name, View x, int ch, View out) {
    Op op;
    op.kind = OP_DW;
    op.conv = new_conv(name, CK_DW, ch, ch, 3, 1, ch, 0, ACT_SILU);
    op.in = {Seg{x, 0}};
    op.out = out;
    op.label = name;
    ops.push_back(op);
}

// Residual (nn.py:42-49): out = x + conv2(conv1(x)), both 3x3 SiLU
void Net::residual(const std::string& p, View x, int ch, double e, View out, int level) {
    const int hid = (int)(ch * e);
    const int t = tensor(level, hid);
    conv3(p + ".conv1", x, ch, hid, 1, ACT_SILU, full(t));
    conv3(p + ".conv2", full(t), hid, ch, 1, ACT_SILU, out, &x);
}
// CSPModule / C3k (nn.py:52-63)
// The residual chain a -> a' -> a'' runs through fresh tensors (not in place) so that no region
// is rewritten after a 3x3 conv of another workgroup read it; the last link writes into the
// concat buffer.
void Net::cspmodule(const std::string& p, View x, int in_ch, int out_ch, View out, int level) {
    const int h = out_ch / 2;
    const int t = tensor(level, 2 * h);
    View a = slice(t, 0, h), b = slice(t, h, h);
    const int a0 = tensor(level, h), a1 = tensor(level, h);
    const int first = (int)ops.size();
    conv1(p + ".conv1", x, in_ch, h, ACT_SILU, full(a0));
    conv1(p + ".conv2", x, in_ch, h, ACT_SILU, b);
    residual(p + ".res_m.0", full(a0), h, 1.0, full(a1), level);
    residual(p + ".res_m.1", full(a1), h, 1.0, a, level);
    conv1(p + ".conv3", full(t), 2 * h, out_ch, ACT_SILU, out);
    // 16-bit handles: the whole block as one launch (c3k.hip) at shapes whose image fits
    // a workgroup's LDS (ensure_plan picks it or the seven launches above per shape)
    // c3k.hip moves 8 channels per 16-byte access at ptr(view) + 8 h: both views must start
    // on an 8-channel boundary (slice() enforces it today; checked here so the op never
    // depends on that)
    if (dtype != F32 && opt.fuse && opt.c3k && (in_ch == 64 || in_ch == 128) && out_ch == in_ch && x.C == in_ch &&
        x.coff % 8 == 0 && out.coff % 8 == 0) {
        Op op;
        op.kind = OP_C3K;
        op.label = p;
        for (int k = 0; k < 7; ++k) {
            op.ck[k] = ops[first + k].conv;
            op.alts.push_back(first + k);
        }
        op.in = {Seg{x, 0}};
        op.out = out;
        ops.push_back(op);
    }
}
// CSP / C3k2 (nn.py:66-80); input may be a 2-segment (optionally upsampled) concat
void Net::csp(const std::string& p, const std::vector<Seg>& in, const std::vector<int>& logical, int out_ch, int n,
              bool use_c3k, int r, View out, int level) {
    const int c = out_ch / r;
    // tail mode even where the whole block fits one launch: Options::csp_tail (tests)
    const bool tail = n == 1 && !use_c3k && fuse_csp_tail(c, out_ch, out) &&
                      (opt.csp_tail || !fuse_csp(in, logical, c, out_ch, out));
    if (tail || (n == 1 && !use_c3k && fuse_csp(in, logical, c, out_ch, out))) {
        // one launch for the whole block (c3k2.hip); the same four convs, loaded by name. Tail
        // mode: conv1 as its own launch into a compact [a | b] tensor, then Residual + conv2 as
        // one launch
        Op op;
        op.kind = OP_CSP;
        op.label = tail ? p + ".tail" : p;
        op.in = in;
        if (tail) {
            const int t1 = tensor(level, 2 * c);
            dense(p + ".conv1", in, logical, 2 * c, 1, 1, ACT_SILU, full(t1));
            op.in = {Seg{full(t1, 2 * c), 0}};
        } else {
            op.cs[0] = new_dense_conv(p + ".conv1", logical[0], 2 * c, 1, 0, ACT_SILU);
        }
        op.cs[1] = new_dense_conv(p + ".res_m.0.conv1", c, c / 2, 3, 0, ACT_SILU);
        op.cs[2] = new_dense_conv(p + ".res_m.0.conv2", c / 2, c, 3, 0, ACT_SILU);
        op.cs[3] = new_dense_conv(p + ".conv2", 3 * c, out_ch, 1, 0, ACT_SILU);
        op.out = out;
        ops.push_back(op);
        return;
    }
    const int t = tensor(level, (2 + n) * c);
    dense(p + ".conv1", in, logical, 2 * c, 1, 1, ACT_SILU, slice(t, 0, 2 * c));
    for (int i = 0; i < n; ++i) {
        View src = slice(t, (1 + i) * c, c), dst = slice(t, (2 + i) * c, c);
        const std::string q = p + ".res_m." + std::to_string(i);
        if (!use_c3k) residual(q, src, c, 0.5, dst, level);
        else cspmodule(q, src, c, c, dst, level);
    }
    conv1(p + ".conv2", full(t), (2 + n) * c, out_ch, ACT_SILU, out);
}
// SPP / SPPF (nn.py:83-94)
void Net::sppf(const std::string& p, View x, int in_ch, int out_ch, View out, int level) {
    const int h = in_ch / 2;
    const int t = tensor(level, 4 * h);
    conv1(p + ".conv1", x, in_ch, h, ACT_SILU, slice(t, 0, h));
    Op op;
    op.kind = OP_SPPF;
    op.out = slice(t, 0, h);
    op.label = p + ".res_m";
    ops.push_back(op);
    conv1(p + ".conv2", full(t), 4 * h, out_ch, ACT_SILU, out);
}
// PSABlock (nn.py:126-136), in place on view x
void Net::psablock(const std::string& p, View x, int ch, int heads, int level) {
    const int dh = ch / heads, dk = dh / 2;
    require(dh == 64 && dk == 32, "PSA head dims must be dh=64, dk=32");
    const int qc = ch + 2 * dk * heads;
    const int tq = tensor(level, qc);
    conv1(p + ".conv1.qkv", x, ch, qc, ACT_ID, full(tq));
    const int ta = tensor(level, ch);
    Op op;
    op.kind = OP_ATTN;
    op.conv = new_conv(p + ".conv1.conv1", CK_PE, ch, ch, 3, 1, ch, 0, ACT_ID);
    op.in = {Seg{full(tq), 0}};
    op.out = full(ta);
    op.heads = heads;
    op.label = p + ".conv1";
    ops.push_back(op);
    conv1(p + ".conv1.conv2", full(ta), ch, ch, ACT_ID, x, &x);
    const int tf = tensor(level, 2 * ch);
    conv1(p + ".conv2.0", x, ch, 2 * ch, ACT_SILU, full(tf));
    conv1(p + ".conv2.1", full(tf), 2 * ch, ch, ACT_ID, x, &x);
}
// PSA / C2PSA (nn.py:139-148)
void Net::psa(const std::string& p, View x, int ch, int n, View out, int level) {
    const int half = ch / 2;
    const int t = tensor(level, 2 * half);
    conv1(p + ".conv1", x, ch, 2 * half, ACT_SILU, full(t));
    for (int i = 0; i < n; ++i) psablock(p + ".res_m." + std::to_string(i), slice(t, half, half), half, ch / 128, level);
    conv1(p + ".conv2", full(t), 2 * half, ch, ACT_SILU, out);
}

// DarkNet (nn.py:151-189) up to net.p5.1, which both tasks share; returns that block's output
// tensor, and the p3 / p4 outputs the detector's FPN reads.
int Net::build_backbone(int& b3, int& b4) {
    const int* w = var.width;
    const int* d = var.depth;
    const bool c0 = var.csp[0] != 0, c1 = var.csp[1] != 0;
    const int t2 = tensor(2, w[2]);
    if (fuse_stem(w[0], w[1], w[2])) {
        // stem + net.p2.0 in one launch: the stem output never reaches HBM
        Op op;
        op.kind = OP_STEM2;
        op.conv = new_conv("net.p1.0", CK_FIRST, w[0], w[1], 3, 2, 1, 0, ACT_SILU);
        op.cs[0] = new_dense_conv("net.p2.0", w[1], w[2], 3, 0, ACT_SILU);
        convs[op.cs[0]].stride = 2;
        op.out = full(t2, w[2]);
        op.label = "net.p1.0+p2.0";
        ops.push_back(op);
    } else {
        const int t1 = tensor(1, w[1]);
        Op op;
        op.kind = OP_FIRST;
        op.conv = new_conv("net.p1.0", CK_FIRST, w[0], w[1], 3, 2, 1, 0, ACT_SILU);
        op.out = full(t1, w[1]);
        op.label = "net.p1.0";
        ops.push_back(op);
        conv3("net.p2.0", full(t1, w[1]), w[1], w[2], 2, ACT_SILU, full(t2, w[2]));
    }
    const int t2b = tensor(2, w[3]);
    csp("net.p2.1", {Seg{full(t2, w[2]), 0}}, {w[2]}, w[3], d[0], c0, 4, full(t2b, w[3]), 2);
    const int t3 = tensor(3, w[3]);
    conv3("net.p3.0", full(t2b, w[3]), w[3], w[3], 2, ACT_SILU, full(t3, w[3]));
    b3 = tensor(3, w[4]);
    csp("net.p3.1", {Seg{full(t3, w[3]), 0}}, {w[3]}, w[4], d[1], c0, 4, full(b3, w[4]), 3);
    const int t4 = tensor(4, w[4]);
    conv3("net.p4.0", full(b3, w[4]), w[4], w[4], 2, ACT_SILU, full(t4, w[4]));
    b4 = tensor(4, w[4]);
    csp("net.p4.1", {Seg{full(t4, w[4]), 0}}, {w[4]}, w[4], d[2], c1, 2, full(b4, w[4]), 4);
    const int t5 = tensor(5, w[5]);
    conv3("net.p5.0", full(b4, w[4]), w[4], w[5], 2, ACT_SILU, full(t5, w[5]));
    const int t5b = tensor(5, w[5]);
    csp("net.p5.1", {Seg{full(t5, w[5]), 0}}, {w[5]}, w[5], d[3], c1, 2, full(t5b, w[5]), 5);
    return t5b;
}

// The classifier (nn.py YOLOCls): the backbone without the SPPF, C2PSA as net.p5.2, then the
// Classify head: head.conv (1x1 to CLS_EMBED, SiLU), the mean over pixels, head.linear (described
// as a 1x1 conv with bias, so weights load by name like every other layer) and the softmax.
void Net::build_cls() {
    const int* w = var.width;
    const int nc = var.num_classes;
    int b3, b4;
    const int t5b = build_backbone(b3, b4);
    const int t5c = tensor(5, w[5]);
    psa("net.p5.2", full(t5b, w[5]), w[5], var.depth[4], full(t5c, w[5]), 5);
    // per-layer path: the dense 1x1 conv writes a, cls_pool reduces it
    const int ta = tensor(5, CLS_EMBED), te = tensor(-1, CLS_EMBED), tz = tensor(-1, nc);
    const int conv_op = (int)ops.size();
    // fp32 handle: this layer's output is held to one fp32 ulp of the fp64 conv (the parity tests),
    // which SiLU in fp32 after the rounded K sum misses; its epilogue runs in fp64 (conv.hip)
    conv1("head.conv", full(t5c, w[5]), w[5], CLS_EMBED, dtype == F32 ? ACT_SILU_F64 : ACT_SILU, full(ta, CLS_EMBED));
    const int pool_op = (int)ops.size();
    Op pool;
    pool.kind = OP_CLSPOOL;
    pool.label = "head.pool";
    pool.in = {Seg{full(ta, CLS_EMBED), 0}};
    pool.out = full(te);
    ops.push_back(pool);
    // 16-bit handles with YH_CLSHEAD=1: conv + pool as one launch (cls.hip cls_head) at shapes where
    // an image's map fits a workgroup (Net::fused_fits); the default keeps the two launches, which
    // measured faster
    if (dtype != F32 && opt.fuse && opt.cls_head && cls_head_pmax(w[5]) > 0 && tensors[t5c].C == w[5]) {
        Op hd;
        hd.kind = OP_CLSHEAD;
        hd.label = "head.conv+pool";
        hd.conv = ops[conv_op].conv;
        hd.in = {Seg{full(t5c, w[5]), 0}};
        hd.out = full(te);
        hd.alts = {conv_op, pool_op};
        ops.push_back(hd);
    }
    Op fc;
    fc.kind = OP_CLSFC;
    fc.label = "head.linear";
    fc.conv = new_dense_conv("head.linear", CLS_EMBED, nc, 1, 1, ACT_ID);
    fc.in = {Seg{full(te), 0}};
    fc.out = full(tz);
    ops.push_back(fc);
    finalize_convs();
    fuse_pw_chains();
}

void Net::build() {
    if (task == 1) { build_cls(); return; }
    const int* w = var.width;
    const int* d = var.depth;
    const bool c0 = var.csp[0] != 0, c1 = var.csp[1] != 0;
    const int nc = var.num_classes;
    int b3, b4;
    const int t5b = build_backbone(b3, b4);
    const int t5c = tensor(5, w[5]);
    sppf("net.p5.2", full(t5b, w[5]), w[5], w[5], full(t5c, w[5]), 5);
    // R = [h5(p4) | p5] (h6 input); backbone p5 is written into its slice 1
    const int R = tensor(5, w[4] + w[5]);
    View p5 = slice(R, w[4], w[5]);
    psa("net.p5.3", full(t5c, w[5]), w[5], d[4], p5, 5);
    // ---- DarkFPN (nn.py:192-209)
    const int Q = tensor(4, w[3] + w[4]);   // [h3(p3) | h1 out]
    View h1o = slice(Q, w[3], w[4]);
    csp("fpn.h1", {Seg{p5, 1}, Seg{full(b4, w[4]), 0}}, {w[5], w[4]}, w[4], d[5], c0, 2, h1o, 4);
    const int P3 = tensor(3, w[3]);
    csp("fpn.h2", {Seg{h1o, 1}, Seg{full(b3, w[4]), 0}}, {w[4], w[4]}, w[3], d[5], c0, 2, full(P3, w[3]), 3);
    conv3("fpn.h3", full(P3, w[3]), w[3], w[3], 2, ACT_SILU, slice(Q, 0, w[3]));
    const int P4 = tensor(4, w[4]);
    csp("fpn.h4", {Seg{full(Q), 0}}, {w[3] + w[4]}, w[4], d[5], c0, 2, full(P4, w[4]), 4);
    conv3("fpn.h5", full(P4, w[4]), w[4], w[4], 2, ACT_SILU, slice(R, 0, w[4]));
    const int P5 = tensor(5, w[5]);
    csp("fpn.h6", {Seg{full(R), 0}}, {w[4] + w[5]}, w[5], d[5], c1, 2, full(P5, w[5]), 5);
    // ---- Head (nn.py:228-270)
    const int boxc = std::max(64, w[3] / 4);
    const int clsc = std::max(std::max(80, w[3]), nc);
    const int ncp = round_up(nc, 8);
    const int xs[3] = {P3, P4, P5};
    const int xc[3] = {w[3], w[4], w[5]};
    int L[3];
    for (int l = 0; l < 3; ++l) L[l] = tensor(3 + l, 64 + ncp);
    // 16-bit handles run the cls branches of the levels that have an LDS tile as one
    // fused launch (head.hip), and fold the decode into the producers of the logits: the
    // box rows into box_dfl (last box conv + DFL), the fused levels' scores into
    // head_cls, the other levels' (a suffix) into a class-rows decode. YH_FUSE=0 keeps
    // the per-layer launches and the decode.
    bool fl[3];
    for (int l = 0; l < 3; ++l) fl[l] = fuse_head_cls(xc[l], clsc, nc);
    const bool fdec = fuse_decode(boxc, nc) && (fl[0] || !fl[1]) && (fl[1] || !fl[2]);
    bool fuse_any = false;
    Op hcop;
    hcop.kind = OP_HEADCLS;
    hcop.label = "head.cls";
    hcop.direct = fdec;
    Op bdop;
    bdop.kind = OP_BOXDFL;
    bdop.label = "head.box_dfl";
    // per level, coarsest first (the 80x80 level's launches come last)
    for (int l : {2, 1, 0}) {
        const int lvl = 3 + l;
        const std::string bp = "head.box." + std::to_string(l);
        const int tb1 = tensor(lvl, boxc), tb2 = tensor(lvl, boxc);
        conv3(bp + ".0", full(xs[l], xc[l]), xc[l], boxc, 1, ACT_SILU, full(tb1, boxc));
        conv3(bp + ".1", full(tb1, boxc), boxc, boxc, 1, ACT_SILU, full(tb2, boxc));
        if (fdec) {
            bdop.bc[l] = new_dense_conv(bp + ".2", boxc, 64, 1, 1, ACT_ID);
            bdop.bx[l] = full(tb2, boxc);
        } else {
            dense(bp + ".2", {Seg{full(tb2, boxc), 0}}, {boxc}, 64, 1, 1, ACT_ID, slice(L[l], 0, 64), nullptr, 1);
        }
        const std::string cp = "head.cls." + std::to_string(l);
        const View o{L[l], 64, ncp};
        if (fl[l]) {
            // the same five convs (weights are loaded by name), no per-layer ops
            fuse_any = hcop.hlv[l] = true;
            hcop.hc[l][0] = new_conv(cp + ".0", CK_DW, xc[l], xc[l], 3, 1, xc[l], 0, ACT_SILU);
            hcop.hc[l][1] = new_dense_conv(cp + ".1", xc[l], clsc, 1, 0, ACT_SILU);
            hcop.hc[l][2] = new_conv(cp + ".2", CK_DW, clsc, clsc, 3, 1, clsc, 0, ACT_SILU);
            hcop.hc[l][3] = new_dense_conv(cp + ".3", clsc, clsc, 1, 0, ACT_SILU);
            hcop.hc[l][4] = new_dense_conv(cp + ".4", clsc, nc, 1, 1, ACT_ID);
            hcop.hx[l] = full(xs[l], xc[l]);
            hcop.hy[l] = o;
            continue;
        }
        const int tc1 = tensor(lvl, xc[l]), tc2 = tensor(lvl, clsc), tc3 = tensor(lvl, clsc), tc4 = tensor(lvl, clsc);
        dw(cp + ".0", full(xs[l], xc[l]), xc[l], full(tc1, xc[l]));
        conv1(cp + ".1", full(tc1, xc[l]), xc[l], clsc, ACT_SILU, full(tc2, clsc));
        dw(cp + ".2", full(tc2, clsc), clsc, full(tc3, clsc));
        conv1(cp + ".3", full(tc3, clsc), clsc, clsc, ACT_SILU, full(tc4, clsc));
        dense(cp + ".4", {Seg{full(tc4, clsc), 0}}, {clsc}, nc, 1, 1, ACT_ID, o, nullptr, 1);
    }
    if (fuse_any) ops.push_back(hcop);
    if (fdec) ops.push_back(bdop);
    Op dec;
    dec.kind = OP_DECODE;
    for (int l = 0; l < 3; ++l) dec.lvl[l] = full(L[l]);
    dec.label = "head.decode";
    dec.dbox = !fdec;
    dec.dlo = fdec ? (fl[2] ? 3 : fl[1] ? 2 : fl[0] ? 1 : 0) : 0;
    if (dec.dlo < 3) {
        if (fdec) dec.label = "head.decode_cls";
        ops.push_back(dec);
    }
    finalize_convs();
    fuse_pw_chains();
}

void Net::finalize_convs() {
    for (auto& d : convs) {
        d.cout_p = round_up(d.cout, 8);
        if (d.kind == CK_DENSE) {
            d.cin_p = 0;
            for (auto& s : d.segs) d.cin_p += s.second;
            d.K = d.k * d.k * d.cin_p;
            d.Kp = round_up(d.K, 64);
            d.coutp_pad = round_up(d.cout_p, 128);
        } else {
            d.cin_p = round_up(d.cin, 8);
            d.coutp_pad = d.cout_p;
        }
    }
}

// ---- pointwise chains (pwchain.hip): maximal runs of consecutive 1x1 conv ops on one
//      40x40-or-smaller map become one launch, inserted after the run's last op; the per-layer
//      ops stay (inactive) for YH_PWCHAIN=0 and the parity tests
void Net::fuse_pw_chains() {
    if (dtype == F32 || !opt.fuse || !opt.pw_chain) return;
    for (size_t i = 0; i < ops.size();) {
        std::vector<char> taken(ops.size(), 0);   // per-layer alternatives of another fused op
        for (auto& o : ops)
            if (o.kind != OP_PWCHAIN)
                for (int k : o.alts) taken[k] = 1;
        auto eligible = [&](size_t k) {
            const Op& o = ops[k];
            if (o.kind != OP_CONV || taken[k]) return false;
            const ConvDesc& d = convs[o.conv];
            if (d.k != 1 || d.stride != 1 || d.cout % 32 || d.K % 128 || d.K > 1024 || d.cout > 1024) return false;
            const int lv = tensors[o.out.t].level;
            if (lv < 4 || o.out.coff % 8) return false;
            for (size_t si = 0; si < o.in.size(); ++si) {
                const Seg& sg = o.in[si];
                if (sg.up || tensors[sg.v.t].level != lv || d.segs[si].first != d.segs[si].second) return false;
            }
            if (o.has_res && (tensors[o.res.t].level != lv || o.res.C < d.cout)) return false;
            return true;
        };
        if (!eligible(i)) { ++i; continue; }
        const int lv = tensors[ops[i].out.t].level;
        size_t j = i + 1;
        while (j < ops.size() && j - i < (size_t)PWC_MAX_STAGES && eligible(j) && tensors[ops[j].out.t].level == lv) ++j;
        size_t made = 0;
        for (size_t e = j; e >= i + 2 && !made; --e)
            if (make_pw_chain(i, e)) made = e + 1;   // the chain op sits at e
        i = made ? made : i + 1;
    }
}
// the chain ops [i, e) as one OP_PWCHAIN inserted at e; false (nothing changed) if the stages'
// sources do not split into whole 128-channel runs or the tile does not fit the LDS
bool Net::make_pw_chain(size_t i, size_t e) {
    const int n = (int)(e - i);
    Op ch;
    ch.kind = OP_PWCHAIN;
    ch.pws.resize(n);
    // the latest stage before k writing channel c of tensor t (-1: none)
    auto producer = [&](int k, int t, int c) {
        for (int q = k - 1; q >= 0; --q) {
            const View& o = ops[i + q].out;
            if (o.t == t && c >= o.coff && c < o.coff + convs[ops[i + q].conv].cout) return q;
        }
        return -1;
    };
    // a global view comes in by the prologue: one load per distinct view
    auto load_of = [&](const View& g) {
        for (size_t z = 0; z < ch.pwl.size(); ++z)
            if (ch.pwl[z].t == g.t && ch.pwl[z].coff == g.coff && ch.pwl[z].C == g.C) return (int)z;
        ch.pwl.push_back(g);
        return (int)ch.pwl.size() - 1;
    };
    for (int k = 0; k < n; ++k) {
        const Op& o = ops[i + k];
        Op::PwStage& st = ch.pws[k];
        for (const Seg& sg : o.in) {
            const View& v = sg.v;
            for (int c = v.coff; c < v.coff + v.C;) {
                const int q = producer(k, v.t, c);
                int c1 = c + 8;
                while (c1 < v.coff + v.C && producer(k, v.t, c1) == q) c1 += 8;
                Op::PwRun r;
                r.stage = q;
                r.nch = c1 - c;
                r.coff = q >= 0 ? c - ops[i + q].out.coff : c;
                if (r.nch % 128) return false;
                if (q < 0) r.load = load_of(View{v.t, c, r.nch});
                else ch.pws[q].keep = true;
                st.runs.push_back(r);
                c = c1;
            }
        }
        if ((int)st.runs.size() > PWC_MAX_RUNS) return false;
        if (o.has_res) {
            const int cout = convs[o.conv].cout;
            const int q = producer(k, o.res.t, o.res.coff);
            for (int c = o.res.coff; c < o.res.coff + cout; c += 8)
                if (producer(k, o.res.t, c) != q) return false;
            st.res_stage = q;
            if (q >= 0) {
                st.res_coff = o.res.coff - ops[i + q].out.coff;
                ch.pws[q].keep = true;
            } else {   // a global residual also comes in by the prologue (no VGPR load in the epilogue)
                st.res_load = load_of(View{o.res.t, o.res.coff, cout});
            }
        }
    }
    if ((int)ch.pwl.size() > PWC_MAX_LOADS) return false;
    // LDS: the kept stage outputs (pixel stride cout + 8), then the loads (stride C + 8,
    // whole 1 KB LDS-DMA instructions)
    auto layout = [&](int P) {
        int off = 0;
        for (int k = 0; k < n; ++k) {
            Op::PwStage& st = ch.pws[k];
            st.lds = -1;
            if (!st.keep) continue;
            st.lds = off;
            off += (P * (convs[ops[i + k].conv].cout + 8) * 2 + 15) & ~15;
        }
        ch.pwl_lds.assign(ch.pwl.size(), 0);
        for (size_t z = 0; z < ch.pwl.size(); ++z) {
            off = (off + 1023) & ~1023;
            ch.pwl_lds[z] = off;
            off += (P * (ch.pwl[z].C + 8) * 2 + 1023) & ~1023;
        }
        off = (off + 1023) & ~1023;
        return off + 1024;   // the weight warm-up DMAs' sink (pw_chain)
    };
    int P = 64, lds = layout(64);
    if (lds > 160 * 1024) {
        P = 32;
        lds = layout(32);
    }
    if (lds > 160 * 1024) return false;
    ch.pwP = P;
    ch.pwLds = lds;
    for (int k = 0; k < n; ++k) ch.alts.push_back((int)(i + k));
    ch.label = ops[i].label + " +" + std::to_string(n - 1);
    ch.out = ops[e - 1].out;
    // insert at e: op indices >= e move up by one
    for (auto& o : ops)
        for (int& k : o.alts)
            if (k >= (int)e) k++;
    ops.insert(ops.begin() + e, ch);
    return true;
}

// ---- which layers run fused: decided when the net is built, before any input size is known
// the stem and net.p2.0 run fused (conv.hip stem_fused) on 16-bit handles for the
// instantiated widths (v11_n 16 -> 32, v11_s 32 -> 64). The kernel addresses one image's three
// planes with 32-bit element offsets, so reserve() refuses an input with 3 * H * W >= 2^32
// elements (stem2_size_ok) on a handle that fuses the stem.
bool Net::fuse_stem(int c0, int c1, int c2) const {
    if (dtype == F32 || !opt.fuse) return false;
    return c0 == 3 && stem2_ok(c1, c2);
}
// a C3k2 block with one Residual runs fused (c3k2.hip) on 16-bit handles when its input
// is one plain view of 16-channel blocks and (Cin, c, cout) has an instantiated kernel
bool Net::fuse_csp(const std::vector<Seg>& in, const std::vector<int>& logical, int c, int out_ch, View out) const {
    if (dtype == F32 || !opt.fuse) return false;
    if (in.size() != 1 || in[0].up || in[0].v.C != logical[0] || logical[0] % 16 || c % 16 || out_ch % 32) return false;
    if (out.coff % 8 || in[0].v.coff % 8) return false;
    int TH, TW;
    return csp_tile(opt.tune, logical[0] / 16, c / 16, out_ch / 32, 1, 1 << 30, 1 << 30, 1, TH, TW);
}
bool Net::fuse_csp_tail(int c, int out_ch, View out) const {
    if (dtype == F32 || !opt.fuse) return false;
    if (c % 16 || out_ch % 32 || out.coff % 8) return false;
    int TH, TW;
    return csp_tile(opt.tune, 0, c / 16, out_ch / 32, 1, 1 << 30, 1 << 30, 1, TH, TW);
}
// the decode folds into box_dfl + head_cls / a class-rows decode (16-bit handles; the
// box branch's last conv has 4 or 6 16-channel K blocks)
bool Net::fuse_decode(int boxc, int nc) const {
    if (dtype == F32 || !opt.fuse) return false;
    return (boxc == 64 || boxc == 96) && nc % 4 == 0;
}
// a level's cls branch is fused when it has 16-channel blocks, 4-channel class groups
// and an LDS tile next to its resident weights
bool Net::fuse_head_cls(int C0, int c3, int nc) const {
    if (dtype == F32 || !opt.fuse) return false;
    if (c3 % 16 || nc % 4 || C0 % 16) return false;
    if (C0 > 128 && !opt.hcls_wide) return false;
    int TH, TW;
    return head_cls_tile(C0, c3, nc, 1 << 30, 1 << 30, TH, TW);
}

}  // namespace yh
