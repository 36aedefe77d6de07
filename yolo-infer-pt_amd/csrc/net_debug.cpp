// Per-op accounting and the parity taps: class, algorithmic bytes and flops of every op
// (yh_op_info), and the op descriptions, partial runs and operand copies the parity tests use
// (yh_debug_*).
#include "net.h"

namespace yh {

// per OpKind, in the enum's order: its name (yh_op_kernel, op_desc) and its class (yh_op_info)
static const struct { const char* name; OpClass cls; } KINDS[] = {
    {"stem", CL_FIRST}, {"conv", CL_CONV1}, {"dwconv", CL_DW}, {"sppf", CL_SPPF}, {"attention", CL_ATTN},
    {"decode", CL_DECODE}, {"head_cls", CL_HEADCLS}, {"box_dfl", CL_BOXDFL}, {"c3k2", CL_CSP}, {"stem_fused", CL_FIRST},
    {"c3k", CL_C3K}, {"pw_chain", CL_PWCHAIN}, {"cls_pool", CL_CLS}, {"cls_head", CL_CLS},
    {"cls_fc", CL_CLS}};
static_assert(sizeof(KINDS) / sizeof(KINDS[0]) == OP_CLSFC + 1, "one entry per OpKind");
const char* op_kind_name(OpKind k) { return KINDS[k].name; }
OpClass Net::op_class(const Op& op) const {
    return op.kind == OP_CONV && convs[op.conv].k == 3 ? CL_CONV3 : KINDS[op.kind].cls;
}
// algorithmic bytes (each operand read once, output written once) and flops per call
void Net::op_cost(const Op& op, int B, int H, int W, double& bytes, double& flops) const {
    bytes = 0; flops = 0;
    auto px = [&](int level) { return (double)B * (H >> level) * (W >> level); };
    switch (op.kind) {
        case OP_FIRST: {
            const ConvDesc& d = convs[op.conv];
            const double out = px(1);
            bytes = (double)B * 3 * H * W * es + out * d.cout * es + d.cout * 27.0 * 4;
            flops = 2.0 * out * d.cout * 27;
            break;
        }
        case OP_CONV: {
            const ConvDesc& d = convs[op.conv];
            const double out = px(tensors[op.out.t].level);
            for (size_t si = 0; si < op.in.size(); ++si) {
                const Seg& sg = op.in[si];
                bytes += px(tensors[sg.v.t].level) * d.segs[si].first * es;
            }
            bytes += out * d.cout * es + (double)d.cout * d.cin * d.k * d.k * es;
            if (op.has_res) bytes += out * d.cout * es;
            flops = 2.0 * out * d.cout * d.cin * d.k * d.k;
            break;
        }
        case OP_DW: {
            const ConvDesc& d = convs[op.conv];
            const double n = px(tensors[op.out.t].level);
            bytes = 2.0 * n * d.cout * es;
            flops = 2.0 * n * d.cout * 9;
            break;
        }
        case OP_SPPF: {
            const double n = px(tensors[op.out.t].level);
            bytes = 6.0 * n * op.out.C * es;
            flops = 3.0 * n * op.out.C * 25;
            break;
        }
        case OP_ATTN: {
            const double T = (double)(H >> tensors[op.out.t].level) * (W >> tensors[op.out.t].level);
            const double C = op.heads * 64.0;
            bytes = (double)B * T * (op.heads * 128.0 + C) * es;
            flops = (double)B * op.heads * (2.0 * T * T * (32 + 64)) + 2.0 * B * T * C * 9;
            break;
        }
        case OP_HEADCLS: {
            // the level inputs read once, the class logits written once, weights once
            for (int l = 0; l < 3; ++l) {
                if (!op.hlv[l]) continue;
                const double n = px(tensors[op.hx[l].t].level);
                const int C0 = op.hx[l].C;
                const ConvDesc& p1 = convs[op.hc[l][1]];
                const int c3 = p1.cout, nc = convs[op.hc[l][4]].cout;
                bytes += n * C0 * es + n * nc * es + (9.0 * (C0 + c3) * 4) +
                         ((double)C0 * c3 + (double)c3 * c3 + (double)c3 * nc) * es;
                flops += 2.0 * n * (9.0 * C0 + (double)C0 * c3 + 9.0 * c3 + (double)c3 * c3 + (double)c3 * nc);
            }
            break;
        }
        case OP_DECODE: {
            double A = 0;
            for (int l = op.dbox ? 0 : op.dlo; l < 3; ++l) A += px(tensors[op.lvl[l].t].level);
            if (op.dbox) {
                bytes = A * (64 + var.num_classes) * es + A * (4 + var.num_classes) * es;
                flops = A * (64 * 4.0 + var.num_classes * 4.0);
            } else {
                bytes = 2.0 * A * var.num_classes * es;
                flops = A * var.num_classes * 4.0;
            }
            break;
        }
        case OP_STEM2: {
            // the image read once, p2.0's output written once, both weights once
            const ConvDesc& d = convs[op.conv];
            const ConvDesc& d2 = convs[op.cs[0]];
            const double s1 = px(1), o2 = px(2);
            bytes = (double)B * 3 * H * W * (in_u8 ? 1 : es) + o2 * d2.cout * es + d.cout * 27.0 * 4 +
                    (double)d2.cout * d2.cin * 9 * es;
            flops = 2.0 * s1 * d.cout * 27 + 2.0 * o2 * d2.cout * d2.cin * 9;
            break;
        }
        case OP_CSP: case OP_C3K: {
            // block input read once (C3k: conv1 and conv2 share it), block output written once,
            // the block's four / seven convs' weights once
            const double n = px(tensors[op.out.t].level);
            const std::vector<int> cv = op_convs(op);
            bytes = n * op.in[0].v.C * es + n * convs[cv.back()].cout * es;
            for (int ci : cv) {
                if (ci < 0) continue;   // C3k2 tail mode: conv1 is its own op
                const ConvDesc& d = convs[ci];
                const double macs = (double)d.cout * d.cin * d.k * d.k;
                bytes += macs * es;
                flops += 2.0 * n * macs;
            }
            break;
        }
        case OP_PWCHAIN: {
            // the prologue's global inputs (incl. the global residuals) read once, every stage's
            // output written (all stay materialised), each stage's weights once
            const double n = px(tensors[op.out.t].level);
            for (const View& v : op.pwl) bytes += n * v.C * es;
            for (size_t k = 0; k < op.pws.size(); ++k) {
                const Op& o = ops[op.alts[k]];
                const ConvDesc& d = convs[o.conv];
                bytes += n * d.cout * es + (double)d.cout * d.cin * es;
                flops += 2.0 * n * d.cout * d.cin;
            }
            break;
        }
        case OP_CLSPOOL:
            // the activations read once, the fp32 embedding written once
            bytes = px(5) * op.out.C * es + (double)B * op.out.C * 4;
            flops = px(5) * op.out.C;
            break;
        case OP_CLSHEAD: {
            // the feature map read once, the fp32 embedding written once, the weights once
            const ConvDesc& d = convs[op.conv];
            bytes = px(5) * d.cin * es + (double)B * d.cout * 4 + (double)d.cout * d.cin * es + d.cout * 4.0;
            flops = 2.0 * px(5) * d.cout * d.cin + px(5) * d.cout;
            break;
        }
        case OP_CLSFC: {
            // the embedding read once; logits, probs and the embedding copy written once; weights once
            const ConvDesc& d = convs[op.conv];
            bytes = (double)B * d.cin * 4 * 2 + 2.0 * B * d.cout * 4 + (double)d.cout * d.cin * es + d.cout * 4.0;
            flops = 2.0 * B * d.cout * d.cin + 4.0 * B * d.cout;
            break;
        }
        case OP_BOXDFL: {
            // the box.l.1 outputs read once, 4 box rows written, weights once per level
            for (int l = 0; l < 3; ++l) {
                const double n = px(tensors[op.bx[l].t].level);
                const int K = op.bx[l].C;
                bytes += n * K * es + n * 4 * es + 64.0 * K * es + 64 * 4.0;
                flops += 2.0 * n * 64 * K + n * 64 * 4.0;
            }
            break;
        }
    }
}

// ---------------------------------------------------------- parity taps (tests only)
// The workspace operands of an op, in a fixed order (yh_debug_op_desc lists them):
// inputs first, then outputs. `logical` = channels the op reads / writes of the view.
std::vector<Net::Operand> Net::operands(const Op& op) const {
    std::vector<Operand> r;
    auto add = [&](const std::string& role, const View& v, int up, int logical) { r.push_back(Operand{role, v, up, logical}); };
    switch (op.kind) {
        case OP_CONV: {
            const ConvDesc& d = convs[op.conv];
            for (size_t si = 0; si < op.in.size(); ++si)
                add("in" + std::to_string(si), op.in[si].v, op.in[si].up, d.segs[si].first);
            if (op.has_res) add("res", op.res, 0, d.cout);
            add("out", op.out, 0, d.cout);
            break;
        }
        case OP_FIRST: case OP_STEM2: add("out", op.out, 0, op.out.C); break;
        case OP_DW: case OP_ATTN: case OP_CSP: case OP_C3K:
            add("in0", op.in[0].v, op.in[0].up, op.in[0].v.C);
            add("out", op.out, 0, op.out.C);
            break;
        case OP_SPPF:
            add("in0", op.out, 0, op.out.C);
            add("out", View{op.out.t, op.out.coff + op.out.C, 3 * op.out.C}, 0, 3 * op.out.C);
            break;
        case OP_HEADCLS:
            for (int l = 0; l < 3; ++l)
                if (op.hlv[l]) add("x" + std::to_string(l), op.hx[l], 0, op.hx[l].C);
            if (!op.direct)
                for (int l = 0; l < 3; ++l)
                    if (op.hlv[l]) add("y" + std::to_string(l), op.hy[l], 0, var.num_classes);
            break;
        case OP_BOXDFL:
            for (int l = 0; l < 3; ++l) add("x" + std::to_string(l), op.bx[l], 0, op.bx[l].C);
            break;
        case OP_DECODE:
            for (int l = 0; l < 3; ++l) add("L" + std::to_string(l), op.lvl[l], 0, 64 + var.num_classes);
            break;
        case OP_CLSPOOL:   // a (the head conv's output), e (fp32)
            add("a", op.in[0].v, 0, op.in[0].v.C);
            add("e", op.out, 0, op.out.C);
            break;
        case OP_CLSHEAD:
            add("in0", op.in[0].v, 0, op.in[0].v.C);
            add("e", op.out, 0, op.out.C);
            break;
        case OP_CLSFC:     // e and the logits z (both fp32)
            add("e", op.in[0].v, 0, op.in[0].v.C);
            add("z", op.out, 0, var.num_classes);
            break;
        case OP_PWCHAIN:
            // per stage s<k>.in<i> / s<k>.res (inputs, read before the chain runs), then the
            // outputs no later stage overwrites (s<k>.out)
            for (size_t k = 0; k < op.alts.size(); ++k) {
                const Op& o = ops[op.alts[k]];
                const ConvDesc& d = convs[o.conv];
                const std::string p = "s" + std::to_string(k) + ".";
                for (size_t si = 0; si < o.in.size(); ++si) add(p + "in" + std::to_string(si), o.in[si].v, 0, d.segs[si].first);
                if (o.has_res) add(p + "res", o.res, 0, d.cout);
            }
            for (size_t k = 0; k < op.alts.size(); ++k)
                if (pw_final(op, (int)k)) {
                    const Op& o = ops[op.alts[k]];
                    add("s" + std::to_string(k) + ".out", o.out, 0, convs[o.conv].cout);
                }
            break;
    }
    return r;
}
// stage k's output is not overwritten by a later stage of the chain
bool Net::pw_final(const Op& op, int k) const {
    const Op& o = ops[op.alts[k]];
    const int c0 = o.out.coff, c1 = c0 + convs[o.conv].cout;
    for (size_t q = k + 1; q < op.alts.size(); ++q) {
        const Op& w = ops[op.alts[q]];
        const int w0 = w.out.coff, w1 = w0 + convs[w.conv].cout;
        if (w.out.t == o.out.t && w0 < c1 && c0 < w1) return false;
    }
    return true;
}
// the convs an op computes, in the op's order (-1: none in that place, e.g. tail-mode conv1)
std::vector<int> Net::op_convs(const Op& op) const {
    std::vector<int> r;
    switch (op.kind) {
        case OP_CONV: case OP_FIRST: case OP_DW: case OP_ATTN: case OP_CLSHEAD: case OP_CLSFC: return {op.conv};
        case OP_STEM2: return {op.conv, op.cs[0]};
        case OP_CSP: return {op.cs[0], op.cs[1], op.cs[2], op.cs[3]};
        case OP_C3K: return std::vector<int>(op.ck, op.ck + 7);
        case OP_HEADCLS:
            for (int l = 0; l < 3; ++l)
                for (int k = 0; k < 5; ++k) r.push_back(op.hlv[l] ? op.hc[l][k] : -1);
            break;
        case OP_BOXDFL: return {op.bc[0], op.bc[1], op.bc[2]};
        case OP_PWCHAIN:
            for (int k : op.alts) r.push_back(ops[k].conv);
            break;
        case OP_SPPF: case OP_DECODE: case OP_CLSPOOL: break;
    }
    return r;
}
std::string Net::op_desc(int oi, int B, int H, int W) const {
    const Op& op = ops[oi];
    auto it = plans.find(GraphKey{B, H, W});
    const int active = it == plans.end() ? -1 : it->second.active[oi];
    std::string s = "{\"index\": " + std::to_string(oi) + ", \"kind\": \"" + op_kind_name(op.kind) +
                    "\", \"label\": \"" + op.label + "\", \"active\": " + std::to_string(active) +
                    ", \"heads\": " + std::to_string(op.heads) + ", \"direct\": " + std::to_string(op.direct ? 1 : 0) +
                    ", \"dlo\": " + std::to_string(op.dlo) + ", \"dbox\": " + std::to_string(op.dbox ? 1 : 0) +
                    ", \"convs\": [";
    const std::vector<int> cv = op_convs(op);
    for (size_t i = 0; i < cv.size(); ++i) {
        if (i) s += ", ";
        if (cv[i] < 0) { s += "null"; continue; }
        const ConvDesc& d = convs[cv[i]];
        s += "{\"name\": \"" + d.name + "\", \"k\": " + std::to_string(d.k) + ", \"s\": " + std::to_string(d.stride) +
             ", \"g\": " + std::to_string(d.groups) + ", \"act\": " + std::to_string(d.act) + ", \"cin\": " +
             std::to_string(d.cin) + ", \"cout\": " + std::to_string(d.cout) + ", \"bias\": " +
             std::to_string(d.has_bias) + "}";
    }
    s += "], \"operands\": [";
    const std::vector<Operand> od = operands(op);
    for (size_t i = 0; i < od.size(); ++i) {
        // a per-image fp32 vector (level < 0) reads as a 1 x 1 map with "f32": 1
        const int lv = tensors[od[i].v.t].level;
        const int oh = lv < 0 ? 1 : H >> lv, ow = lv < 0 ? 1 : W >> lv;
        s += std::string(i ? ", " : "") + "{\"role\": \"" + od[i].role + "\", \"H\": " + std::to_string(oh) +
             ", \"W\": " + std::to_string(ow) + ", \"C\": " + std::to_string(od[i].v.C) + ", \"logical\": " +
             std::to_string(od[i].logical) + ", \"up\": " + std::to_string(od[i].up) + ", \"f32\": " +
             std::to_string(lv < 0 ? 1 : 0) + "}";
    }
    s += "]";
    if (op.kind == OP_PWCHAIN) {
        // per stage: its input runs in weight order (seg = input segment, off = channel within
        // it; src = -1: that device operand, else the output of stage src from channel soff) and
        // its residual source (-2 none, -1 the s<k>.res operand, else a stage's output)
        s += ", \"stages\": [";
        for (size_t k = 0; k < op.pws.size(); ++k) {
            const Op& o = ops[op.alts[k]];
            const Op::PwStage& ps = op.pws[k];
            s += std::string(k ? ", " : "") + "{\"runs\": [";
            int si = 0, soff = 0;
            for (size_t r = 0; r < ps.runs.size(); ++r) {
                const Op::PwRun& pr = ps.runs[r];
                while (soff >= o.in[si].v.C) {
                    soff -= o.in[si].v.C;
                    ++si;
                }
                s += std::string(r ? ", " : "") + "{\"seg\": " + std::to_string(si) + ", \"off\": " +
                     std::to_string(soff) + ", \"n\": " + std::to_string(pr.nch) + ", \"src\": " +
                     std::to_string(pr.stage) + ", \"soff\": " + std::to_string(pr.stage >= 0 ? pr.coff : 0) + "}";
                soff += pr.nch;
            }
            s += "], \"res\": " + std::to_string(o.has_res ? ps.res_stage : -2) + ", \"res_off\": " +
                 std::to_string(ps.res_coff) + ", \"final\": " + std::to_string(pw_final(op, (int)k) ? 1 : 0) + "}";
        }
        s += "]";
    }
    s += "}";
    return s;
}
// the active ops in [first, last) of the forward at (B, H, W), launched eagerly on s
void Net::debug_run(const void* x, int x_u8, int B, int H, int W, void* y, int first, int last, hipStream_t s) {
    // a classifier handle's y is its (B, num_classes) fp32 probs; no logits / embed copies, no count
    in_u8 = x_u8;
    for (auto& d : convs) require(d.loaded, "weights of " + d.name + " not loaded", YH_ESTATE);
    require(ws.base && ws.B == B && ws.H == H && ws.W == W, "yh_debug_run_ops: run yh_forward at this shape first",
            YH_ESTATE);
    require(first >= 0 && first <= last && last <= (int)ops.size(), "op range out of bounds");
    HIPCHECK(hipSetDevice(device));
    const int rc = task == 1 ? launch_set_io_cls(io_dev, x, (float*)y, nullptr, nullptr, nullptr, s) : launch_set_io(io_dev, x, y, s);
    require(rc == 0, "set_io launch failed", YH_EHIP);
    ensure_plan(B, H, W);
    ensure_tuned(B, H, W, s);
    for (int i = first; i < last; ++i)
        if (cur_plan->active[i]) launch_op((size_t)i, B, H, W, s);
}
// operand `slot` of op `oi` copied out of the workspace as a dense (B, h, w, C) array
void Net::debug_operand(int oi, int slot, void* dst, size_t dst_bytes, hipStream_t s) const {
    require(oi >= 0 && oi < (int)ops.size(), "op index out of range");
    const std::vector<Operand> od = operands(ops[oi]);
    require(slot >= 0 && slot < (int)od.size(), "operand slot out of range");
    require(ws.base != nullptr, "no workspace yet", YH_ESTATE);
    const View& v = od[slot].v;
    const int lv = tensors[v.t].level;
    const size_t rows = lv < 0 ? (size_t)ws.B : (size_t)ws.B * (ws.H >> lv) * (ws.W >> lv);
    const int es = lv < 0 ? 4 : this->es;   // per-image vectors are fp32 on every handle
    // the caller sizes dst from a desc made at some (batch, H, W): a desc of another shape
    // (or a later reserve() at a larger one) must not turn into an out-of-bounds write
    require(dst_bytes == rows * (size_t)v.C * es, "yh_debug_operand: dst size " + std::to_string(dst_bytes) +
            " B does not match the operand at the workspace shape (" + std::to_string(rows * (size_t)v.C * es) +
            " B)");
    HIPCHECK(hipMemcpy2DAsync(dst, (size_t)v.C * es, ptr(v), (size_t)ldc(v) * es, (size_t)v.C * es, rows,
                              hipMemcpyDeviceToDevice, s));
}

}  // namespace yh
