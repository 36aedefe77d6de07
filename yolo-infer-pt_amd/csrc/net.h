// The host runtime's model of one handle: the layer graph of a variant (mirroring the reference
// module tree, nets/nn.py:28-305), its folded weights, the NHWC activation workspace and the
// per-shape launch state. Net's members are defined in net_build.cpp (graph and fusion passes),
// net_weights.cpp (folding, upload, packed images), net_forward.cpp (workspace, plans, captured
// graphs), net_launch.cpp (launch arguments, launch_op, autotuner) and net_debug.cpp (per-op
// accounting, parity taps); engine.cpp exports the handle's C ABI.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "conv_mx.h"
#include "host_util.h"

namespace yh {

// ---------------------------------------------------------------- graph model
enum ConvKind { CK_DENSE = 0, CK_FIRST = 1, CK_DW = 2, CK_PE = 3 };
enum OpKind { OP_FIRST, OP_CONV, OP_DW, OP_SPPF, OP_ATTN, OP_DECODE, OP_HEADCLS, OP_BOXDFL, OP_CSP, OP_STEM2, OP_C3K,
              OP_PWCHAIN, OP_CLSPOOL, OP_CLSHEAD, OP_CLSFC };
const char* op_kind_name(OpKind k);
enum OpClass { CL_CONV3 = 0, CL_CONV1 = 1, CL_FIRST = 2, CL_DW = 3, CL_SPPF = 4, CL_ATTN = 5, CL_DECODE = 6,
               CL_HEADCLS = 7, CL_BOXDFL = 8, CL_CSP = 9, CL_C3K = 10, /* 11: unused */ CL_PWCHAIN = 12, CL_CLS = 13, CL_N = 14 };

// level < 0: one fp32 vector of C values per image (the classifier's embedding and logits)
struct Tensor { int level; int C; };        // physical channels = pixel stride
struct View { int t = -1; int coff = 0; int C = 0; };

struct Seg { View v; int up = 0; };

struct ConvDesc {
    std::string name;
    ConvKind kind;
    int cout, cin, k, stride, groups, has_bias, act;
    std::vector<std::pair<int, int>> segs;   // (logical, physical) channel counts of the input
    int cin_p = 0, cout_p = 0, K = 0, Kp = 0, coutp_pad = 0;
    bool loaded = false;
    std::vector<float> wf, bf;  // folded fp32 weights (cout, cin/g, k, k) and bias (cout)
    void* w_dev = nullptr;
    float* b_dev = nullptr;
    int* ktab_dev = nullptr;
    std::vector<int> phys2log;                  // dense: physical input channel -> logical (-1 = pad)
    // 16-bit dense: packed weights per conv_mx layout, "pwfrag", and the fused ops' parameter
    // images with their dependency markers (Net::fused_params); all dropped by a reload
    std::map<std::string, void*> mx_w;
};

struct Op {
    OpKind kind;
    int conv = -1;
    std::vector<Seg> in;
    View out, res;
    bool has_res = false;
    int heads = 0;
    View lvl[3];
    // OP_HEADCLS: per level (index = detect level 0..2) the five convs of the cls branch
    // (dw1, pw1, dw2, pw2, pw3), the level input and the head tensor's cls slice
    int hc[3][5] = {};
    View hx[3], hy[3];
    bool hlv[3] = {false, false, false};   // levels the fused op covers
    bool direct = false;                   // OP_HEADCLS: scores straight into y (decode folded in)
    // OP_BOXDFL: per level the last box conv and its input (the box.l.1 output)
    int bc[3] = {-1, -1, -1};
    View bx[3];
    // OP_DECODE: first level decoded, and whether the box rows are (false: box_dfl writes them)
    int dlo = 0;
    bool dbox = true;
    // OP_CSP: conv1, res_m.0.conv1, res_m.0.conv2, conv2 of a fused C3k2 block (in[0] -> out)
    // OP_STEM2: cs[0] = net.p2.0 (conv = the stem)
    int cs[4] = {-1, -1, -1, -1};
    // OP_C3K: conv1, conv2, res_m.0.conv1, res_m.0.conv2, res_m.1.conv1, res_m.1.conv2, conv3 of
    // a CSPModule
    int ck[7] = {-1, -1, -1, -1, -1, -1, -1};
    // OP_C3K, OP_PWCHAIN: the per-layer ops this op replaces at shapes where it fits
    // (Net::fused_fits); exactly one side is active in a plan. OP_C3K: the block's seven convs.
    // OP_PWCHAIN: the member 1x1 conv ops (stages, in order)
    std::vector<int> alts;
    // OP_PWCHAIN: per stage its input runs (16-channel blocks in weight order: LDS region of an
    // earlier stage's output, or a prologue-loaded global view), its residual and whether its
    // output is kept in LDS
    struct PwRun { int stage = -1; int coff = 0; int nch = 0; int load = -1; };   // coff: channel in the source
    struct PwStage { std::vector<PwRun> runs; int res_stage = -2; int res_coff = 0; int res_load = -1; bool keep = false; int lds = -1; };
    std::vector<PwStage> pws;
    std::vector<View> pwl;          // prologue loads (global views)
    std::vector<int> pwl_lds;       // their LDS byte offsets
    int pwP = 0, pwLds = 0;
    // OP_CLSPOOL: in[0] = the head conv's output, out = the embedding vector. OP_CLSHEAD: conv =
    // head.conv, in[0] = its input, out = the embedding (alts: the conv op and the pool).
    // OP_CLSFC: conv = head.linear, in[0] = the embedding, out = the logits vector
    std::string label;
};

struct Workspace {
    int B = 0, H = 0, W = 0;
    void* base = nullptr;
    size_t bytes = 0;
    std::vector<size_t> off;  // per tensor
};

struct GraphKey {
    int B, H, W;
    int X = 0;   // input kind of a captured forward graph: 0 = handle dtype, 1 = uint8
    bool operator<(const GraphKey& o) const {
        return B != o.B ? B < o.B : (H != o.H ? H < o.H : (W != o.W ? W < o.W : X < o.X));
    }
};

// Every environment switch of the library, read once per handle at yh_create / yh_create_cls and
// at no later moment (INTEGRATION.md lists them): a handle keeps its switches for its life, on the
// eager path and in every captured graph alike. YH_FUSE=0 turns every cross-layer fusion off (the
// bit-identity tests compare both), YH_CSP_TAIL=1 forces the C3k2 tail mode where
// the whole block would fit one launch (tested the same way), YH_CONV=<k> forces
// candidate plan k of every 16-bit dense conv, YH_TUNE_LOG=1 prints the tuner's timings,
// YH_C3K=0 keeps the C3k blocks as per-layer launches (compared bit for bit by the tests),
// YH_HCLS_WIDE=0 keeps a 256-channel level's cls branch (v11_n 20x20) as per-layer launches,
// YH_CLSHEAD=1 runs a classifier's head.conv + cls_pool as one launch (cls_head; bit-identical, compared
// by the tests; off by default because the two launches measured faster).
// The kernel-variant switches fill `tune` (common.h Tuning), which the launchers get with the CU
// count: YH_ATTN_FULL, YH_ATTN_LDS, YH_ATTN_NW, YH_ATTN_QS, YH_SPPF_FUSED, YH_SPPF_CPW, YH_SPPF_XCD,
// YH_C3K_BANDS, YH_C3K_NB, YH_CSP_TILE, YH_BOXDFL_TPW, YH_PWC_WARM.
struct Options {
    bool fuse = true, csp_tail = false, tune_log = false, c3k = true, hcls_wide = true, pw_chain = true;
    bool cls_head = false;
    int conv_force = -1;
    Tuning tune;
    static Options from_env() {
        Options o;
        Tuning& t = o.tune;
        if (const char* e = getenv("YH_ATTN_FULL")) t.attn_full = atoi(e) != 0;
        if (const char* e = getenv("YH_ATTN_LDS")) t.attn_lds = atoi(e) != 0;
        if (const char* e = getenv("YH_ATTN_NW")) t.attn_nw = atoi(e) == 8 ? 8 : 16;
        // a count that is set is at least 1; the launchers clamp it to what the shape allows
        if (const char* e = getenv("YH_ATTN_QS")) t.attn_qs = std::max(1, atoi(e));
        if (const char* e = getenv("YH_SPPF_FUSED")) t.sppf_fused = atoi(e) != 0;
        if (const char* e = getenv("YH_SPPF_CPW")) t.sppf_cpw = std::max(1, atoi(e));
        if (const char* e = getenv("YH_SPPF_XCD")) t.sppf_xcd = atoi(e);
        if (const char* e = getenv("YH_C3K_BANDS")) t.c3k_bands = std::max(1, atoi(e));
        if (const char* e = getenv("YH_C3K_NB")) t.c3k_nb = std::max(1, atoi(e));
        if (const char* e = getenv("YH_CSP_TILE")) {
            int th = 0, tw = 0;
            if (sscanf(e, "%dx%d", &th, &tw) == 2 && th > 0 && tw > 0) { t.csp_th = th; t.csp_tw = tw; }
        }
        if (const char* e = getenv("YH_BOXDFL_TPW"))
            if (const int v = atoi(e); v == 1 || v == 2 || v == 4) t.boxdfl_tpw = v;
        if (const char* e = getenv("YH_PWC_WARM")) t.pwc_warm = atoi(e) != 0;
        if (const char* e = getenv("YH_FUSE")) o.fuse = atoi(e) != 0;
        if (const char* e = getenv("YH_PWCHAIN")) o.pw_chain = atoi(e) != 0;
        if (const char* e = getenv("YH_CSP_TAIL")) o.csp_tail = atoi(e) != 0;
        if (const char* e = getenv("YH_C3K")) o.c3k = atoi(e) != 0;
        if (const char* e = getenv("YH_HCLS_WIDE")) o.hcls_wide = atoi(e) != 0;
        if (const char* e = getenv("YH_CLSHEAD")) o.cls_head = atoi(e) != 0;
        if (const char* e = getenv("YH_CONV")) o.conv_force = atoi(e);
        o.tune_log = getenv("YH_TUNE_LOG") != nullptr;
        return o;
    }
};

struct Net {
    yh_variant var;
    int task = 0;   // 0: detection (yh_create), 1: classification (yh_create_cls)
    Options opt;
    int device, dtype, es;
    std::vector<Tensor> tensors;
    std::vector<ConvDesc> convs;
    std::vector<Op> ops;
    Workspace ws;
    void** io_dev = nullptr;      // {x, y, probs, logits, embed, count} (the last four: classifier)
    void* zero_dev = nullptr;     // 256 zero bytes: source of padded conv taps
    bool use_graph = true;
    std::map<GraphKey, hipGraphExec_t> graphs;
    hipStream_t cap_stream = nullptr;
    bool profile = false;
    std::vector<double> prof_ms;     // per launch of the profiled shape's plan (Plan::order)
    std::vector<int> prof_calls;
    GraphKey prof_key{0, 0, 0};
    std::vector<hipEvent_t> ev;
    int in_u8 = 0;   // the current forward's input kind (see GraphKey::X)
    // 16-bit dense convs: the conv_mx plan chosen for every op at a shape (all plans of a
    // layer are bit-identical, the choice only changes speed), timed once per (B, H, W)
    // on the caller's stream or forced by yh_force_conv_kernel / YH_CONV=<candidate>
    struct MxChoice { MxPlan plan; std::string name; };
    std::map<GraphKey, std::vector<MxChoice>> conv_kern;
    const std::vector<MxChoice>* cur_kern = nullptr;
    int force_kern = -1;   // candidate index (testing); -1 = autotune
    int num_cus = 0;       // queried at create
    LaunchCtx ctx() const { return LaunchCtx{num_cus, opt.tune}; }
    // plan string of every fused C3k2 launch made so far: c3k2_t<TH>x<TW>, per shape and op index
    std::map<std::pair<GraphKey, int>, std::string> csp_plan;
    // the forward at one shape: which ops are launched (fused blocks pick per shape) and their
    // order. yh_unit_count / yh_unit_info list `order` (one op per unit).
    struct Plan {
        std::vector<char> active;   // per op
        std::vector<int> order;     // the active op indices, ascending
    };
    std::map<GraphKey, Plan> plans;
    const Plan* cur_plan = nullptr;

    ~Net();

    // ---------------------------------------------------------- net_build.cpp
    void build();
    int build_backbone(int& b3, int& b4);
    void build_cls();
    int tensor(int level, int C);
    View full(int t, int C = -1) const { return View{t, 0, C < 0 ? tensors[t].C : C}; }
    View slice(int t, int coff, int C) const;
    int new_conv(const std::string& name, ConvKind kind, int cin, int cout, int k, int s, int g, int has_bias, int act);
    int new_dense_conv(const std::string& name, int cin, int cout, int k, int has_bias, int act);
    void dense(const std::string& name, const std::vector<Seg>& in, const std::vector<int>& logical, int cout, int k,
               int s, int act, View out, const View* res = nullptr, int has_bias = 0);
    View conv1(const std::string& name, View x, int xc, int cout, int act, View out, const View* res = nullptr);
    View conv3(const std::string& name, View x, int xc, int cout, int s, int act, View out, const View* res = nullptr);
    void dw(const std::string& name, View x, int ch, View out);
    void residual(const std::string& p, View x, int ch, double e, View out, int level);
    void cspmodule(const std::string& p, View x, int in_ch, int out_ch, View out, int level);
    void csp(const std::string& p, const std::vector<Seg>& in, const std::vector<int>& logical, int out_ch, int n,
             bool use_c3k, int r, View out, int level);
    void sppf(const std::string& p, View x, int in_ch, int out_ch, View out, int level);
    void psablock(const std::string& p, View x, int ch, int heads, int level);
    void psa(const std::string& p, View x, int ch, int n, View out, int level);
    void finalize_convs();
    void fuse_pw_chains();
    bool make_pw_chain(size_t i, size_t e);
    bool fuse_stem(int c0, int c1, int c2) const;
    bool fuse_csp(const std::vector<Seg>& in, const std::vector<int>& logical, int c, int out_ch, View out) const;
    bool fuse_csp_tail(int c, int out_ch, View out) const;
    bool fuse_decode(int boxc, int nc) const;
    bool fuse_head_cls(int C0, int c3, int nc) const;

    // ---------------------------------------------------------- net_weights.cpp
    void load_conv(int idx, const float* w, const float* b, const float* g, const float* be, const float* mu,
                   const float* var_, double eps);
    void upload(ConvDesc& d);
    void* to_device(const std::vector<float>& v) const;
    static void free_conv(ConvDesc& d);
    uint16_t to16(float v) const { return dtype == BF16 ? f2bf(v) : f2h(v); }
    const void* fused_params(int owner, const std::string& key, const std::vector<int>& others,
                             const std::function<std::vector<uint8_t>()>& image);
    const void* stem2_params(const Op& op, int& bias_off, int& stem_off);
    const void* csp_params(const Op& op);
    const void* c3k_params(const Op& op);
    const char* mx_weights(int ci, const MxPlan& p, const MxShape& sh);

    // ---------------------------------------------------------- net_forward.cpp
    size_t tensor_bytes(const Tensor& t, int B, int H, int W) const;
    size_t ws_bytes_for(int B, int H, int W, std::vector<size_t>* offs) const;
    void check_shape(int B, int H, int W) const;
    void reserve(int B, int H, int W);
    char* ptr(const View& v) const { return (char*)ws.base + ws.off[v.t] + (size_t)v.coff * es; }
    int ldc(const View& v) const { return tensors[v.t].C; }
    void drop_graphs();
    bool fused_fits(const Op& op, int B, int H, int W) const;
    void ensure_plan(int B, int H, int W);
    void run_ops(int B, int H, int W, hipStream_t s);
    void forward(const void* x, int B, int H, int W, void* y, hipStream_t s, int x_u8 = 0);
    void classify(const void* x, int x_u8, int B, int H, int W, const int* count, float* probs, float* logits,
                  float* embed, hipStream_t s);
    void launch_plan(int B, int H, int W, hipStream_t s);

    // ---------------------------------------------------------- net_launch.cpp
    static int anchor_off(int l, int H, int W);
    static bool csp_tile(const Tuning& tune, int ni, int nc, int no, int B, int H, int W, int cus, int& TH, int& TW);
    static bool head_cls_tile(int C0, int c3, int nc, int H, int W, int& TH, int& TW);
    void conv_args(const Op& op, int B, int H, int W, ConvArgs& a, int& BM, int& BN) const;
    MxShape mx_shape(const ConvArgs& a, int B) const;
    FirstConvArgs first_args(const Op& op, int B, int H, int W) const;
    Stem2Args stem2_args(const Op& op, int B, int H, int W);
    DwArgs dw_args(const Op& op, int B, int H, int W) const;
    PoolArgs pool_args(const Op& op, int B, int H, int W) const;
    AttnArgs attn_args(const Op& op, int H, int W) const;
    DecodeArgs decode_args(const Op& op, int B, int H, int W) const;
    HeadClsArgs head_cls_args(const Op& op, int B, int H, int W);
    BoxDflArgs box_dfl_args(const Op& op, int B, int H, int W);
    PwChainArgs pw_chain_args(const Op& op, int B, int H, int W);
    CspArgs csp_args(size_t oi, int B, int H, int W, int& grid);
    C3kArgs c3k_args(const Op& op, int B, int H, int W);
    ClsPoolArgs cls_pool_args(const Op& op, int B, int H, int W) const;
    ClsHeadArgs cls_head_args(const Op& op, int B, int H, int W) const;
    ClsFcArgs cls_fc_args(const Op& op, int B) const;
    int launch_mx_op(const Op& op, const MxPlan& pl, int B, int H, int W, hipStream_t s);
    void launch_op(size_t oi, int B, int H, int W, hipStream_t s);
    void ensure_tuned(int B, int H, int W, hipStream_t s);

    // ---------------------------------------------------------- net_debug.cpp
    struct Operand { std::string role; View v; int up = 0; int logical = 0; };
    OpClass op_class(const Op& op) const;
    void op_cost(const Op& op, int B, int H, int W, double& bytes, double& flops) const;
    std::vector<Operand> operands(const Op& op) const;
    bool pw_final(const Op& op, int k) const;
    std::vector<int> op_convs(const Op& op) const;
    std::string op_desc(int oi, int B, int H, int W) const;
    void debug_run(const void* x, int x_u8, int B, int H, int W, void* y, int first, int last, hipStream_t s);
    void debug_operand(int oi, int slot, void* dst, size_t dst_bytes, hipStream_t s) const;
};

}  // namespace yh
