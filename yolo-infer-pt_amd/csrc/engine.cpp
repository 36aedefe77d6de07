// The handle's C ABI (include/yolo_hip.h): argument checks and error codes around yh::Net.
#include <algorithm>
#include <memory>

#include "net.h"

struct yh_handle {
    yh::Net net;
};

using yh::Fail;
using yh::guarded;

extern "C" {

int yh_abi_version(void) { return YH_ABI_VERSION; }

const char* yh_last_error(void) { return yh::g_err.c_str(); }

static int create(const yh_variant* v, int device, int dtype, yh_handle** out, int task) {
    return guarded([&] {
        yh::require(v && out, "null argument");
        yh::require(dtype == YH_F32 || dtype == YH_F16 || dtype == YH_BF16, "dtype must be YH_F32, YH_F16 or YH_BF16");
        yh::require(v->num_classes > 0, "num_classes must be positive");
        for (int i = 1; i < 6; ++i) yh::require(v->width[i] > 0 && v->width[i] % 8 == 0, "widths must be multiples of 8");
        yh::require(v->width[0] == 3, "input channels (width[0]) must be 3");
        for (int i = 0; i < 6; ++i) yh::require(v->depth[i] >= 1, "depths must be >= 1");
        int ndev = 0;
        HIPCHECK(hipGetDeviceCount(&ndev));
        yh::require(device >= 0 && device < ndev, "device ordinal out of range");
        HIPCHECK(hipSetDevice(device));
        std::unique_ptr<yh_handle> h(new yh_handle());
        yh::Net& n = h->net;
        n.var = *v;
        n.task = task;
        n.opt = yh::Options::from_env();
        n.device = device;
        HIPCHECK(hipDeviceGetAttribute(&n.num_cus, hipDeviceAttributeMultiprocessorCount, device));
        yh::require(n.num_cus > 0, "device reports no compute units");
        n.dtype = dtype;
        n.es = yh::dtype_size(dtype);
        n.build();
        HIPCHECK(hipMalloc(&n.io_dev, 6 * sizeof(void*)));
        HIPCHECK(hipMemset(n.io_dev, 0, 6 * sizeof(void*)));
        HIPCHECK(hipMalloc(&n.zero_dev, 256));
        HIPCHECK(hipMemset(n.zero_dev, 0, 256));
        *out = h.release();
    });
}

int yh_create(const yh_variant* v, int device, int dtype, yh_handle** out) { return create(v, device, dtype, out, 0); }
int yh_create_cls(const yh_variant* v, int device, int dtype, yh_handle** out) { return create(v, device, dtype, out, 1); }

void yh_destroy(yh_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->net.device);
    delete h;
}

int yh_conv_count(const yh_handle* h) { return h ? (int)h->net.convs.size() : YH_EINVAL; }

int yh_conv_info(const yh_handle* h, int index, const char** name, int* cout, int* cin_per_group, int* ksize,
                 int* groups, int* has_bias) {
    return guarded([&] {
        yh::require(h && index >= 0 && index < (int)h->net.convs.size(), "conv index out of range");
        const yh::ConvDesc& d = h->net.convs[index];
        if (name) *name = d.name.c_str();
        if (cout) *cout = d.cout;
        if (cin_per_group) *cin_per_group = d.cin / d.groups;
        if (ksize) *ksize = d.k;
        if (groups) *groups = d.groups;
        if (has_bias) *has_bias = d.has_bias;
    });
}

int yh_load_conv(yh_handle* h, int index, const float* weight, const float* bias, const float* bn_gamma,
                 const float* bn_beta, const float* bn_mean, const float* bn_var, double bn_eps) {
    return guarded([&] {
        yh::require(h && weight, "null argument");
        yh::require(!bn_gamma || (bn_beta && bn_mean && bn_var), "BatchNorm needs gamma, beta, mean and var");
        HIPCHECK(hipSetDevice(h->net.device));
        h->net.load_conv(index, weight, bias, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps);
        h->net.drop_graphs();   // captured graphs hold the old weight pointers
    });
}

int yh_num_anchors(const yh_handle* h, int height, int width, int* anchors) {
    return guarded([&] {
        yh::require(h && anchors, "null argument");
        yh::require(h->net.task == 0, "yh_num_anchors: a classifier handle has no anchors", YH_ESTATE);
        yh::require(height > 0 && width > 0 && height % 32 == 0 && width % 32 == 0, "height/width must be multiples of 32");
        *anchors = yh::Net::anchor_off(3, height, width);
    });
}

int yh_workspace_bytes(const yh_handle* h, int batch, int height, int width, size_t* bytes) {
    return guarded([&] {
        yh::require(h && bytes, "null argument");
        yh::require(batch > 0 && height % 32 == 0 && width % 32 == 0, "bad shape");
        *bytes = h->net.ws_bytes_for(batch, height, width, nullptr);
    });
}

int yh_reserve(yh_handle* h, int batch, int height, int width) {
    return guarded([&] {
        yh::require(h, "null handle");
        HIPCHECK(hipSetDevice(h->net.device));
        h->net.reserve(batch, height, width);
    });
}

static int forward(yh_handle* h, const void* x, int batch, int height, int width, void* y, void* stream, int x_u8) {
    return guarded([&] {
        yh::require(h && x && y, "null argument");
        yh::require(batch > 0, "batch must be positive");
        yh::require(h->net.task == 0, "yh_forward on a classifier handle (made by yh_create_cls): call yh_classify", YH_ESTATE);
        HIPCHECK(hipSetDevice(h->net.device));
        h->net.forward(x, batch, height, width, y, (hipStream_t)stream, x_u8);
    });
}
int yh_forward(yh_handle* h, const void* x, int batch, int height, int width, void* y, void* stream) {
    return forward(h, x, batch, height, width, y, stream, 0);
}
int yh_forward_u8(yh_handle* h, const void* x, int batch, int height, int width, void* y, void* stream) {
    return forward(h, x, batch, height, width, y, stream, 1);
}

int yh_classify(yh_handle* h, const void* x, int x_u8, int batch, int height, int width, const int* count, float* probs,
                float* logits, float* embed, void* stream) {
    return guarded([&] {
        yh::require(h && x && probs, "null argument");
        yh::require(batch > 0, "batch must be positive");
        yh::require(h->net.task == 1, "yh_classify on a detection handle (made by yh_create): call yh_forward", YH_ESTATE);
        HIPCHECK(hipSetDevice(h->net.device));
        h->net.classify(x, x_u8 != 0, batch, height, width, count, probs, logits, embed, (hipStream_t)stream);
    });
}

// Launch units: unit i of a shape's plan is its i-th active op (one op per unit, never a level).
int yh_unit_count(const yh_handle* h, int batch, int height, int width) {
    if (!h) return YH_EINVAL;
    auto it = h->net.plans.find(yh::GraphKey{batch, height, width});
    if (it == h->net.plans.end()) return YH_ESTATE;
    return (int)it->second.order.size();
}

int yh_unit_info(const yh_handle* h, int index, int batch, int height, int width, int* first_op, int* num_ops,
                 int* is_level, double* ms_total, int* calls) {
    return guarded([&] {
        yh::require(h, "null handle");
        const yh::Net& n = h->net;
        auto it = n.plans.find(yh::GraphKey{batch, height, width});
        yh::require(it != n.plans.end(), "no forward has run at this shape yet", YH_ESTATE);
        const std::vector<int>& order = it->second.order;
        yh::require(index >= 0 && index < (int)order.size(), "unit index out of range");
        const bool prof_here = n.prof_key.B == batch && n.prof_key.H == height && n.prof_key.W == width;
        if (first_op) *first_op = order[index];
        if (num_ops) *num_ops = 1;
        if (is_level) *is_level = 0;
        if (ms_total) *ms_total = prof_here && index < (int)n.prof_ms.size() ? n.prof_ms[index] : 0.0;
        if (calls) *calls = prof_here && index < (int)n.prof_calls.size() ? n.prof_calls[index] : 0;
    });
}

int yh_set_graph(yh_handle* h, int enable) {
    return guarded([&] {
        yh::require(h, "null handle");
        h->net.use_graph = enable != 0;
    });
}

int yh_profile_enable(yh_handle* h, int enable) {
    return guarded([&] {
        yh::require(h, "null handle");
        h->net.profile = enable != 0;
    });
}

int yh_profile_reset(yh_handle* h) {
    return guarded([&] {
        yh::require(h, "null handle");
        std::fill(h->net.prof_ms.begin(), h->net.prof_ms.end(), 0.0);
        std::fill(h->net.prof_calls.begin(), h->net.prof_calls.end(), 0);
    });
}

int yh_force_conv_kernel(yh_handle* h, int kernel) {
    return guarded([&] {
        yh::require(h, "null handle");
        yh::require(kernel >= -1, "conv plan index out of range");
        h->net.force_kern = kernel;
        h->net.conv_kern.clear();
        h->net.cur_kern = nullptr;
        h->net.drop_graphs();
    });
}

int yh_debug_op_desc(const yh_handle* h, int index, int batch, int height, int width, char* buf, size_t size) {
    int len = 0;
    const int rc = guarded([&] {
        yh::require(h && index >= 0 && index < (int)h->net.ops.size(), "op index out of range");
        const std::string s = h->net.op_desc(index, batch, height, width);
        yh::require(buf && size > s.size(), "buffer too small");
        std::memcpy(buf, s.c_str(), s.size() + 1);
        len = (int)s.size();
    });
    return rc == YH_OK ? len : rc;
}

int yh_debug_run_ops(yh_handle* h, const void* x, int x_u8, int batch, int height, int width, void* y, int first,
                     int last, void* stream) {
    return guarded([&] {
        yh::require(h && x && y, "null argument");
        h->net.debug_run(x, x_u8, batch, height, width, y, first, last, (hipStream_t)stream);
    });
}

int yh_debug_operand(const yh_handle* h, int index, int slot, void* dst, size_t dst_bytes, void* stream) {
    return guarded([&] {
        yh::require(h && dst, "null argument");
        HIPCHECK(hipSetDevice(h->net.device));
        h->net.debug_operand(index, slot, dst, dst_bytes, (hipStream_t)stream);
    });
}

int yh_debug_silu_pairs(int dtype, const void* x, void* y_scalar, void* y_pair, size_t n) {
    return guarded([&] {
        yh::require(dtype == YH_F16 || dtype == YH_BF16, "yh_debug_silu_pairs: dtype must be YH_F16 or YH_BF16");
        yh::require(n == 0 || (x && y_scalar && y_pair), "null argument");
        HIPCHECK((hipError_t)yh::launch_silu_pairs(dtype, (const float*)x, (unsigned*)y_scalar, (unsigned*)y_pair, n,
                                                   nullptr));
    });
}

int yh_op_count(const yh_handle* h) { return h ? (int)h->net.ops.size() : YH_EINVAL; }

int yh_op_kernel(const yh_handle* h, int index, int batch, int height, int width, const char** name) {
    return guarded([&] {
        yh::require(h && index >= 0 && index < (int)h->net.ops.size(), "op index out of range");
        const yh::Net& n = h->net;
        const yh::Op& op = n.ops[index];
        if (op.kind != yh::OP_CONV) {
            if (name) *name = yh::op_kind_name(op.kind);
            auto cp = n.csp_plan.find({yh::GraphKey{batch, height, width}, index});
            if (name && cp != n.csp_plan.end()) *name = cp->second.c_str();
            return;
        }
        if (n.dtype == yh::F32) {
            if (name) *name = "gemm_f32";
            return;
        }
        auto it = n.conv_kern.find(yh::GraphKey{batch, height, width});
        yh::require(it != n.conv_kern.end(), "no forward has run at this shape yet", YH_ESTATE);
        if (name) *name = it->second[index].name.c_str();
    });
}

int yh_op_info(const yh_handle* h, int index, int batch, int height, int width, const char** label, int* op_class,
               double* bytes, double* flops, double* ms_total, int* calls) {
    return guarded([&] {
        yh::require(h && index >= 0 && index < (int)h->net.ops.size(), "op index out of range");
        const yh::Net& n = h->net;
        const yh::Op& op = n.ops[index];
        if (label) *label = op.label.c_str();
        if (op_class) *op_class = (int)n.op_class(op);
        double b = 0, f = 0;
        n.op_cost(op, batch, height, width, b, f);
        if (bytes) *bytes = b;
        if (flops) *flops = f;
        // profiled time of the op's own launch; 0 calls for ops inactive at this shape
        double ms = 0.0;
        int nc = 0;
        auto it = n.plans.find(yh::GraphKey{batch, height, width});
        const bool prof_here = n.prof_key.B == batch && n.prof_key.H == height && n.prof_key.W == width;
        if (it != n.plans.end() && prof_here) {
            const std::vector<int>& order = it->second.order;
            const size_t u = std::lower_bound(order.begin(), order.end(), index) - order.begin();
            if (u < order.size() && order[u] == index && u < n.prof_ms.size()) { ms = n.prof_ms[u]; nc = n.prof_calls[u]; }
        }
        if (ms_total) *ms_total = ms;
        if (calls) *calls = nc;
    });
}

}  // extern "C"
