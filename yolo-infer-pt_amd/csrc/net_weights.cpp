// Weight folding, upload and packed images: BatchNorm folded into the convs exactly like
// fuse_conv (nets/nn.py:8-25), the per-layer device copies, and the cached parameter images of
// the fused kernels.
#include <cstdio>

#include "net.h"

namespace yh {

static void* upload_bytes(const void* src, size_t bytes) {
    void* dev = nullptr;
    HIPCHECK(hipMalloc(&dev, bytes));
    HIPCHECK(hipMemcpy(dev, src, bytes, hipMemcpyHostToDevice));
    return dev;
}

void Net::load_conv(int idx, const float* w, const float* b, const float* g, const float* be, const float* mu,
                    const float* var_, double eps) {
    require(idx >= 0 && idx < (int)convs.size(), "conv index out of range");
    ConvDesc& d = convs[idx];
    const int cpg = d.cin / d.groups;
    const size_t per = (size_t)cpg * d.k * d.k;
    d.wf.assign(w, w + per * d.cout);
    d.bf.assign(d.cout, 0.0f);
    if (b) for (int o = 0; o < d.cout; ++o) d.bf[o] = b[o];
    if (g) {
        // fuse_conv (nets/nn.py:8-25), fp32 throughout:
        //   s = gamma / sqrt(eps + var); W' = s * W; b' = s * b + (beta - gamma*mean / sqrt(var + eps))
        const float epsf = (float)eps;
        for (int o = 0; o < d.cout; ++o) {
            const float den = std::sqrt(var_[o] + epsf);
            const float s = g[o] / den;
            for (size_t i = 0; i < per; ++i) d.wf[o * per + i] = s * d.wf[o * per + i];
            const float bnorm = be[o] - (g[o] * mu[o]) / den;
            d.bf[o] = s * d.bf[o] + bnorm;
        }
    }
    upload(d);
    d.loaded = true;
}

void Net::upload(ConvDesc& d) {
    free_conv(d);
    std::vector<float> bias(d.coutp_pad, 0.0f);
    for (int o = 0; o < d.cout; ++o) bias[o] = d.bf[o];
    d.b_dev = (float*)upload_bytes(bias.data(), bias.size() * 4);
    if (d.kind == CK_DENSE) {
        // packed [coutp_pad][Kp], k = (kh*KW + kw)*cin_p + ci_phys
        std::vector<float> wp((size_t)d.coutp_pad * d.Kp, 0.0f);
        std::vector<int> ktab(d.Kp / 8, 0xffff);
        // physical -> logical channel map
        std::vector<int> phys2log(d.cin_p, -1);
        int lo = 0, ph = 0;
        for (auto& s : d.segs) {
            for (int c = 0; c < s.first; ++c) phys2log[ph + c] = lo + c;
            lo += s.first;
            ph += s.second;
        }
        d.phys2log = phys2log;
        const size_t per = (size_t)d.cin * d.k * d.k;
        for (int kh = 0; kh < d.k; ++kh)
            for (int kw = 0; kw < d.k; ++kw)
                for (int cp = 0; cp < d.cin_p; ++cp) {
                    const int kk = (kh * d.k + kw) * d.cin_p + cp;
                    if (cp % 8 == 0) ktab[kk / 8] = (kh << 24) | (kw << 16) | cp;
                    const int cl = phys2log[cp];
                    if (cl < 0) continue;
                    for (int o = 0; o < d.cout; ++o)
                        wp[(size_t)o * d.Kp + kk] = d.wf[o * per + (size_t)cl * d.k * d.k + kh * d.k + kw];
                }
        d.w_dev = to_device(wp);
        if (d.k == 1 && dtype != F32 && d.Kp % 16 == 0) {
            // the same 16-bit weights in MFMA A-fragment order for pw_chain: fragment (a, kb) =
            // couts 32a .. 32a + 31 x k 16kb .. 16kb + 15 as 64 lanes x 16 B (lane l: cout 32a +
            // (l & 31), k 16kb + 8 (l >> 5) .. + 7), one contiguous KB, so a wave's fragment load
            // is one coalesced KB instead of 32 strided rows
            const int na = (d.cout + 31) / 32, nkb = d.Kp / 16;
            std::vector<float> fr((size_t)na * 32 * d.Kp, 0.0f);
            for (int a = 0; a < na; ++a)
                for (int kb = 0; kb < nkb; ++kb)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            const int o = a * 32 + (l & 31), k = kb * 16 + 8 * (l >> 5) + e;
                            fr[(((size_t)a * nkb + kb) * 64 + l) * 8 + e] = o < d.coutp_pad ? wp[(size_t)o * d.Kp + k] : 0.0f;
                        }
            d.mx_w["pwfrag"] = to_device(fr);
        }
        d.ktab_dev = (int*)upload_bytes(ktab.data(), ktab.size() * 4);
    } else if (d.kind == CK_FIRST) {
        // transposed [27][cout_p]: k = ci*9 + kh*3 + kw
        std::vector<float> wp((size_t)d.cout_p * 27, 0.0f);
        for (int o = 0; o < d.cout; ++o)
            for (int k = 0; k < 27; ++k) wp[(size_t)k * d.cout_p + o] = d.wf[(size_t)o * 27 + k];
        d.w_dev = upload_bytes(wp.data(), wp.size() * 4);
    } else {  // depthwise / pe: [9][C] fp32
        std::vector<float> wp((size_t)9 * d.cout_p, 0.0f);
        for (int c = 0; c < d.cout; ++c)
            for (int t = 0; t < 9; ++t) wp[(size_t)t * d.cout_p + c] = d.wf[(size_t)c * 9 + t];
        d.w_dev = upload_bytes(wp.data(), wp.size() * 4);
    }
}

// v on the device in the handle dtype
void* Net::to_device(const std::vector<float>& v) const {
    if (dtype == F32) return upload_bytes(v.data(), v.size() * 4);
    std::vector<uint16_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = to16(v[i]);
    return upload_bytes(h.data(), h.size() * 2);
}

void Net::free_conv(ConvDesc& d) {
    for (auto& kv : d.mx_w) (void)hipFree(kv.second);
    d.mx_w.clear();
    if (d.w_dev) (void)hipFree(d.w_dev);
    if (d.b_dev) (void)hipFree(d.b_dev);
    if (d.ktab_dev) (void)hipFree(d.ktab_dev);
    d.w_dev = nullptr;
    d.b_dev = nullptr;
    d.ktab_dev = nullptr;
}

// packed weights of conv `ci` in the layout of plan `p` (cached per layout)
const char* Net::mx_weights(int ci, const MxPlan& p, const MxShape& sh) {
    ConvDesc& d = convs[ci];
    char k[96];
    snprintf(k, sizeof(k), "%d/%d/%d/%d/%d/%d/%d/%d", p.cfg.kind, p.cfg.ks, p.cfg.na, p.cfg.wn, p.cfg.ncb, p.nst,
             p.nslices, p.wstage);
    auto it = d.mx_w.find(k);
    if (it != d.mx_w.end()) return (const char*)it->second;
    require(d.loaded, "weights of " + d.name + " not loaded", YH_ESTATE);
    const std::vector<uint16_t> pk = mx_pack(p, sh, d.wf.data(), d.cin, d.phys2log, dtype == BF16, d.cout);
    return (const char*)d.mx_w.emplace(k, upload_bytes(pk.data(), pk.size() * 2)).first->second;
}

// ---------------------------------------------------------- parameter images of the fused ops
// The image of a fused op that computes several convs, cached under `key` in the owner conv's
// mx_w; every other member conv holds a marker under key_dep. A reload of any member clears
// that conv's mx_w (free_conv), so the image or a marker is missing at the next launch: the old
// device block is freed and the image built again from the members' folded weights.
const void* Net::fused_params(int owner, const std::string& key, const std::vector<int>& others,
                              const std::function<std::vector<uint8_t>()>& image) {
    ConvDesc& d0 = convs[owner];
    const std::string dep = key + "_dep";
    auto it = d0.mx_w.find(key);
    bool ok = it != d0.mx_w.end();
    for (int c : others) ok = ok && convs[c].mx_w.count(dep);
    if (ok) return it->second;
    if (it != d0.mx_w.end()) {
        (void)hipFree(it->second);
        d0.mx_w.erase(it);
    }
    require(d0.loaded, "weights of " + d0.name + " not loaded", YH_ESTATE);
    for (int c : others) require(convs[c].loaded, "weights of " + convs[c].name + " not loaded", YH_ESTATE);
    const std::vector<uint8_t> img = image();
    void* dev = upload_bytes(img.data(), img.size());
    d0.mx_w.emplace(key, dev);
    for (int c : others) convs[c].mx_w.emplace(dep, nullptr);
    return dev;
}

// row of a 32-cout MFMA A tile held by lane R (0..31 within a lane half): conv_mx's order (lane
// half hh of the k-step holds K values 8hh + j; accumulator rows come out as couts 16hh ..), or
// the same with bits 2 and 3 of the row swapped (rho: a conv whose accumulators become the next
// 1x1 conv's B fragments)
enum RowOrder { ROWS_MX, ROWS_RHO };
static int frag_row(int R, RowOrder ro) {
    return ro == ROWS_RHO ? ((R & 0x13) | ((R & 4) << 1) | ((R & 8) >> 1)) : 16 * ((R >> 2) & 1) + (R & 3) + 4 * (R >> 3);
}
// A fragments of conv d at dst: fragment (tile a, step k, lane, j) = cout 32a + frag_row(lane & 31),
// K value 8 (lane >> 5) + j of step k = (16-channel block cb, tap); zero beyond cout / cin
static void pack_frags(const Net& n, uint8_t* dst8, const ConvDesc& d, int ntile, int nk, RowOrder ro = ROWS_MX) {
    const int kk2 = d.k * d.k;
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst8);
    for (int a = 0; a < ntile; ++a)
        for (int k = 0; k < nk; ++k)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int co = 32 * a + frag_row(lane & 31, ro);
                    const int cb = k / kk2, tap = k - cb * kk2, ch = 16 * cb + 8 * (lane >> 5) + j;
                    float v = 0.f;
                    if (co < d.cout && ch < d.cin) v = d.wf[((size_t)co * d.cin + ch) * kk2 + tap];
                    dst[((size_t)(a * nk + k) * 64 + lane) * 8 + j] = n.to16(v);
                }
}
static void put_bias(uint8_t* dst, const ConvDesc& d) { std::memcpy(dst, d.bf.data(), (size_t)d.cout * 4); }

// packed p2.0 parameters of the fused stem: fragments (tile a, step k = cb*9 + tap), then the
// fp32 bias and the stem's own fragments (tile i, lane (fr, g), j): cout 16 i + fr, k = 8 g + j
// of its 27 taps in conv_first_tile's order, zero for the K padding (cached with p2.0)
const void* Net::stem2_params(const Op& op, int& bias_off, int& stem_off) {
    const ConvDesc &d = convs[op.cs[0]], &d1 = convs[op.conv];
    const int nt = d.cout / 32, nk = 9 * (d.cin / 16);
    bias_off = nt * nk * 1024;
    stem_off = bias_off + d.cout * 4;
    return fused_params(op.cs[0], "stem2", {op.conv}, [&] {
        std::vector<uint8_t> img((size_t)stem_off + (size_t)(d1.cout / 16) * 1024, 0);
        uint16_t* sd = reinterpret_cast<uint16_t*>(img.data() + stem_off);
        for (int i = 0; i < d1.cout / 16; ++i)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = 8 * (lane >> 4) + j;
                    sd[((size_t)i * 64 + lane) * 8 + j] = to16(k < 27 ? d1.wf[(size_t)(16 * i + (lane & 15)) * 27 + k] : 0.0f);
                }
        pack_frags(*this, img.data(), d, nt, nk);
        put_bias(img.data() + bias_off, d);
        return img;
    });
}
// packed parameter image of a fused C3k2 op (c3k2.hip csp_offsets), cached with conv1; tail mode
// (no conv1 in the op): with the Residual's first conv
const void* Net::csp_params(const Op& op) {
    const int k0 = op.cs[0] >= 0 ? 0 : 1;
    return fused_params(op.cs[k0], "csp", std::vector<int>(op.cs + k0 + 1, op.cs + 4), [&] {
        const ConvDesc &r1 = convs[op.cs[1]], &r2 = convs[op.cs[2]], &c2 = convs[op.cs[3]];
        const int ni = k0 == 0 ? convs[op.cs[0]].cin / 16 : 0, nc = r1.cin / 16, no = c2.cout / 32, nh = (nc + 1) / 2;
        int off[9];
        csp_offsets(ni, nc, no, off);
        std::vector<uint8_t> img((size_t)off[8], 0);
        if (ni) pack_frags(*this, img.data() + off[0], convs[op.cs[0]], nc, ni);
        pack_frags(*this, img.data() + off[1], r1, 1, 9 * nc);
        pack_frags(*this, img.data() + off[2], r2, nh, 9 * nh);
        pack_frags(*this, img.data() + off[3], c2, no, 3 * nc);
        if (ni) put_bias(img.data() + off[4], convs[op.cs[0]]);
        put_bias(img.data() + off[5], r1);
        put_bias(img.data() + off[6], r2);
        put_bias(img.data() + off[7], c2);
        return img;
    });
}
// packed parameters of a fused C3k block (c3k.hip c3k_offsets), cached with its first conv
const void* Net::c3k_params(const Op& op) {
    return fused_params(op.ck[0], "c3k", std::vector<int>(op.ck + 1, op.ck + 7), [&] {
        // hidden channels hh = conv1's couts (32 or 64): NT3 = hh / 32 tiles of conv1 / conv2 /
        // the 3x3 convs over hh / 8 (1x1) or 9 hh / 16 (3x3) K steps, conv3: hh / 16 tiles
        const int hh = convs[op.ck[0]].cout, nt3 = hh / 32, nk1 = hh / 8, nk3 = 9 * hh / 16;
        int off[9];
        c3k_offsets(hh, off);
        std::vector<uint8_t> img((size_t)off[8], 0);
        pack_frags(*this, img.data() + off[0], convs[op.ck[0]], nt3, nk1);
        pack_frags(*this, img.data() + off[1], convs[op.ck[1]], nt3, nk1, ROWS_RHO);   // conv3's B fragments
        for (int r = 0; r < 4; ++r) pack_frags(*this, img.data() + off[2] + r * nt3 * nk3 * 1024, convs[op.ck[2 + r]], nt3, nk3);
        pack_frags(*this, img.data() + off[3], convs[op.ck[6]], hh / 16, nk1);
        put_bias(img.data() + off[4], convs[op.ck[0]]);
        put_bias(img.data() + off[5], convs[op.ck[1]]);
        for (int r = 0; r < 4; ++r) put_bias(img.data() + off[6] + r * hh * 4, convs[op.ck[2 + r]]);
        put_bias(img.data() + off[7], convs[op.ck[6]]);
        return img;
    });
}

}  // namespace yh
