// ops.cpp — single-layer entry points of the C ABI (anh_op_*): one conv / cont forward, backward-data or
// backward-filter on host tensors, through the same kernel choice the net uses.  They exist so that each kernel can be
// checked against the oracle with IDENTICAL inputs (whole-net bf16 gradients decorrelate at the one-ulp level), and for
// per-kernel micro-benchmarks.
//
// The second half of the file holds the forms the bf16 training step runs by default and the conv entry points above never reach —
// the batch-norm accumulator tables (bnacc.h) — and the training kernels that are not convolutions:
//   anh_op_bn_fold                        bn_fold_all over up to 16 tables built on the host from given sums
//   anh_op_bn_forward_stats               the partials form of the same arrays (statistics kernel + finalize)
//   anh_op_conv_forward_stats_table       forward conv adding its statistics into a table (ConvArgs::stat_acc), inputs optionally in
//                                         table form (Src::a_tab / b_tab), the stem's image source included
//   anh_op_conv_backward_data_bn_table    backward-data conv with ConvArgs::bnred_acc / bnred_finish
//   anh_op_bn_backward                    bn_bwd_reduce* / bn_bwd_finalize / bn_bwd_apply* (scalar, vector, head form), partials or table
//   anh_op_head_train                     head_train_kernel + head_finalize in every form of its arguments
//   anh_op_loss                           loss_kernel + loss_finalize
// Tables are written and decoded on the host (bnacc_spread_host / bnacc_total_host), never with bnacc_add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bnacc.h"
#include "common.h"
#include "kernels.h"
#include "spec.h"

using namespace anh;

namespace {
inline uint16_t to_bf16_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float from_bf16_bits(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

// the stream of one entry point: synchronised before it is destroyed, also when an error unwinds past launched work
struct OpStream {
    Stream own;
    hipStream_t s = nullptr;
    OpStream() { own.create(hipStreamNonBlocking); s = own.get(); }
    ~OpStream() { (void)hipStreamSynchronize(s); }
};

// host fp32 -> device tensor in the mode's storage type
void upload(DevBuf& d, const float* host, size_t count, DType dt) {
    if (dt == DT_F32) {
        d.reserve(std::max<size_t>(count, 1) * 4);
        HIP_CHECK(hipMemcpy(d.p, host, count * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> tmp(count);
        for (size_t i = 0; i < count; ++i) tmp[i] = to_bf16_bits(host[i]);
        d.reserve(std::max<size_t>(count, 1) * 2);
        HIP_CHECK(hipMemcpy(d.p, tmp.data(), count * 2, hipMemcpyHostToDevice));
    }
}
void upload_f32(DevBuf& d, const float* host, size_t count) { upload(d, host, count, DT_F32); }

void download(const DevBuf& d, float* host, size_t count, DType dt) {
    if (dt == DT_F32) HIP_CHECK(hipMemcpy(host, d.p, count * 4, hipMemcpyDeviceToHost));
    else {
        std::vector<uint16_t> tmp(count);
        HIP_CHECK(hipMemcpy(tmp.data(), d.p, count * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < count; ++i) host[i] = from_bf16_bits(tmp[i]);
    }
}

struct Filters {
    DevBuf tm_f32, km_f32, tm_bf16, km_bf16;
};
// canonical -> [tap][ci][co] and [tap][co][ci]; in bf16 mode the fp32 copies carry the rounded values (as the engine's do)
void upload_filters(Filters& f, const anh_conv_desc& d, const float* canon, DType dt) {
    const int kk = d.k * d.k;
    const size_t nw = (size_t)kk * d.cin * d.cout;
    std::vector<float> tm(nw), km(nw);
    std::vector<uint16_t> tmb(nw), kmb(nw);
    for (int t = 0; t < kk; ++t)
        for (int ci = 0; ci < d.cin; ++ci)
            for (int co = 0; co < d.cout; ++co) {
                const size_t src = d.type == 0 ? ((size_t)co * d.cin + ci) * kk + t : ((size_t)ci * d.cout + co) * kk + t;
                float w = canon[src];
                const uint16_t b = to_bf16_bits(w);
                if (dt == DT_BF16) w = from_bf16_bits(b);
                const size_t i_tm = ((size_t)t * d.cin + ci) * d.cout + co, i_km = ((size_t)t * d.cout + co) * d.cin + ci;
                tm[i_tm] = w; km[i_km] = w; tmb[i_tm] = b; kmb[i_km] = b;
            }
    upload_f32(f.tm_f32, tm.data(), nw);
    upload_f32(f.km_f32, km.data(), nw);
    if (dt == DT_BF16) {
        f.tm_bf16.reserve(nw * 2); f.km_bf16.reserve(nw * 2);
        HIP_CHECK(hipMemcpy(f.tm_bf16.p, tmb.data(), nw * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(f.km_bf16.p, kmb.data(), nw * 2, hipMemcpyHostToDevice));
    }
}

struct OpSource {
    DevBuf xa, xb, sa, ta, sb, tb;
    Src src;
};
void make_source(OpSource& o, const anh_op_input* a, const anh_op_input* b, size_t elems, int c, DType dt) {
    ANH_REQUIRE(a && a->x, "null input tensor");
    ANH_REQUIRE(!b || (b->x && a->scale && b->scale), "a skip input needs both inputs to carry scale/shift");
    upload(o.xa, a->x, elems, dt);
    o.src.dtype = dt;
    o.src.a = o.xa.p;
    o.src.kind = SRC_RAW;
    if (a->scale) {
        ANH_REQUIRE(a->shift, "scale without shift");
        upload_f32(o.sa, a->scale, c); upload_f32(o.ta, a->shift, c);
        o.src.a_scale = o.sa.as<float>(); o.src.a_shift = o.ta.as<float>();
        o.src.kind = SRC_ACT;
    }
    if (b) {
        ANH_REQUIRE(b->shift, "scale without shift");
        upload(o.xb, b->x, elems, dt);
        upload_f32(o.sb, b->scale, c); upload_f32(o.tb, b->shift, c);
        o.src.b = o.xb.p; o.src.b_scale = o.sb.as<float>(); o.src.b_shift = o.tb.as<float>();
        o.src.kind = SRC_ACT2;
    }
}

void check_desc(const anh_conv_desc* d, int n, int h, int w) {
    ANH_REQUIRE(d, "null descriptor");
    ANH_REQUIRE((d->type == 0 || d->type == 1) && d->k >= 1 && d->k <= 7 && d->stride >= 1 && d->stride <= 4 && d->pad >= 0 && d->cin >= 1 && d->cout >= 1,
                "bad conv descriptor");
    ANH_REQUIRE(n >= 1 && h >= 1 && w >= 1, "empty tensor");
}
int out_dim(const anh_conv_desc& d, int in) {
    anh_layer_desc L{};
    L.type = d.type; L.k = d.k; L.stride = d.stride; L.pad = d.pad;
    return Spec::out_dim(L, in);
}

// ---- helpers of the table-mode and training-kernel entry points ----
void fill_nan(DevBuf& d, size_t count) {   // an output no kernel wrote must not compare equal to anything
    std::vector<float> v(std::max<size_t>(count, 1), std::numeric_limits<float>::quiet_NaN());
    upload_f32(d, v.data(), v.size());
}
void fetch_f32(const DevBuf& d, float* host, size_t count) { if (host) HIP_CHECK(hipMemcpy(host, d.p, count * 4, hipMemcpyDeviceToHost)); }

// a bn accumulator table on the host and on the device
struct Table {
    std::vector<long long> host;
    DevBuf dev;
    int c = 0;
    void zero(int channels) { c = channels; host.assign(bnacc_words(c), 0); }
    // sums[c][2] -> the two sums first_which, first_which + 1 of every channel, spread over all replicas
    void add_sums(const double* sums, int first_which, unsigned long long& state) {
        for (int ch = 0; ch < c; ++ch)
            for (int w = 0; w < 2; ++w) {
                long long hi, lo;
                ANH_REQUIRE(bnacc_split_host(sums[ch * 2 + w], hi, lo), "a sum is not a multiple of 2^-60 below 3e16");
                bnacc_spread_host(host.data(), first_which + w, c, ch, hi, lo, state);
            }
    }
    void upload() {
        dev.reserve(host.size() * sizeof(long long));
        HIP_CHECK(hipMemcpy(dev.p, host.data(), host.size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    void download() { HIP_CHECK(hipMemcpy(host.data(), dev.p, host.size() * sizeof(long long), hipMemcpyDeviceToHost)); }
    void totals(int first_which, double* sums) const {
        for (int ch = 0; ch < c; ++ch)
            for (int w = 0; w < 2; ++w) sums[ch * 2 + w] = bnacc_total_host(host.data(), first_which + w, c, ch);
    }
    long long poison() const { return host[bnacc_poison_index(c)]; }
    long long ticket() const { return host[bnacc_poison_index(c) + 1]; }
    long long* acc() const { return dev.as<long long>(); }
};

// the device side of one anh_op_bn_layer
struct LayerDev {
    DevBuf gamma, beta, mean, invstd, scale, shift, var, rmean, rvar;
    void prepare(const anh_op_bn_layer& L) {
        ANH_REQUIRE(L.c >= 1 && L.pixels >= 1 && L.gamma && L.beta && L.mean && L.invstd && L.scale && L.shift && L.var, "bad bn layer");
        ANH_REQUIRE((L.running_mean == nullptr) == (L.running_var == nullptr), "running statistics come as a pair");
        upload_f32(gamma, L.gamma, L.c); upload_f32(beta, L.beta, L.c);
        fill_nan(mean, L.c); fill_nan(invstd, L.c); fill_nan(scale, L.c); fill_nan(shift, L.c); fill_nan(var, (size_t)2 * L.c);
        if (L.running_mean) { upload_f32(rmean, L.running_mean, L.c); upload_f32(rvar, L.running_var, L.c); }
    }
    BnFoldJob job(const anh_op_bn_layer& L, const long long* acc) const {
        BnFoldJob j;
        j.acc = acc; j.gamma = gamma.as<float>(); j.beta = beta.as<float>();
        j.mean = mean.as<float>(); j.invstd = invstd.as<float>(); j.scale = scale.as<float>(); j.shift = shift.as<float>(); j.var = var.as<double>();
        j.rmean = L.running_mean ? rmean.as<float>() : nullptr; j.rvar = L.running_mean ? rvar.as<float>() : nullptr;
        j.pixels = L.pixels; j.af = L.af; j.unbias = L.unbias; j.eps = L.eps; j.c = L.c;
        return j;
    }
    void fetch(anh_op_bn_layer& L) const {
        fetch_f32(mean, L.mean, L.c); fetch_f32(invstd, L.invstd, L.c); fetch_f32(scale, L.scale, L.c); fetch_f32(shift, L.shift, L.c);
        HIP_CHECK(hipMemcpy(L.var, var.p, (size_t)L.c * sizeof(double), hipMemcpyDeviceToHost));
        if (L.running_mean) { fetch_f32(rmean, L.running_mean, L.c); fetch_f32(rvar, L.running_var, L.c); }
    }
};

// one side of a table-mode consumer's input (anh_op_bn_input)
struct BnSide {
    DevBuf x, scale, shift, gamma, beta;
    Table tab;
    BnTable bn;
    void make(const anh_op_bn_input& in, size_t elems, int c, DType dt, unsigned long long& state) {
        ANH_REQUIRE(in.x, "null input tensor");
        upload(x, in.x, elems, dt);
        if (in.sums) {   // table form: the arrays exist (as in the engine) but hold NaN — a kernel that read them would show
            ANH_REQUIRE(in.gamma && in.beta, "a table-form input needs gamma and beta");
            fill_nan(scale, c); fill_nan(shift, c);
            upload_f32(gamma, in.gamma, c); upload_f32(beta, in.beta, c);
            tab.zero(c); tab.add_sums(in.sums, BNACC_SUM_Y, state); tab.upload();
            bn.acc = tab.acc(); bn.gamma = gamma.as<float>(); bn.beta = beta.as<float>(); bn.pixels = (double)(elems / c); bn.eps = in.eps; bn.c = c;
        } else {
            ANH_REQUIRE(in.scale && in.shift, "an input needs scale and shift, or sums");
            upload_f32(scale, in.scale, c); upload_f32(shift, in.shift, c);
        }
    }
};
struct BnSource {
    BnSide a, b;
    Src src;
    void make(const anh_op_bn_input* ia, const anh_op_bn_input* ib, size_t elems, int c, DType dt, unsigned long long& state) {
        ANH_REQUIRE(ia, "null input");
        ANH_REQUIRE(!ib || ((ia->sums == nullptr) == (ib->sums == nullptr)), "both inputs take the same form");
        a.make(*ia, elems, c, dt, state);
        src.dtype = dt; src.kind = SRC_ACT;
        src.a = a.x.p; src.a_scale = a.scale.as<float>(); src.a_shift = a.shift.as<float>(); src.a_tab = a.bn;
        if (ib) {
            b.make(*ib, elems, c, dt, state);
            src.kind = SRC_ACT2;
            src.b = b.x.p; src.b_scale = b.scale.as<float>(); src.b_shift = b.shift.as<float>(); src.b_tab = b.bn;
        }
    }
};

void sum_partials(const DevBuf& partials, int blocks, int c, double* sums) {   // [channel][2][blocks] -> sums[c][2]
    std::vector<double> p((size_t)blocks * 2 * c);
    HIP_CHECK(hipMemcpy(p.data(), partials.p, p.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int ch = 0; ch < c; ++ch)
        for (int which = 0; which < 2; ++which) {
            double s = 0;
            for (int k = 0; k < blocks; ++k) s += p[((size_t)ch * 2 + which) * blocks + k];
            sums[ch * 2 + which] = s;
        }
}
}  // namespace

extern "C" {

int anh_op_conv_forward(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                        const float* filters, const float* bias, float* y, int* used_mfma) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(filters && y, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        OpSource in;
        make_source(in, a, b, (size_t)n * h_in * w_in * d->cin, d->cin, dt);
        Filters f;
        upload_filters(f, *d, filters, dt);
        DevBuf dbias, out;
        if (bias) upload_f32(dbias, bias, d->cout);
        const DType out_dt = bias ? DT_F32 : dt;  // biased (head) outputs are fp32 logits
        const size_t out_elems = (size_t)n * h_out * w_out * d->cout;
        out.reserve(out_elems * (out_dt == DT_BF16 ? 2 : 4));
        ConvArgs c;
        c.src = in.src;
        c.n = n; c.h_in = h_in; c.w_in = w_in; c.c_red = d->cin; c.h_out = h_out; c.w_out = w_out; c.c_out = d->cout;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = d->type;
        c.w_f32 = f.tm_f32.as<float>(); c.w_bf16 = f.km_bf16.p;
        c.bias = bias ? dbias.as<float>() : nullptr;
        c.out = out.p; c.out_dtype = out_dt;
        const bool fast = conv_takes_mfma(c, dt);
        if (fast) launch_conv_mfma(c, st.s); else launch_conv_generic(c, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, y, out_elems, out_dt);
        if (used_mfma) *used_mfma = fast ? 1 : 0;
    });
}

int anh_op_conv_backward_data(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy, const float* filters,
                              float* dx, int* used_mfma) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(dy && filters && dx, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        DevBuf g, out;
        upload(g, dy, (size_t)n * h_out * w_out * d->cout, dt);
        Filters f;
        upload_filters(f, *d, filters, dt);
        const size_t out_elems = (size_t)n * h_in * w_in * d->cin;
        out.reserve(out_elems * (dt == DT_BF16 ? 2 : 4));
        ConvArgs c;
        c.src.kind = SRC_RAW; c.src.dtype = dt; c.src.a = g.p;
        c.n = n; c.h_in = h_out; c.w_in = w_out; c.c_red = d->cout; c.h_out = h_in; c.w_out = w_in; c.c_out = d->cin;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = 1 - d->type;
        c.w_f32 = f.km_f32.as<float>(); c.w_bf16 = f.tm_bf16.p;
        c.out = out.p; c.out_dtype = dt;
        const bool fast = conv_takes_mfma(c, dt);
        if (fast) launch_conv_mfma(c, st.s); else launch_conv_generic(c, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, dx, out_elems, dt);
        if (used_mfma) *used_mfma = fast ? 1 : 0;
    });
}

int anh_op_conv_backward_filter(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                                const float* dy, float* dw, int* used_mfma) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(dy && dw, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        OpSource in;
        make_source(in, a, b, (size_t)n * h_in * w_in * d->cin, d->cin, dt);
        DevBuf g, out, scratch;
        upload(g, dy, (size_t)n * h_out * w_out * d->cout, dt);
        const int kk = d->k * d->k;
        const size_t nw = (size_t)kk * d->cin * d->cout;
        out.reserve(nw * 4);
        WgradArgs w;
        w.src = in.src; w.dy = g.p; w.dy_dtype = dt;
        w.n = n; w.h_in = h_in; w.w_in = w_in; w.c_in = d->cin; w.h_out = h_out; w.w_out = w_out; w.c_out = d->cout;
        w.k = d->k; w.stride = d->stride; w.pad = d->pad; w.gather = d->type;
        w.dw = out.as<float>();
        const bool fast = wgrad_takes_mfma(w, dt);
        const int64_t need = fast ? wgrad_mfma_scratch_floats(w) : wgrad_generic_scratch_floats(w);
        scratch.reserve((size_t)std::max<int64_t>(need, 1) * 4);
        w.partials = scratch.as<float>(); w.partials_capacity = (int64_t)(scratch.bytes / 4);
        if (fast) launch_wgrad_mfma(w, st.s); else launch_wgrad_generic(w, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        std::vector<float> tm(nw);
        HIP_CHECK(hipMemcpy(tm.data(), out.p, nw * 4, hipMemcpyDeviceToHost));
        for (int t = 0; t < kk; ++t)
            for (int ci = 0; ci < d->cin; ++ci)
                for (int co = 0; co < d->cout; ++co) {
                    const size_t dst = d->type == 0 ? ((size_t)co * d->cin + ci) * kk + t : ((size_t)ci * d->cout + co) * kk + t;
                    dw[dst] = tm[((size_t)t * d->cin + ci) * d->cout + co];
                }
        if (used_mfma) *used_mfma = fast ? 1 : 0;
    });
}

// ---- the fused forms (see include/annonet_hip.h) ----
int anh_op_conv_forward_stats(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                              const float* filters, float* y, double* sums, int* fused) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(filters && y && sums, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        OpSource in;
        make_source(in, a, b, (size_t)n * h_in * w_in * d->cin, d->cin, dt);
        Filters f;
        upload_filters(f, *d, filters, dt);
        DevBuf out, partials, stat;
        const size_t out_elems = (size_t)n * h_out * w_out * d->cout;
        const int64_t pixels = (int64_t)n * h_out * w_out;
        out.reserve(out_elems * (dt == DT_BF16 ? 2 : 4));
        ConvArgs c;
        c.src = in.src;
        c.n = n; c.h_in = h_in; c.w_in = w_in; c.c_red = d->cin; c.h_out = h_out; c.w_out = w_out; c.c_out = d->cout;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = d->type;
        c.w_f32 = f.tm_f32.as<float>(); c.w_bf16 = f.km_bf16.p;
        c.out = out.p; c.out_dtype = dt;
        const bool fast = conv_takes_mfma(c, dt);
        int blocks = fast ? conv_fused_stat_blocks(c) : 0;
        const int fused_here = blocks > 0;
        partials.reserve((size_t)std::max(blocks, std::max(bn_partial_blocks(pixels), 1)) * 2 * d->cout * sizeof(double));
        if (fused_here) c.stat_partials = partials.as<double>();
        if (fast) launch_conv_mfma(c, st.s); else launch_conv_generic(c, st.s);
        if (!fused_here) {
            BnFwdArgs bn;
            bn.y = out.p; bn.dtype = dt; bn.pixels = pixels; bn.c = d->cout; bn.partials = partials.as<double>();
            blocks = launch_bn_forward_partials(bn, st.s);
        }
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, y, out_elems, dt);
        sum_partials(partials, blocks, d->cout, sums);
        if (fused) *fused = fused_here;
    });
}

int anh_op_conv_backward_data_bn(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy, const float* filters,
                                 const float* dx_init, const float* y_prev, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, float* dx, double* sums, int* fused) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(dy && filters && dx && y_prev && scale && shift && mean && invstd && sums, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        DevBuf g, out, yp, sc, sf, mn, is, partials, coef;
        upload(g, dy, (size_t)n * h_out * w_out * d->cout, dt);
        Filters f;
        upload_filters(f, *d, filters, dt);
        const size_t out_elems = (size_t)n * h_in * w_in * d->cin;
        const int64_t pixels = (int64_t)n * h_in * w_in;
        if (dx_init) upload(out, dx_init, out_elems, dt); else out.reserve(out_elems * (dt == DT_BF16 ? 2 : 4));
        upload(yp, y_prev, out_elems, dt);
        upload_f32(sc, scale, d->cin); upload_f32(sf, shift, d->cin); upload_f32(mn, mean, d->cin); upload_f32(is, invstd, d->cin);
        ConvArgs c;
        c.src.kind = SRC_RAW; c.src.dtype = dt; c.src.a = g.p;
        c.n = n; c.h_in = h_out; c.w_in = w_out; c.c_red = d->cout; c.h_out = h_in; c.w_out = w_in; c.c_out = d->cin;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = 1 - d->type;
        c.w_f32 = f.km_f32.as<float>(); c.w_bf16 = f.tm_bf16.p;
        c.out = out.p; c.out_dtype = dt; c.out_accumulate = dx_init ? 1 : 0;
        const bool fast = conv_takes_mfma(c, dt);
        int blocks = fast ? conv_fused_bnred_blocks(c) : 0;
        const int fused_here = blocks > 0;
        partials.reserve((size_t)std::max(blocks, std::max(bn_partial_blocks(pixels), 1)) * 2 * d->cin * sizeof(double));
        if (fused_here) {
            c.bnred_y = yp.p; c.bnred_scale = sc.as<float>(); c.bnred_shift = sf.as<float>(); c.bnred_mean = mn.as<float>(); c.bnred_invstd = is.as<float>();
            c.bnred_partials = partials.as<double>();
        }
        if (fast) launch_conv_mfma(c, st.s); else launch_conv_generic(c, st.s);
        if (!fused_here) {
            BnBwdArgs bn;
            bn.da = out.p; bn.y = yp.p; bn.dtype = dt; bn.pixels = pixels; bn.c = d->cin;
            bn.mean = mn.as<float>(); bn.invstd = is.as<float>(); bn.scale = sc.as<float>(); bn.shift = sf.as<float>();
            bn.partials = partials.as<double>();
            launch_bn_bwd_reduce(bn, st.s);
            blocks = bn_partial_blocks(pixels);
        }
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, dx, out_elems, dt);
        sum_partials(partials, blocks, d->cin, sums);
        if (fused) *fused = fused_here;
    });
}

int anh_op_conv_backward_filter_bn(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const uint8_t* image,
                                   const anh_op_bn_dy* dy, float* dw, int* computed_in_kernel) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(image && dy && dy->da && dy->y && dy->scale && dy->shift && dy->mean && dy->invstd && dy->coef && dw, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        DevBuf img, da, yy, sc, sf, mn, is, cf, out, scratch;
        const size_t img_bytes = (size_t)n * h_in * w_in * d->cin;
        img.reserve(img_bytes);
        HIP_CHECK(hipMemcpy(img.p, image, img_bytes, hipMemcpyHostToDevice));
        const size_t g_elems = (size_t)n * h_out * w_out * d->cout;
        upload(da, dy->da, g_elems, dt); upload(yy, dy->y, g_elems, dt);
        upload_f32(sc, dy->scale, d->cout); upload_f32(sf, dy->shift, d->cout); upload_f32(mn, dy->mean, d->cout);
        upload_f32(is, dy->invstd, d->cout); upload_f32(cf, dy->coef, (size_t)3 * d->cout);
        const int kk = d->k * d->k;
        const size_t nw = (size_t)kk * d->cin * d->cout;
        out.reserve(nw * 4);
        WgradArgs w;
        w.src = image_source(img.as<uint8_t>(), h_in, w_in, d->cin);
        w.dy = da.p; w.dy_dtype = dt;
        w.n = n; w.h_in = h_in; w.w_in = w_in; w.c_in = d->cin; w.h_out = h_out; w.w_out = w_out; w.c_out = d->cout;
        w.k = d->k; w.stride = d->stride; w.pad = d->pad; w.gather = d->type;
        w.dw = out.as<float>();
        const bool in_kernel = wgrad_accepts_bnbwd(w, dt);
        if (in_kernel) {
            w.dy_y = yy.p; w.dy_scale = sc.as<float>(); w.dy_shift = sf.as<float>(); w.dy_mean = mn.as<float>(); w.dy_invstd = is.as<float>();
            w.dy_coef = cf.as<float>();
        } else {   // the unfused schedule: materialise dy first
            BnBwdArgs bn;
            bn.da = da.p; bn.y = yy.p; bn.dtype = dt; bn.pixels = (int64_t)n * h_out * w_out; bn.c = d->cout;
            bn.mean = mn.as<float>(); bn.invstd = is.as<float>(); bn.scale = sc.as<float>(); bn.shift = sf.as<float>(); bn.coef = cf.as<float>();
            launch_bn_bwd_apply(bn, st.s);
        }
        const bool fast = wgrad_takes_mfma(w, dt);
        const int64_t need = fast ? wgrad_mfma_scratch_floats(w) : wgrad_generic_scratch_floats(w);
        scratch.reserve((size_t)std::max<int64_t>(need, 1) * 4);
        w.partials = scratch.as<float>(); w.partials_capacity = (int64_t)(scratch.bytes / 4);
        if (fast) launch_wgrad_mfma(w, st.s); else launch_wgrad_generic(w, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        std::vector<float> tm(nw);
        HIP_CHECK(hipMemcpy(tm.data(), out.p, nw * 4, hipMemcpyDeviceToHost));
        for (int t = 0; t < kk; ++t)
            for (int ci = 0; ci < d->cin; ++ci)
                for (int co = 0; co < d->cout; ++co) {
                    const size_t dst = d->type == 0 ? ((size_t)co * d->cin + ci) * kk + t : ((size_t)ci * d->cout + co) * kk + t;
                    dw[dst] = tm[((size_t)t * d->cin + ci) * d->cout + co];
                }
        if (computed_in_kernel) *computed_in_kernel = in_kernel ? 1 : 0;
    });
}

// ---- table mode and the training kernels that are not convolutions (see include/annonet_hip.h) ----
int anh_op_bn_fold(anh_op_bn_layer* layers, int n_jobs, uint64_t spread_seed) {
    return guarded([&] {
        ANH_REQUIRE(layers && n_jobs >= 1 && n_jobs <= 16, "1 to 16 fold jobs");
        OpStream st;
        unsigned long long state = spread_seed;
        std::vector<Table> tabs(n_jobs);
        std::vector<LayerDev> dev(n_jobs);
        BnFoldJobs jobs;
        for (int i = 0; i < n_jobs; ++i) {
            ANH_REQUIRE(layers[i].sums, "a fold job needs sums");
            dev[i].prepare(layers[i]);
            tabs[i].zero(layers[i].c); tabs[i].add_sums(layers[i].sums, BNACC_SUM_Y, state); tabs[i].upload();
            jobs.job[jobs.n++] = dev[i].job(layers[i], tabs[i].acc());
        }
        launch_bn_fold_all(jobs, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        for (int i = 0; i < n_jobs; ++i) dev[i].fetch(layers[i]);
    });
}

int anh_op_bn_forward_stats(int precision, const float* y, anh_op_bn_layer* layer, double* sums_out) {
    return guarded([&] {
        ANH_REQUIRE(y && layer && sums_out, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const anh_op_bn_layer& L = *layer;
        const int64_t pixels = (int64_t)L.pixels;
        OpStream st;
        LayerDev dev;
        dev.prepare(L);
        DevBuf yy, partials;
        upload(yy, y, (size_t)pixels * L.c, dt);
        partials.reserve((size_t)std::max(bn_partial_blocks(pixels), 1) * 2 * L.c * sizeof(double));
        BnFwdArgs bn;
        bn.y = yy.p; bn.dtype = dt; bn.pixels = pixels; bn.c = L.c; bn.gamma = dev.gamma.as<float>(); bn.beta = dev.beta.as<float>();
        bn.mean = dev.mean.as<float>(); bn.invstd = dev.invstd.as<float>(); bn.scale = dev.scale.as<float>(); bn.shift = dev.shift.as<float>();
        bn.var = dev.var.as<double>(); bn.partials = partials.as<double>(); bn.eps = L.eps;
        if (L.running_mean) { bn.running_mean = dev.rmean.as<float>(); bn.running_var = dev.rvar.as<float>(); bn.averaging_factor = L.af; bn.unbias = L.unbias; }
        const int blocks = launch_bn_forward_partials(bn, st.s);
        launch_bn_forward_finalize(bn, blocks, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        sum_partials(partials, blocks, L.c, sums_out);
        dev.fetch(*layer);
    });
}

int anh_op_conv_forward_stats_table(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const uint8_t* image,
                                    const anh_op_bn_input* a, const anh_op_bn_input* b, const float* filters, int tables,
                                    float* y, double* sums, int64_t* poison, int64_t* ticket, int* workgroups) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(filters && y && sums && (image || a) && !(image && (a || b)), "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        OpStream st;
        unsigned long long state = 0x7ab1e5ull + (unsigned long long)d->cout;
        BnSource in;
        DevBuf img;
        ConvArgs c;
        const size_t in_elems = (size_t)n * h_in * w_in * d->cin;
        if (image) {
            img.reserve(in_elems);
            HIP_CHECK(hipMemcpy(img.p, image, in_elems, hipMemcpyHostToDevice));
            c.src = image_source(img.as<uint8_t>(), h_in, w_in, d->cin);
            c.src.dtype = dt;
        } else {
            in.make(a, b, in_elems, d->cin, dt, state);
            c.src = in.src;
        }
        Filters f;
        upload_filters(f, *d, filters, dt);
        DevBuf out, partials;
        Table tab;
        const size_t out_elems = (size_t)n * h_out * w_out * d->cout;
        out.reserve(out_elems * (dt == DT_BF16 ? 2 : 4));
        c.n = n; c.h_in = h_in; c.w_in = w_in; c.c_red = d->cin; c.h_out = h_out; c.w_out = w_out; c.c_out = d->cout;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = d->type;
        c.w_f32 = f.tm_f32.as<float>(); c.w_bf16 = f.km_bf16.p;
        c.out = out.p; c.out_dtype = dt;
        // Engine::choose_table_mode: every bn layer's forward kernel adds its statistics itself, and folds its producers' tables
        const int blocks = conv_takes_mfma(c, dt) ? conv_fused_stat_blocks(c) : 0;
        ANH_REQUIRE(blocks > 0, "this layer's kernel does not fuse the bn statistics");
        ANH_REQUIRE(!c.src.a_tab.acc || conv_folds_bn_tables(c), "this layer's kernel does not fold bn accumulator tables");
        if (tables) { tab.zero(d->cout); tab.upload(); c.stat_acc = tab.acc(); }
        else { partials.reserve((size_t)blocks * 2 * d->cout * sizeof(double)); c.stat_partials = partials.as<double>(); }
        launch_conv_mfma(c, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, y, out_elems, dt);
        if (tables) { tab.download(); tab.totals(BNACC_SUM_Y, sums); }
        else sum_partials(partials, blocks, d->cout, sums);
        if (poison) *poison = tables ? tab.poison() : 0;
        if (ticket) *ticket = tables ? tab.ticket() : 0;
        if (workgroups) *workgroups = tables ? conv_mfma_workgroups(c) : blocks;
    });
}

int anh_op_conv_backward_data_bn_table(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy, const float* filters,
                                       const float* dx_init, const float* y_prev, const float* scale, const float* shift, const float* mean,
                                       const float* invstd, const float* gamma, float* dx, double* sums, float* dgamma, float* dbeta, float* coef,
                                       int64_t* ticket, int* workgroups) {
    return guarded([&] {
        check_desc(d, n, h_in, w_in);
        ANH_REQUIRE(dy && filters && dx && y_prev && scale && shift && mean && invstd && gamma && sums && dgamma && dbeta && coef, "null argument");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int h_out = out_dim(*d, h_in), w_out = out_dim(*d, w_in);
        ANH_REQUIRE(h_out >= 1 && w_out >= 1, "input too small");
        ANH_REQUIRE(bn_table_mode_ok(d->cin), "no table mode at this width");
        OpStream st;
        DevBuf g, out, yp, sc, sf, mn, is, gm, dg, db, cf;
        upload(g, dy, (size_t)n * h_out * w_out * d->cout, dt);
        Filters f;
        upload_filters(f, *d, filters, dt);
        const size_t out_elems = (size_t)n * h_in * w_in * d->cin;
        const int64_t pixels = (int64_t)n * h_in * w_in;
        if (dx_init) upload(out, dx_init, out_elems, dt); else out.reserve(out_elems * (dt == DT_BF16 ? 2 : 4));
        upload(yp, y_prev, out_elems, dt);
        upload_f32(sc, scale, d->cin); upload_f32(sf, shift, d->cin); upload_f32(mn, mean, d->cin); upload_f32(is, invstd, d->cin); upload_f32(gm, gamma, d->cin);
        fill_nan(dg, d->cin); fill_nan(db, d->cin); fill_nan(cf, (size_t)3 * d->cin);
        Table tab;
        tab.zero(d->cin); tab.upload();
        BnBwdFinish fin;
        fin.acc = tab.acc(); fin.gamma = gm.as<float>(); fin.invstd = is.as<float>(); fin.dgamma = dg.as<float>(); fin.dbeta = db.as<float>(); fin.coef = cf.as<float>();
        fin.pixels = (double)pixels; fin.c = d->cin;
        ConvArgs c;
        c.src.kind = SRC_RAW; c.src.dtype = dt; c.src.a = g.p;
        c.n = n; c.h_in = h_out; c.w_in = w_out; c.c_red = d->cout; c.h_out = h_in; c.w_out = w_in; c.c_out = d->cin;
        c.k = d->k; c.stride = d->stride; c.pad = d->pad; c.gather = 1 - d->type;
        c.w_f32 = f.km_f32.as<float>(); c.w_bf16 = f.tm_bf16.p;
        c.out = out.p; c.out_dtype = dt; c.out_accumulate = dx_init ? 1 : 0;
        const bool fast = conv_takes_mfma(c, dt);
        const bool fused_here = fast && conv_fused_bnred_blocks(c) > 0;
        int wgs;
        if (fused_here) {
            c.bnred_y = yp.p; c.bnred_scale = sc.as<float>(); c.bnred_shift = sf.as<float>(); c.bnred_mean = mn.as<float>(); c.bnred_invstd = is.as<float>();
            c.bnred_acc = tab.acc(); c.bnred_finish = fin;
            wgs = conv_mfma_workgroups(c);
        }
        if (fast) launch_conv_mfma(c, st.s); else launch_conv_generic(c, st.s);
        if (!fused_here) {   // the layer's own reduce pass adds to the table and finishes it (Engine::backward)
            BnBwdArgs bn;
            bn.da = out.p; bn.y = yp.p; bn.dtype = dt; bn.pixels = pixels; bn.c = d->cin;
            bn.mean = mn.as<float>(); bn.invstd = is.as<float>(); bn.scale = sc.as<float>(); bn.shift = sf.as<float>();
            bn.acc = tab.acc(); bn.finish = fin;
            launch_bn_bwd_reduce(bn, st.s);
            wgs = bn_partial_blocks(pixels);
        }
        HIP_CHECK(hipStreamSynchronize(st.s));
        download(out, dx, out_elems, dt);
        tab.download(); tab.totals(BNACC_SUM_DZ_XHAT, sums);
        fetch_f32(dg, dgamma, d->cin); fetch_f32(db, dbeta, d->cin); fetch_f32(cf, coef, (size_t)3 * d->cin);
        if (ticket) *ticket = tab.ticket();
        if (workgroups) *workgroups = wgs;
    });
}

int anh_op_bn_backward(int precision, anh_op_bn_bwd* op) {
    return guarded([&] {
        ANH_REQUIRE(op && op->y && op->mean && op->invstd && op->scale && op->shift && op->c >= 1 && op->pixels >= 1, "null argument");
        anh_op_bn_bwd& o = *op;
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const bool head = o.head_g != nullptr;
        const bool reduce = o.stages & 1, finalize = o.stages & 2, apply = o.stages & 4;
        ANH_REQUIRE(head ? (!o.da && o.head_w_tm && !reduce && !finalize) : o.da != nullptr, "da, or the head form with the apply stage alone");
        ANH_REQUIRE(!finalize || reduce, "finalize needs the reduce stage");
        ANH_REQUIRE(!o.tables || (bn_table_mode_ok(o.c) && !finalize), "table mode: vector widths, and no finalize kernel");
        ANH_REQUIRE(!reduce || (o.gamma && o.sums), "the reduce stage needs gamma and sums");
        const bool coef_made = finalize || (o.tables && reduce);
        ANH_REQUIRE(!apply || ((coef_made || o.coef_in) && o.dy), "the apply stage needs coefficients and dy");
        const size_t elems = (size_t)o.pixels * o.c;
        const size_t es = dt == DT_BF16 ? 2 : 4;
        OpStream st;
        DevBuf da, yy, mn, is, sc, sf, gm, dg, db, cf, partials, dyb, hg, hw;
        if (head) { da.reserve(elems * es); HIP_CHECK(hipMemset(da.p, 0xff, elems * es)); }
        else upload(da, o.da, elems, dt);
        upload(yy, o.y, elems, dt);
        upload_f32(mn, o.mean, o.c); upload_f32(is, o.invstd, o.c); upload_f32(sc, o.scale, o.c); upload_f32(sf, o.shift, o.c);
        if (o.gamma) upload_f32(gm, o.gamma, o.c);
        fill_nan(dg, o.c); fill_nan(db, o.c);
        if (!coef_made && o.coef_in) upload_f32(cf, o.coef_in, (size_t)3 * o.c); else fill_nan(cf, (size_t)3 * o.c);
        const int blocks = bn_partial_blocks(o.pixels);
        partials.reserve((size_t)std::max(blocks, 1) * 2 * o.c * sizeof(double));
        Table tab;
        BnBwdArgs b;
        b.da = da.p; b.y = yy.p; b.dtype = dt; b.pixels = o.pixels; b.c = o.c;
        b.gamma = gm.as<float>(); b.mean = mn.as<float>(); b.invstd = is.as<float>(); b.scale = sc.as<float>(); b.shift = sf.as<float>();
        b.dgamma = dg.as<float>(); b.dbeta = db.as<float>(); b.partials = partials.as<double>(); b.coef = cf.as<float>();
        if (o.out_of_place) { dyb.reserve(elems * es); HIP_CHECK(hipMemset(dyb.p, 0xff, elems * es)); b.dy_out = dyb.p; }
        if (head) {
            upload_f32(hg, o.head_g, (size_t)o.pixels * o.head_k);
            std::vector<float> w((size_t)32 * std::max(o.head_k, 1));   // the engine's fp32 copy carries the rounded values
            for (size_t i = 0; i < w.size(); ++i) w[i] = dt == DT_BF16 ? from_bf16_bits(to_bf16_bits(o.head_w_tm[i])) : o.head_w_tm[i];
            upload_f32(hw, w.data(), w.size());
            b.head_g = hg.as<float>(); b.head_w_tm = hw.as<float>(); b.head_k = o.head_k;
        }
        if (o.tables) {
            tab.zero(o.c); tab.upload();
            b.acc = tab.acc();
            b.finish.gamma = gm.as<float>(); b.finish.invstd = is.as<float>(); b.finish.dgamma = dg.as<float>(); b.finish.dbeta = db.as<float>();
            b.finish.coef = cf.as<float>(); b.finish.pixels = (double)o.pixels; b.finish.c = o.c;
        }
        if (reduce) launch_bn_bwd_reduce(b, st.s);
        if (finalize) launch_bn_bwd_finalize(b, st.s);
        if (apply) launch_bn_bwd_apply(b, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        if (reduce) {
            if (o.tables) { tab.download(); tab.totals(BNACC_SUM_DZ_XHAT, o.sums); o.ticket = tab.ticket(); }
            else sum_partials(partials, blocks, o.c, o.sums);
        }
        fetch_f32(dg, o.dgamma, o.c); fetch_f32(db, o.dbeta, o.c); fetch_f32(cf, o.coef, (size_t)3 * o.c);
        if (apply) download(o.out_of_place ? dyb : da, o.dy, elems, dt);
        o.workgroups = blocks;
    });
}

int anh_op_head_train(int precision, anh_op_head* op) {
    return guarded([&] {
        ANH_REQUIRE(op && op->a && op->w_tm && op->bias && op->labels && op->weights && op->logits && op->dlogits && op->loss && op->dbias && op->dw &&
                    op->pixels >= 1, "null argument");
        anh_op_head& o = *op;
        ANH_REQUIRE(o.k >= 1 && o.k <= 4, "1 to 4 classes");
        ANH_REQUIRE(o.da_virtual || o.da, "da, or da_virtual");
        ANH_REQUIRE(o.bn_sums >= 0 && o.bn_sums <= 2 && (o.bn_sums == 0 || (!o.b && o.bn_sums_out)), "bn sums: single input only");
        ANH_REQUIRE(o.bn_sums != 1 || (o.bn_mean && o.bn_invstd), "the partials form needs mean and invstd");
        ANH_REQUIRE(o.bn_sums != 2 || (o.a->sums && o.bn_gamma && o.dgamma && o.dbeta && o.coef), "the table form needs the input's table and gamma");
        ANH_REQUIRE(o.n_fold_jobs >= 0 && o.n_fold_jobs <= 16 && (o.n_fold_jobs == 0 || o.fold_jobs), "0 to 16 fold jobs");
        const DType dt = precision == ANH_BF16 ? DT_BF16 : DT_F32;
        const int C = 32, K = o.k;
        const size_t elems = (size_t)o.pixels * C;
        OpStream st;
        unsigned long long state = 0x4ead5ull + (unsigned long long)K;
        BnSource in;
        in.make(o.a, o.b, elems, C, dt, state);
        std::vector<float> wt((size_t)C * K), wk((size_t)C * K);
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < K; ++k) {
                const float w = dt == DT_BF16 ? from_bf16_bits(to_bf16_bits(o.w_tm[c * K + k])) : o.w_tm[c * K + k];
                wt[(size_t)c * K + k] = w; wk[(size_t)k * C + c] = w;
            }
        DevBuf w_tm, w_km, bias, labels, weights, logits, dlogits, da, partials, loss, loss32, dbias, dw, err, mn, is, gm, bnp, dg, db, cf;
        upload_f32(w_tm, wt.data(), wt.size()); upload_f32(w_km, wk.data(), wk.size()); upload_f32(bias, o.bias, K);
        labels.reserve((size_t)o.pixels * 2);
        HIP_CHECK(hipMemcpy(labels.p, o.labels, (size_t)o.pixels * 2, hipMemcpyHostToDevice));
        upload_f32(weights, o.weights, o.pixels);
        fill_nan(logits, (size_t)o.pixels * K); fill_nan(dlogits, (size_t)o.pixels * K);
        fill_nan(dbias, K); fill_nan(dw, (size_t)C * K); fill_nan(loss32, 1);
        loss.reserve(sizeof(double)); err.reserve(sizeof(int));
        HIP_CHECK(hipMemset(loss.p, 0xff, sizeof(double))); HIP_CHECK(hipMemset(err.p, 0, sizeof(int)));
        HeadTrainArgs t;
        t.src = in.src; t.c_in = C; t.k = K;
        t.w_tm = w_tm.as<float>(); t.w_km = w_km.as<float>(); t.bias = bias.as<float>();
        t.labels = labels.as<uint16_t>(); t.weights = weights.as<float>();
        t.logits = logits.as<float>(); t.dlogits = dlogits.as<float>();
        if (!o.da_virtual) { da.reserve(elems * (dt == DT_BF16 ? 2 : 4)); HIP_CHECK(hipMemset(da.p, 0xff, da.bytes)); t.da = da.p; }
        t.pixels = o.pixels; t.scale = o.scale;
        ANH_REQUIRE(head_train_supported(t), "not a shape of the fused head");
        const int blocks = head_train_blocks(o.pixels);
        partials.reserve((size_t)head_train_partial_doubles(t) * sizeof(double));
        t.partials = partials.as<double>();
        t.loss_out = loss.as<double>(); t.loss_out_f32 = loss32.as<float>(); t.dbias = dbias.as<float>(); t.dw = dw.as<float>();
        t.error_flag = err.as<int>();
        fill_nan(dg, C); fill_nan(db, C); fill_nan(cf, (size_t)3 * C);
        if (o.bn_sums == 1) {
            upload_f32(mn, o.bn_mean, C); upload_f32(is, o.bn_invstd, C);
            bnp.reserve((size_t)blocks * 2 * C * sizeof(double));
            t.bnred_mean = mn.as<float>(); t.bnred_invstd = is.as<float>(); t.bnred_partials = bnp.as<double>();
        } else if (o.bn_sums == 2) {   // the arrays exist in the engine, but this launch's fold jobs may not have written them yet: NaN here
            fill_nan(mn, C); fill_nan(is, C); upload_f32(gm, o.bn_gamma, C);
            t.bnred_mean = mn.as<float>(); t.bnred_invstd = is.as<float>();
            t.bnred_acc = in.a.tab.acc();
            t.bnred_finish.acc = in.a.tab.acc(); t.bnred_finish.gamma = gm.as<float>(); t.bnred_finish.invstd = is.as<float>();
            t.bnred_finish.dgamma = dg.as<float>(); t.bnred_finish.dbeta = db.as<float>(); t.bnred_finish.coef = cf.as<float>();
            t.bnred_finish.pixels = (double)o.pixels; t.bnred_finish.c = C;
        }
        std::vector<Table> ftabs(o.n_fold_jobs);
        std::vector<LayerDev> fdev(o.n_fold_jobs);
        BnFoldJobs jobs;
        for (int i = 0; i < o.n_fold_jobs; ++i) {
            ANH_REQUIRE(o.fold_jobs[i].sums, "a fold job needs sums");
            fdev[i].prepare(o.fold_jobs[i]);
            ftabs[i].zero(o.fold_jobs[i].c); ftabs[i].add_sums(o.fold_jobs[i].sums, BNACC_SUM_Y, state); ftabs[i].upload();
            jobs.job[jobs.n++] = fdev[i].job(o.fold_jobs[i], ftabs[i].acc());
        }
        if (jobs.n) {   // Engine::backward: the jobs ride in the head kernel's first workgroups when it has enough of them
            if (blocks >= jobs.n) t.fold = &jobs; else launch_bn_fold_all(jobs, st.s);
        }
        launch_head_train(t, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        fetch_f32(logits, o.logits, (size_t)o.pixels * K); fetch_f32(dlogits, o.dlogits, (size_t)o.pixels * K);
        if (!o.da_virtual) download(da, o.da, elems, dt);
        HIP_CHECK(hipMemcpy(o.loss, loss.p, sizeof(double), hipMemcpyDeviceToHost));
        fetch_f32(dbias, o.dbias, K); fetch_f32(dw, o.dw, (size_t)C * K);
        HIP_CHECK(hipMemcpy(&o.error_flag, err.p, sizeof(int), hipMemcpyDeviceToHost));
        if (o.bn_sums == 1) sum_partials(bnp, blocks, C, o.bn_sums_out);
        if (o.bn_sums == 2) { in.a.tab.download(); in.a.tab.totals(BNACC_SUM_DZ_XHAT, o.bn_sums_out); o.ticket = in.a.tab.ticket(); }
        fetch_f32(dg, o.dgamma, C); fetch_f32(db, o.dbeta, C); fetch_f32(cf, o.coef, (size_t)3 * C);
        for (int i = 0; i < o.n_fold_jobs; ++i) fdev[i].fetch(o.fold_jobs[i]);
        o.workgroups = blocks;
    });
}

int anh_op_loss(const float* logits, const uint16_t* labels, const float* weights, int64_t pixels, int k, double scale,
                float* dlogits, double* loss, float* dbias, int* error_flag) {
    return guarded([&] {
        ANH_REQUIRE(logits && labels && weights && dlogits && loss && dbias && pixels >= 1 && k >= 1, "null argument");
        OpStream st;
        DevBuf z, lab, wgt, g, partials, ls, ls32, db, err;
        upload_f32(z, logits, (size_t)pixels * k);
        lab.reserve((size_t)pixels * 2);
        HIP_CHECK(hipMemcpy(lab.p, labels, (size_t)pixels * 2, hipMemcpyHostToDevice));
        upload_f32(wgt, weights, pixels);
        fill_nan(g, (size_t)pixels * k); fill_nan(db, k); fill_nan(ls32, 1);
        ls.reserve(sizeof(double)); err.reserve(sizeof(int));
        HIP_CHECK(hipMemset(ls.p, 0xff, sizeof(double))); HIP_CHECK(hipMemset(err.p, 0, sizeof(int)));
        partials.reserve((size_t)loss_partial_blocks(pixels) * (1 + k) * sizeof(double));
        LossArgs a;
        a.logits = z.as<float>(); a.labels = lab.as<uint16_t>(); a.weights = wgt.as<float>(); a.dlogits = g.as<float>();
        a.pixels = pixels; a.k = k; a.scale = scale;
        a.partials = partials.as<double>(); a.loss_out = ls.as<double>(); a.loss_out_f32 = ls32.as<float>(); a.dbias = db.as<float>();
        a.error_flag = err.as<int>();
        launch_loss(a, st.s);
        HIP_CHECK(hipStreamSynchronize(st.s));
        fetch_f32(g, dlogits, (size_t)pixels * k); fetch_f32(db, dbias, k);
        HIP_CHECK(hipMemcpy(loss, ls.p, sizeof(double), hipMemcpyDeviceToHost));
        if (error_flag) HIP_CHECK(hipMemcpy(error_flag, err.p, sizeof(int), hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
