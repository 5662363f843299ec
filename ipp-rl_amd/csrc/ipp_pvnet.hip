// The policy-value network's inference engine (include/ipp_engine.h "Policy-value network"): a validated plan of op records, the
// packed weights on the device (fp32, and their bf16 rounding for the bf16 path), three activation buffers sized for max_batch,
// and a forward that launches one kernel per op (csrc/k_pvnet.h).  A translation unit of its own: nothing here touches the env engine.
// The trainer's two calls (ipp_pvnet_loss, ipp_pvnet_sgd_step: csrc/k_train.h) live here too; they need no handle.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "../../include/ipp_engine.h"
#include "ipp_host.h"
#include "k_pvnet.h"
#include "k_train.h"

using ipp::fail;

namespace {

constexpr int kBuffers = 3, kSlots = 2, kMaxKmax = 8192;

struct PvNet {
    int device = 0, precision = 0, max_batch = 0, pooled_floats = 0;
    uint64_t n_floats = 0, buf_floats = 0;  // buf_floats: per sample
    std::vector<ipp_pvnet_op> ops;
    float* w = nullptr;
    unsigned short* wbf = nullptr;
    float* buf[kBuffers] = {nullptr, nullptr, nullptr};
    float* pooled = nullptr;  // [kSlots][max_batch][pooled_floats]
    int in_c = 0, in_h = 0, in_w = 0;
    ~PvNet() {
        if (w) (void)hipFree(w);
        if (wbf) (void)hipFree(wbf);
        for (auto* b : buf)
            if (b) (void)hipFree(b);
        if (pooled) (void)hipFree(pooled);
    }
};

int bad_plan(int i, const char* why) { return fail(-1, "ipp_pvnet_create: op %d: %s", i, why); }

// every condition a launch relies on, checked once: an invalid plan fails here and never at launch
int validate(PvNet& net) {
    struct Shape { int h = 0, w = 0, c = 0; bool set = false; } shape[kBuffers];
    bool pooled_set[kSlots] = {false, false};
    int pooled_c[kSlots] = {0, 0};
    const uint64_t nf = net.n_floats;
    auto fits = [&](int64_t off, uint64_t n) { return off >= 0 && (uint64_t)off <= nf && n <= nf - (uint64_t)off; };
    bool has_policy = false, has_value = false;
    for (int i = 0; i < (int)net.ops.size(); ++i) {
        const ipp_pvnet_op& o = net.ops[i];
        if (o.kind < IPP_PV_OP_CONV || o.kind > IPP_PV_OP_POLICY) return bad_plan(i, "unknown op kind");
        if (o.act < 0 || o.act > 2) return bad_plan(i, "unknown activation");
        if (o.kind == IPP_PV_OP_CONV || o.kind == IPP_PV_OP_MIX || o.kind == IPP_PV_OP_POOL) {
            if (o.cin < 1 || o.cout < 1 || o.hin < 1 || o.win < 1 || o.hin > 4096 || o.win > 4096 || o.cin > 65536 || o.cout > 65536)
                return bad_plan(i, "extent out of range");
            const int c_src = o.kind == IPP_PV_OP_MIX ? o.cout : o.cin;
            if (o.src == IPP_PV_INPUT) {
                if (i != 0 || o.kind != IPP_PV_OP_CONV) return bad_plan(i, "only the first conv reads the planes");
                net.in_c = o.cin; net.in_h = o.hin; net.in_w = o.win;
            } else {
                if (o.src < 0 || o.src >= kBuffers) return bad_plan(i, "buffer id out of range");
                const Shape& s = shape[o.src];
                if (!s.set || s.h != o.hin || s.w != o.win || s.c != c_src) return bad_plan(i, "shapes do not chain");
            }
        }
        if (o.kind == IPP_PV_OP_CONV) {
            const bool known = (o.kh == 7 && o.kw == 7) || (o.kh == 3 && o.kw == 3) || (o.kh == 3 && o.kw == 1) || (o.kh == 1 && o.kw == 3) ||
                               (o.kh == 1 && o.kw == 1);
            if (!known) return bad_plan(i, "kernel extent not one of 7x7, 3x3, 3x1, 1x3, 1x1");
            if (o.stride != 1 && o.stride != 2) return bad_plan(i, "stride not 1 or 2");
            if (o.pad_h < 0 || o.pad_h > 3 || o.pad_w < 0 || o.pad_w > 3) return bad_plan(i, "padding out of range");
            if (o.hout != (o.hin + 2 * o.pad_h - o.kh) / o.stride + 1 || o.wout != (o.win + 2 * o.pad_w - o.kw) / o.stride + 1 || o.hout < 1 || o.wout < 1)
                return bad_plan(i, "output extent does not follow from the input");
            if (o.dst < 0 || o.dst >= kBuffers) return bad_plan(i, "buffer id out of range");
            if (o.dst == o.src) return bad_plan(i, "a conv cannot run in place");
            if (o.res != -1) {
                if (o.res < 0 || o.res >= kBuffers) return bad_plan(i, "buffer id out of range");
                if (o.res == o.dst) return bad_plan(i, "the residual cannot be the output buffer");
                const Shape& s = shape[o.res];
                if (!s.set || s.h != o.hout || s.w != o.wout || s.c != o.cout) return bad_plan(i, "shapes do not chain (residual)");
            }
            if (!fits(o.w_off, (uint64_t)o.cout * o.kh * o.kw * o.cin) || !fits(o.b_off, o.cout)) return bad_plan(i, "weight offset beyond the blob");
            shape[o.dst] = Shape{o.hout, o.wout, o.cout, true};
            const uint64_t per = (uint64_t)o.hout * o.wout * o.cout;
            if (per > net.buf_floats) net.buf_floats = per;
        } else if (o.kind == IPP_PV_OP_MIX) {
            if (o.dst != o.src) return bad_plan(i, "the context mix runs in place");
            if (o.cin >= o.cout) return bad_plan(i, "pooled channels must be fewer than the channels");
            if ((uint64_t)(o.cout + o.cin) * 4 > 48 * 1024) return bad_plan(i, "channels beyond the mix kernel's LDS");
            const uint64_t r = o.cout - o.cin;
            if (!fits(o.w_off, o.cin) || !fits(o.b_off, o.cin) || !fits(o.w2_off, r * 2 * o.cin) || !fits(o.b2_off, r))
                return bad_plan(i, "weight offset beyond the blob");
        } else if (o.kind == IPP_PV_OP_POOL) {
            if (o.dst < 0 || o.dst >= kSlots) return bad_plan(i, "pooled slot out of range");
            pooled_set[o.dst] = true;
            pooled_c[o.dst] = o.cin;
            if (2 * o.cin > net.pooled_floats) net.pooled_floats = 2 * o.cin;
        } else {
            if (o.src < 0 || o.src >= kSlots) return bad_plan(i, "pooled slot out of range");
            if (!pooled_set[o.src] || pooled_c[o.src] != o.cin || o.cout < 1) return bad_plan(i, "shapes do not chain (pooled vector)");
            const uint64_t rows = o.kind == IPP_PV_OP_VALUE ? 1 : (uint64_t)o.cout;
            if (!fits(o.w_off, rows * 2 * o.cin) || !fits(o.b_off, rows)) return bad_plan(i, "weight offset beyond the blob");
            (o.kind == IPP_PV_OP_VALUE ? has_value : has_policy) = true;
        }
    }
    if (net.in_c == 0) return fail(-1, "ipp_pvnet_create: the plan does not start with a conv on the planes");
    if (!has_value || !has_policy) return fail(-1, "ipp_pvnet_create: the plan lacks a value or a policy head");
    return 0;
}

int upload(PvNet& net, const float* weights, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(net.w, weights, net.n_floats * sizeof(float), hipMemcpyHostToDevice, s));
    if (net.precision == IPP_PV_BF16) {
        const unsigned blocks = (unsigned)((net.n_floats + 255) / 256);
        hipLaunchKernelGGL(pv::k_pv_to_bf16, dim3(blocks), dim3(256), 0, s, net.w, net.wbf, (unsigned long long)net.n_floats);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));  // the host blob may go away when the call returns
    return 0;
}

}  // namespace

extern "C" {

int ipp_pvnet_create(const ipp_pvnet_op* ops, int32_t n_ops, const float* weights, uint64_t n_floats, int32_t precision, int32_t max_batch,
                     int32_t device, void** out) {
    if (!ops || !weights || !out || n_ops < 1 || n_floats < 1) return fail(-1, "ipp_pvnet_create: null / empty argument");
    *out = nullptr;
    if (precision != IPP_PV_FP32 && precision != IPP_PV_BF16) return fail(-1, "ipp_pvnet_create: unknown precision");
    if (max_batch < 1) return fail(-1, "ipp_pvnet_create: max_batch < 1");
    if (n_floats > ((uint64_t)1 << 31)) return fail(-1, "ipp_pvnet_create: weight blob too large");
    PvNet* net = new PvNet;
    net->device = device; net->precision = precision; net->max_batch = max_batch; net->n_floats = n_floats;
    net->ops.assign(ops, ops + n_ops);
    int rc = validate(*net);
    if (rc == 0 && net->buf_floats * (uint64_t)max_batch >= ((uint64_t)1 << 40)) rc = fail(-1, "ipp_pvnet_create: activation buffers too large");
    if (rc != 0) { delete net; return rc; }
    auto guard = [&](hipError_t e, const char* what) { if (e == hipSuccess) return 0; delete net; return fail(-2, "%s failed: %s", what, hipGetErrorString(e)); };
    if ((rc = guard(hipSetDevice(device), "hipSetDevice"))) return rc;
    if ((rc = guard(hipMalloc(&net->w, n_floats * sizeof(float)), "hipMalloc(weights)"))) return rc;
    if (precision == IPP_PV_BF16 && (rc = guard(hipMalloc(&net->wbf, n_floats * sizeof(unsigned short)), "hipMalloc(bf16 weights)"))) return rc;
    for (int b = 0; b < kBuffers; ++b)
        if ((rc = guard(hipMalloc(&net->buf[b], net->buf_floats * (uint64_t)max_batch * sizeof(float)), "hipMalloc(activations)"))) return rc;
    if ((rc = guard(hipMalloc(&net->pooled, (uint64_t)kSlots * max_batch * net->pooled_floats * sizeof(float)), "hipMalloc(pooled)"))) return rc;
    rc = upload(*net, weights, nullptr);
    if (rc != 0) { delete net; return rc; }
    *out = net;
    return 0;
}

int ipp_pvnet_set_weights(void* handle, const float* weights, uint64_t n_floats, void* stream) {
    PvNet* net = static_cast<PvNet*>(handle);
    if (!net || !weights) return fail(-1, "ipp_pvnet_set_weights: null argument");
    if (n_floats != net->n_floats) return fail(-1, "ipp_pvnet_set_weights: the blob's size differs from the plan's");
    HIP_TRY(hipSetDevice(net->device));
    return upload(*net, weights, reinterpret_cast<hipStream_t>(stream));
}

int ipp_pvnet_forward(void* handle, const float* planes, int32_t n, const int32_t* valid_idx, int32_t kmax, double* prior, double* value,
                      int32_t tap_op, float* tap_out, void* stream) {
    PvNet* net = static_cast<PvNet*>(handle);
    if (!net || !planes || !valid_idx || !prior || !value) return fail(-1, "ipp_pvnet_forward: null argument");
    if (n < 0) return fail(-1, "ipp_pvnet_forward: n < 0");
    if (kmax < 1 || kmax > kMaxKmax) return fail(-1, "ipp_pvnet_forward: kmax out of range");
    if (tap_op != -1 && (tap_op < 0 || tap_op >= (int)net->ops.size() || net->ops[tap_op].kind != IPP_PV_OP_CONV || !tap_out))
        return fail(-1, "ipp_pvnet_forward: tap_op must be a conv op of the plan, with tap_out");
    HIP_TRY(hipSetDevice(net->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t plane_floats = (uint64_t)net->in_c * net->in_h * net->in_w;
    const void* wts = net->precision == IPP_PV_BF16 ? static_cast<const void*>(net->wbf) : static_cast<const void*>(net->w);
    const size_t wsz = net->precision == IPP_PV_BF16 ? sizeof(unsigned short) : sizeof(float);
    for (int32_t c0 = 0; c0 < n; c0 += net->max_batch) {
        const int nb = n - c0 < net->max_batch ? n - c0 : net->max_batch;
        for (int i = 0; i < (int)net->ops.size(); ++i) {
            const ipp_pvnet_op& o = net->ops[i];
            if (o.kind == IPP_PV_OP_CONV) {
                pv::ConvArgs a;
                a.in = o.src == IPP_PV_INPUT ? planes + (uint64_t)c0 * plane_floats : net->buf[o.src];
                a.w = static_cast<const char*>(wts) + (uint64_t)o.w_off * wsz;
                a.bias = net->w + o.b_off;
                a.res = o.res >= 0 ? net->buf[o.res] : nullptr;
                a.out = net->buf[o.dst];
                a.M = (long long)nb * o.hout * o.wout;
                a.K = o.kh * o.kw * o.cin;
                a.cin = o.cin; a.cout = o.cout; a.hin = o.hin; a.win = o.win; a.hout = o.hout; a.wout = o.wout;
                a.kh = o.kh; a.kw = o.kw; a.stride = o.stride; a.pad_h = o.pad_h; a.pad_w = o.pad_w; a.act = o.act;
                a.in_nchw = o.src == IPP_PV_INPUT;
                const dim3 grid((unsigned)((a.M + pv::kBM - 1) / pv::kBM), (unsigned)((o.cout + pv::kBN - 1) / pv::kBN));
                if (net->precision == IPP_PV_BF16) hipLaunchKernelGGL(pv::k_pv_conv<true>, grid, dim3(pv::kThreads), 0, s, a);
                else hipLaunchKernelGGL(pv::k_pv_conv<false>, grid, dim3(pv::kThreads), 0, s, a);
                if (i == tap_op) {
                    const int P = o.hout * o.wout;
                    const long long total = (long long)nb * P * o.cout;
                    hipLaunchKernelGGL(pv::k_pv_tap, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)net->buf[o.dst],
                                       tap_out + (uint64_t)c0 * P * o.cout, total, P, o.cout);
                }
            } else if (o.kind == IPP_PV_OP_MIX) {
                hipLaunchKernelGGL(pv::k_pv_mix, dim3(nb), dim3(pv::kThreads), (size_t)(o.cout + o.cin) * sizeof(float), s, net->buf[o.src],
                                   o.hin * o.win, o.cout, o.cin, (const float*)(net->w + o.w_off), (const float*)(net->w + o.b_off),
                                   (const float*)(net->w + o.w2_off), (const float*)(net->w + o.b2_off), o.act);
            } else {
                const bool pool = o.kind == IPP_PV_OP_POOL;
                const int slot = pool ? o.dst : o.src;
                float* pooled = net->pooled + (uint64_t)slot * net->max_batch * net->pooled_floats;
                const int mode = pool ? pv::kHeadPool : (o.kind == IPP_PV_OP_VALUE ? pv::kHeadValue : pv::kHeadPolicy);
                // (the pooled rows of a slot are 2 cin floats apart: validate() ties the head's cin to the pool's)
                hipLaunchKernelGGL(pv::k_pv_heads, dim3(nb), dim3(pv::kThreads), mode == pv::kHeadPolicy ? (size_t)kmax * sizeof(float) : 0, s, mode,
                                   pool ? (const float*)net->buf[o.src] : (const float*)nullptr, o.hin * o.win, o.cin, pooled,
                                   pool ? (const float*)nullptr : (const float*)(net->w + o.w_off),
                                   pool ? (const float*)nullptr : (const float*)(net->w + o.b_off), o.act, o.cout,
                                   valid_idx + (uint64_t)c0 * kmax, kmax, prior + (uint64_t)c0 * kmax, value + c0);
            }
        }
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int ipp_pvnet_loss(const float* logits, const float* target_policy, const uint8_t* valid_msk, const float* value, const float* reward,
                   const double* target_value, const double* target_reward, const double* weights, int32_t n, int32_t num_actions,
                   double policy_coeff, double value_coeff, double reward_coeff, double entropy_coeff, double* stats, float* grad_logits,
                   float* grad_value, float* grad_reward, int32_t device, void* stream) {
    if (n < 0) return fail(-1, "ipp_pvnet_loss: n < 0");
    if (num_actions < 1) return fail(-1, "ipp_pvnet_loss: num_actions < 1");
    if (!logits || !target_policy || !valid_msk || !value || !target_value || !weights || !stats || !grad_logits || !grad_value)
        return fail(-1, "ipp_pvnet_loss: null argument");
    if ((reward == nullptr) != (target_reward == nullptr) || (reward == nullptr) != (grad_reward == nullptr))
        return fail(-1, "ipp_pvnet_loss: reward, target_reward and grad_reward are given together or not at all");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    pvt::LossArgs a;
    a.n = n; a.A = num_actions;
    a.logits = logits; a.target_policy = target_policy; a.valid_msk = valid_msk; a.value = value; a.reward = reward;
    a.target_value = target_value; a.target_reward = target_reward; a.weights = weights;
    a.pc = policy_coeff; a.vc = value_coeff; a.rc = reward_coeff; a.ec = entropy_coeff;
    a.stats = stats; a.grad_logits = grad_logits; a.grad_value = grad_value; a.grad_reward = grad_reward;
    hipLaunchKernelGGL(pvt::k_pv_loss, dim3((unsigned)n), dim3(pvt::kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_pvnet_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, double lr, double momentum, double weight_decay,
                       double max_norm, double* norm_out, double* scratch, uint64_t scratch_doubles, int32_t device, void* stream) {
    static_assert(pvt::kSgdMaxBlocks == IPP_PVNET_SGD_SCRATCH, "scratch bound");
    if (n < 0) return fail(-1, "ipp_pvnet_sgd_step: n < 0");
    if (!params || !grads || !momentum_buf || !norm_out || !scratch) return fail(-1, "ipp_pvnet_sgd_step: null argument");
    const int blocks = pvt::sgd_blocks(n);
    if (scratch_doubles < (uint64_t)blocks)
        return fail(-1, "ipp_pvnet_sgd_step: scratch of %llu doubles, %d needed", (unsigned long long)scratch_doubles, blocks);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pvt::k_sgd_partial, dim3(blocks), dim3(pvt::kThreads), 0, s, grads, (long long)n, scratch);
    hipLaunchKernelGGL(pvt::k_sgd_update, dim3(blocks), dim3(pvt::kThreads), 0, s, params, grads, momentum_buf, (long long)n, lr, momentum,
                       weight_decay, max_norm, (const double*)scratch, norm_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ipp_pvnet_destroy(void* handle) {
    PvNet* net = static_cast<PvNet*>(handle);
    if (!net) return 0;
    (void)hipSetDevice(net->device);
    delete net;
    return 0;
}

}  // extern "C"
