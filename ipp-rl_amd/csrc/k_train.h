// Training of the policy-value network (planning/mcts_zero/network_wrappers/policy_value_network_wrappers.py:34-215): the two parts of
// an iteration that stock PyTorch runs as dozens of small launches, one kernel each.  Everything after the f32 loads is fp64 and every
// sum runs in a fixed order (no floating-point atomics), so two runs agree bit for bit.  Kernels:
//   k_pv_loss       one workgroup per minibatch row: the masked log-softmax (:116-118 with layers.py's shift by 1000), policy loss,
//                   entropy, value / reward losses, the weighted total (:120-154, :251-261) and the gradient of the batch mean with
//                   respect to the logits, the value and the reward.  The row is read four times (max, normaliser, sums, gradients):
//                   a row of 20 000 actions does not fit in registers, the re-reads come from cache.
//   k_sgd_partial   per-workgroup partial sums of g^2 over a fixed grid-stride partition                           (:169-171)
//   k_sgd_update    every workgroup adds the partials in index order (the norm), then clip, weight decay, momentum and the update of
//                   its elements (clip_grad_norm_ + torch.optim.SGD.step, dampening 0, no Nesterov; :169-172)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pvt {

constexpr int kThreads = 256;        // workgroup of every kernel here: 4 waves
constexpr int kSgdMaxBlocks = 1024;  // = IPP_PVNET_SGD_SCRATCH: the most partial sums a step writes
constexpr int kSgdPerBlock = 1024;   // elements per workgroup below which the grid grows instead of the stride loop

// Sum over the workgroup, the same value in every thread: a butterfly inside each wave, then the waves' sums in wave order.
// s_wave: kThreads / 64 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // (s_wave may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) tot += s_wave[w];
    return tot;
}

__device__ __forceinline__ double block_max(double v, double* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = s_wave[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) m = fmax(m, s_wave[w]);
    return m;
}

struct LossArgs {
    int n, A;
    const float* logits; const float* target_policy; const uint8_t* valid_msk;
    const float* value; const float* reward;  // reward: null without a reward target
    const double* target_value; const double* target_reward; const double* weights;
    double pc, vc, rc, ec;
    double* stats;  // [n][6]
    float* grad_logits; float* grad_value; float* grad_reward;
};

// z' = z - (1 - m) 1000: a shift, not a mask (layers.py:343-344)
__device__ __forceinline__ double shifted(const float* __restrict__ z, const uint8_t* __restrict__ m, long long j) {
    return (double)z[j] - (1.0 - (double)m[j]) * 1000.0;
}

__global__ __launch_bounds__(kThreads) void k_pv_loss(LossArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kThreads / 64];
    const int i = blockIdx.x;
    const int A = a.A;
    const long long row = (long long)i * A;
    const float* __restrict__ z = a.logits + row;
    const float* __restrict__ t = a.target_policy + row;
    const uint8_t* __restrict__ m = a.valid_msk + row;
    float* __restrict__ gz = a.grad_logits + row;

    double mx = -INFINITY;
    for (int j = threadIdx.x; j < A; j += kThreads) mx = fmax(mx, shifted(z, m, j));
    mx = block_max(mx, s_wave);
    double s = 0.0;
    for (int j = threadIdx.x; j < A; j += kThreads) s += exp(shifted(z, m, j) - mx);
    const double lse = mx + log(block_sum(s, s_wave));
    double pl = 0.0, H = 0.0, T = 0.0;
    for (int j = threadIdx.x; j < A; j += kThreads) {
        const double lp = shifted(z, m, j) - lse;
        const double tm = (double)t[j] * (double)m[j];
        pl -= tm * lp;  // (targets * predicted * valid_actions_msk, :257)
        H -= exp(lp) * lp;
        T += tm;
    }
    pl = block_sum(pl, s_wave);
    H = block_sum(H, s_wave);
    T = block_sum(T, s_wave);

    const double w = a.weights[i], wn = w / (double)a.n;
    const double v = (double)a.value[i], tv = (double)(float)a.target_value[i];
    const double dv = v - tv, vl = dv * dv;
    double rl = 0.0, dr = 0.0;
    if (a.reward) {
        dr = (double)a.reward[i] - (double)(float)a.target_reward[i];
        rl = dr * dr;
    }
    for (int j = threadIdx.x; j < A; j += kThreads) {
        const double lp = shifted(z, m, j) - lse;
        const double p = exp(lp);
        const double tm = (double)t[j] * (double)m[j];
        gz[j] = (float)(wn * (a.pc * (T * p - tm) + a.ec * (p * (lp + H))));
    }
    if (threadIdx.x == 0) {
        double* st = a.stats + (long long)i * 6;
        st[0] = pl; st[1] = vl; st[2] = rl; st[3] = H;
        st[4] = (a.pc * pl + a.vc * vl + a.rc * rl - a.ec * H) * w;
        st[5] = fabs(tv - v) / fabs(tv);
        a.grad_value[i] = (float)(wn * (2.0 * a.vc * dv));
        if (a.reward) a.grad_reward[i] = (float)(wn * (2.0 * a.rc * dr));
    }
}

// workgroups of a step over N elements: a function of N alone, so that the partition (and with it the order of the additions) is fixed
__host__ __device__ inline int sgd_blocks(long long N) {
    const long long b = (N + kSgdPerBlock - 1) / kSgdPerBlock;
    return (int)(b < 1 ? 1 : (b > kSgdMaxBlocks ? kSgdMaxBlocks : b));
}

__global__ __launch_bounds__(kThreads) void k_sgd_partial(const float* __restrict__ g, long long N, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kThreads / 64];
    double s = 0.0;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < N; k += stride) {
        const double x = (double)g[k];
        s += x * x;
    }
    s = block_sum(s, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_sgd_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long N,
                                                         double lr, double mu, double wd, double max_norm, const double* __restrict__ partial,
                                                         double* __restrict__ norm_out) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kThreads / 64];
    double s = 0.0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kThreads) s += partial[b];  // (the grid of k_sgd_partial is this grid)
    const double norm = sqrt(block_sum(s, s_wave));
    const double c = max_norm / (norm + 1e-6);
    const double coef = c < 1.0 ? c : (c != c ? c : 1.0);  // clamp(max=1) that keeps a NaN, as torch's does
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < N; k += stride) {
        const double pk = (double)p[k];
        const double gk = coef * (double)g[k] + wd * pk;
        const double bk = mu * (double)buf[k] + gk;
        buf[k] = (float)bk;
        p[k] = (float)(pk - lr * bk);
    }
}

}  // namespace pvt
