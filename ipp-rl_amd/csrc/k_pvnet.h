// Kernels of the policy-value network's inference (include/ipp_engine.h "Policy-value network"; the plan: planning/mcts_zero/networks.py).
//
//   k_pv_conv   every convolution of the network as ONE implicit GEMM: M = batch x output pixels, N = output channels,
//               K = kh x kw x input channels (tap-major, channel-minor: contiguous in the channel-innermost activations).  A 64 x 64
//               output tile per workgroup of four waves, K in chunks of 32 gathered into LDS (padding, stride and every tail as
//               zeros in the gather), a 32 x 32 quadrant = 2 x 2 MFMA accumulators per wave; bias, residual and activation in the
//               epilogue.  fp32: mfma_f32_16x16x4f32, a k-ordered f32 fma chain per output element whose order depends on K alone,
//               so a sample's result does not depend on the batch around it.  bf16: mfma_f32_16x16x32_bf16, activations rounded
//               (nearest even) on the way into LDS, weights once at upload; accumulators and stored activations stay fp32.
//   k_pv_mix    the pooled part of MixGlobalContext, one workgroup per sample, in place.
//   k_pv_heads  one workgroup per sample: average / maximum pool of a head trunk; the value head; the policy head on the leaf's
//               valid actions only.
//
// The sparse policy equals the reference's exp(log_softmax(logits - 1000 (1 - mask))) on the valid set whenever the logits of a
// sample span less than about 900: an invalid action's term exp(-1000 + span) is then 0 in fp32 and the dense normaliser is the sum
// over the valid set.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pv {

constexpr int kBM = 64, kBN = 64, kBK = 32, kThreads = 256;
constexpr int kActNone = 0, kActRelu = 1, kActSilu = 2;

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;

__device__ __forceinline__ float activate(float v, int act) {
    if (act == kActRelu) return fmaxf(v, 0.f);
    if (act == kActSilu) return v / (1.f + expf(-v));
    return v;
}

// float -> bfloat16 bits, round to nearest even (no NaN payload care: activations and weights are finite)
__device__ __host__ __forceinline__ unsigned short to_bf16(float f) {
    unsigned u = __builtin_bit_cast(unsigned, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

struct ConvArgs {
    const float* in;            // [n][hin][win][cin], or the planes [n][cin][hin][win] (in_nchw)
    const void* w;              // [cout][kh][kw][cin] float or bf16 bits
    const float* bias;          // [cout]
    const float* res;           // [n][hout][wout][cout] or null
    float* out;                 // [n][hout][wout][cout]
    long long M;                // n * hout * wout
    int K, cin, cout, hin, win, hout, wout, kh, kw, stride, pad_h, pad_w, act, in_nchw;
};

template <bool BF16>
__global__ __launch_bounds__(kThreads) void k_pv_conv(ConvArgs a) {
    using lds_t = typename std::conditional<BF16, unsigned short, float>::type;
    constexpr int kLd = BF16 ? kBK + 8 : kBK + 1;  // bf16: 80-byte rows keep the 16-byte fragment reads aligned
    __shared__ __attribute__((aligned(16))) lds_t As[kBM][kLd];
    __shared__ __attribute__((aligned(16))) lds_t Bs[kBN][kLd];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int kl = t & 31, r0 = t >> 5;  // this thread gathers column kl of rows r0 + 8 j
    const long long m0 = (long long)blockIdx.x * kBM;
    const int n0 = blockIdx.y * kBN;
    const int hw_out = a.hout * a.wout;

    // the eight output pixels whose operand rows this thread gathers (constant over K)
    int iy0[8], ix0[8];
    long long base[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long long m = m0 + r0 + 8 * j;
        if (m < a.M) {
            const long long b = m / hw_out;
            const int p = (int)(m - b * hw_out), oy = p / a.wout, ox = p - oy * a.wout;
            iy0[j] = oy * a.stride - a.pad_h;
            ix0[j] = ox * a.stride - a.pad_w;
            base[j] = b * (long long)a.hin * a.win * a.cin;
        } else {
            iy0[j] = -(1 << 20);  // every tap falls outside: zeros
            ix0[j] = 0;
            base[j] = 0;
        }
    }

    float ra[8], rb[8];
    auto gather = [&](int k0) {
        const int k = k0 + kl;
        const bool kin = k < a.K;
        const int tap = kin ? k / a.cin : 0, ci = kin ? k - tap * a.cin : 0, ky = tap / a.kw, kx = tap - ky * a.kw;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int iy = iy0[j] + ky, ix = ix0[j] + kx;
            float v = 0.f;
            if (kin && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) {
                const long long off = a.in_nchw ? ((long long)ci * a.hin + iy) * a.win + ix : ((long long)iy * a.win + ix) * a.cin + ci;
                v = a.in[base[j] + off];
            }
            ra[j] = v;
            const int n = n0 + r0 + 8 * j;
            float w = 0.f;
            if (kin && n < a.cout) {
                const long long off = (long long)n * a.K + k;
                if constexpr (BF16) w = __builtin_bit_cast(float, (unsigned)static_cast<const unsigned short*>(a.w)[off] << 16);
                else w = static_cast<const float*>(a.w)[off];
            }
            rb[j] = w;
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32, lr = lane & 15, lq = lane >> 4;

    gather(0);
    for (int k0 = 0; k0 < a.K; k0 += kBK) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (BF16) {
                As[r0 + 8 * j][kl] = to_bf16(ra[j]);
                Bs[r0 + 8 * j][kl] = (unsigned short)(__builtin_bit_cast(unsigned, rb[j]) >> 16);  // (already bf16: exact)
            } else {
                As[r0 + 8 * j][kl] = ra[j];
                Bs[r0 + 8 * j][kl] = rb[j];
            }
        }
        __syncthreads();
        if (k0 + kBK < a.K) gather(k0 + kBK);
        if constexpr (BF16) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(&As[wm + 16 * i + lr][8 * lq]));
                fb[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(&Bs[wn + 16 * i + lr][8 * lq]));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int kk = 0; kk < kBK; kk += 4) {
                float fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = As[wm + 16 * i + lr][kk + lq];
                    fb[i] = Bs[wn + 16 * i + lr][kk + lq];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D map of the 16 x 16 forms: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + 16 * j + lr;
            if (n >= a.cout) continue;
            const float bias = a.bias[n];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm + 16 * i + 4 * lq + r;
                if (m >= a.M) continue;
                float v = acc[i][j][r] + bias;
                if (a.res) v += a.res[m * a.cout + n];
                a.out[m * a.cout + n] = activate(v, a.act);
            }
        }
}

// Mean and maximum over the P pixels of act(scale x + shift) (or of x: scale == null) for channels [0, G) of xs [P][C], by all threads
// of the workgroup: the pixels go to kThreads / G slices (one when G >= kThreads), then the slices are combined in slice order --
// a fixed order for given P and G, whatever the batch.  part: 2 * kThreads floats of LDS.  out[g] = mean, out[G + g] = maximum.
__device__ __forceinline__ void pool_channels(const float* __restrict__ xs, int P, int C, int G, const float* __restrict__ scale,
                                              const float* __restrict__ shift, int act, float* part, float* out) {
    const int t = threadIdx.x;
    const int slices = G >= kThreads ? 1 : kThreads / G;
    for (int g0 = 0; g0 < G; g0 += kThreads) {
        const int g = g0 + (slices == 1 ? t : t % G), sl = slices == 1 ? 0 : t / G;
        const bool on = g < G && sl < slices;
        float sum = 0.f, mx = -INFINITY;
        if (on) {
            const float s = scale ? scale[g] : 1.f, sh = scale ? shift[g] : 0.f;
            for (int p = sl; p < P; p += slices) {
                float v = xs[(size_t)p * C + g];
                if (scale) v = activate(v * s + sh, act);
                sum += v;
                mx = fmaxf(mx, v);
            }
            part[t] = sum;
            part[kThreads + t] = mx;
        }
        __syncthreads();
        if (on && sl == 0) {
            for (int i = 1; i < slices; ++i) {
                sum += part[i * G + (g - g0)];
                mx = fmaxf(mx, part[kThreads + i * G + (g - g0)]);
            }
            out[g] = sum / (float)P;
            out[G + g] = mx;
        }
        __syncthreads();
    }
}

// x [n][P][C] in place: pool act(scale x + shift) on channels [0, G) over the P pixels (mean, then maximum), ctx = act(fc [C - G][2 G]
// pooled + fcb), x[:, :, G:] += ctx.  Dynamic LDS: (2 G + C - G) floats.
__global__ __launch_bounds__(kThreads) void k_pv_mix(float* __restrict__ x, int P, int C, int G, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const float* __restrict__ fcw,
                                                      const float* __restrict__ fcb, int act) {
    extern __shared__ float lds[];
    __shared__ float part[2 * kThreads];
    float* pooled = lds;        // [2 G]
    float* ctx = lds + 2 * G;   // [C - G]
    float* xs = x + (size_t)blockIdx.x * P * C;
    const int t = threadIdx.x, R = C - G;
    pool_channels(xs, P, C, G, scale, shift, act, part, pooled);
    for (int c = t; c < R; c += kThreads) {
        float d = fcb[c];
        for (int i = 0; i < 2 * G; ++i) d = fmaf(fcw[(size_t)c * 2 * G + i], pooled[i], d);
        ctx[c] = activate(d, act);
    }
    __syncthreads();
    for (int i = t; i < P * R; i += kThreads) {
        const int p = i / R, c = i - p * R;
        xs[(size_t)p * C + G + c] += ctx[c];
    }
}

constexpr int kHeadPool = 0, kHeadValue = 1, kHeadPolicy = 2;

__device__ __forceinline__ double block_reduce(double v, double* red, bool is_max) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = is_max ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// mode kHeadPool:   x [n][P][C] -> pooled [n][2 C] (mean | maximum)
// mode kHeadValue:  value[b] = v^2 + 2 v, v = softplus(act(<w, pooled[b]> + bias))               (invert_scaled_value_target)
// mode kHeadPolicy: prior[b][k] = softmax over the slots k with 0 <= valid_idx[b][k] < A of bias[a] + <w[a, :], pooled[b]>; other
//                   slots (the -1 padding) and rows without a valid action get 0.  Dynamic LDS: kmax floats.
__global__ __launch_bounds__(kThreads) void k_pv_heads(int mode, const float* __restrict__ x, int P, int C, float* __restrict__ pooled,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int act, int A,
                                                        const int32_t* __restrict__ valid_idx, int kmax, double* __restrict__ prior,
                                                        double* __restrict__ value) {
    extern __shared__ float logit[];
    __shared__ double red[kThreads];
    const int b = blockIdx.x, t = threadIdx.x, C2 = 2 * C;
    float* pb = pooled + (size_t)b * C2;
    if (mode == kHeadPool) {
        const float* xs = x + (size_t)b * P * C;
        pool_channels(xs, P, C, C, nullptr, nullptr, 0, reinterpret_cast<float*>(red), pb);
        return;
    }
    if (mode == kHeadValue) {
        float d = 0.f;
        for (int i = t; i < C2; i += kThreads) d = fmaf(w[i], pb[i], d);
        const float z = activate((float)block_reduce((double)d, red, false) + bias[0], act);
        if (t == 0) {
            const double v = z > 20.f ? (double)z : log1p(exp((double)z));  // nn.Softplus (beta 1, threshold 20)
            value[b] = v * v + 2.0 * v;
        }
        return;
    }
    const int32_t* idx = valid_idx + (size_t)b * kmax;
    const int lane = t & 63, wave = t >> 6;
    for (int k = wave; k < kmax; k += kThreads / 64) {  // one wave per valid action: a row of 2 C weights
        const int aidx = idx[k];
        if (aidx < 0 || aidx >= A) continue;
        const float* wr = w + (size_t)aidx * C2;
        float d = 0.f;
        for (int i = lane; i < C2; i += 64) d = fmaf(wr[i], pb[i], d);
        for (int s = 32; s > 0; s >>= 1) d += __shfl_xor(d, s, 64);
        if (lane == 0) logit[k] = d + bias[aidx];
    }
    __syncthreads();
    double mx = -INFINITY;
    for (int k = t; k < kmax; k += kThreads)
        if (idx[k] >= 0 && idx[k] < A) mx = fmax(mx, (double)logit[k]);
    mx = block_reduce(mx, red, true);
    double sum = 0.0;
    for (int k = t; k < kmax; k += kThreads)
        if (idx[k] >= 0 && idx[k] < A) sum += exp((double)logit[k] - mx);
    sum = block_reduce(sum, red, false);
    for (int k = t; k < kmax; k += kThreads) {
        const bool ok = idx[k] >= 0 && idx[k] < A;
        prior[(size_t)b * kmax + k] = ok ? exp((double)logit[k] - mx) / sum : 0.0;
    }
}

// tap: [n][P][C] -> [n][C][P]
__global__ void k_pv_tap(const float* __restrict__ x, float* __restrict__ out, long long total, int P, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long b = i / ((long long)P * C);
    const int r = (int)(i - b * P * C), c = r / P, p = r - c * P;
    out[i] = x[(b * P + p) * C + c];
}

__global__ void k_pv_to_bf16(const float* __restrict__ src, unsigned short* __restrict__ dst, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = to_bf16(src[i]);
}

}  // namespace pv
