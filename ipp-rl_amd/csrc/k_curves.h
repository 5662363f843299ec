// Planner-comparison curves on the device (experiments/experiments.py:194-236 of the reference: every run's metric against its
// cumulative flight time, resampled onto one axis, mean and spread over the runs).  The kernels:
//   k_curve_record    one thread per env: appends (cumulative flight time, the 8 metrics) to the env's log [T_cap][9]; a full log sets
//                     the env's overflow flag and drops the point
//   k_curve_extent    one workgroup: max over the envs of the last recorded time
//   k_curve_resample  one workgroup per env, threads over the grid points: np.interp by a binary search in the env's times
//   k_curve_reduce    one workgroup per grid point: mean and sd (ddof = 1) over the envs, summed in a FIXED order (thread slot s takes
//                     the envs s, s + 32, ... in ascending order, the 32 slots are folded pairwise 16, 8, 4, 2, 1): same bits every run
// fp64 throughout, no fused multiply-adds, no atomics.
#pragma once
#include "ipp_common.h"

namespace ipp {
namespace cv {

constexpr int kPoint = IPP_CURVE_POINT;    // doubles per log entry: time + the metrics
constexpr int kValues = IPP_CURVE_VALUES;  // metrics per entry (ipp_metrics)
constexpr int kSlots = 32;                 // env slots of a reduce workgroup (256 threads = 32 slots x 8 values)

struct RecordArgs {
    int n, first, t_cap;
    double vmax, amax;
    const float* metrics;          // [n][8]
    const double* action;          // [n][3]
    const double* prev_before;     // [n][3]
    const unsigned char* executed; // [n]
    double* log;                   // [n][t_cap][9]
    int* count;                    // [n]
    unsigned char* overflow;       // [n]
};

__global__ __launch_bounds__(256) void k_curve_record(RecordArgs a) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n) return;
    if (!a.first && !a.executed[e]) return;
    const int c = a.count[e];
    if (c < 0 || c >= a.t_cap) { a.overflow[e] = 1; return; }
    double dt = 0.0;
    if (!a.first) {  // compute_flight_time (planning/common/actions.py:32-41), whatever the engine's cost mode
        const double dx = a.action[3 * e + 0] - a.prev_before[3 * e + 0], dy = a.action[3 * e + 1] - a.prev_before[3 * e + 1],
                     dz = a.action[3 * e + 2] - a.prev_before[3 * e + 2];
        const double dist = sqrt(dx * dx + dy * dy + dz * dz);
        const double d_acc = fmin(dist * 0.5, a.vmax * a.vmax / (2 * a.amax));
        dt = (dist - 2 * d_acc) / a.vmax + 2 * sqrt(2 * d_acc / a.amax);
    }
    double* row = a.log + ((size_t)e * a.t_cap + c) * kPoint;
    row[0] = c > 0 ? row[-kPoint] + dt : dt;  // (np.cumsum: one rounded sum per point)
#pragma unroll
    for (int v = 0; v < kValues; ++v) row[1 + v] = (double)a.metrics[(size_t)e * kValues + v];
    a.count[e] = c + 1;
}

// LDS: double[256]
__global__ __launch_bounds__(256) void k_curve_extent(int n, int t_cap, const double* __restrict__ log, const int* __restrict__ count,
                                                      double* __restrict__ max_x_all) {
    __shared__ double s_max[256];
    const int tid = threadIdx.x;
    double m = 0.0;
    for (int e = tid; e < n; e += 256) {
        const int c = min(count[e], t_cap);
        if (c > 0) m = fmax(m, log[((size_t)e * t_cap + (c - 1)) * kPoint]);
    }
    s_max[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) s_max[tid] = fmax(s_max[tid], s_max[tid + s]);
        __syncthreads();
    }
    if (tid == 0) *max_x_all = s_max[0];
}

// out[e][g][v] = np.interp(x_g, xs_e, ys_e[:, v]); x_g = g step, the last grid point max_x itself (np.linspace(0, max_x, G)); G == 1: x_0 = 0.
// j = the largest index with xs[j] <= x; j == last: ys[last]; x < xs[0]: ys[0]; else slope dx + ys[j].  An empty log: NaN.
__global__ __launch_bounds__(256) void k_curve_resample(int t_cap, int G, double step, double max_x, const double* __restrict__ log,
                                                        const int* __restrict__ count, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int e = blockIdx.x;
    const int n = min(count[e], t_cap);
    const double* rows = log + (size_t)e * t_cap * kPoint;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        double* o = out + ((size_t)e * G + g) * kValues;
        if (n <= 0) {
#pragma unroll
            for (int v = 0; v < kValues; ++v) o[v] = __longlong_as_double(0x7ff8000000000000ll);
            continue;
        }
        const double x = (g == G - 1 && G > 1) ? max_x : (double)g * step;
        // invariant: xs[lo] <= x (or lo == 0) and xs[hi] > x (or hi == n)
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rows[(size_t)mid * kPoint] <= x) lo = mid; else hi = mid;
        }
        const double* r0 = rows + (size_t)lo * kPoint;
        if (lo == n - 1 || !(r0[0] <= x)) {
#pragma unroll
            for (int v = 0; v < kValues; ++v) o[v] = r0[1 + v];
            continue;
        }
        const double* r1 = r0 + kPoint;
        const double dx = x - r0[0], w = r1[0] - r0[0];
#pragma unroll
        for (int v = 0; v < kValues; ++v) {
            const double slope = (r1[1 + v] - r0[1 + v]) / w;
            o[v] = slope * dx + r0[1 + v];
        }
    }
}

// LDS: double[256]
__global__ __launch_bounds__(256) void k_curve_reduce(int n, int G, const double* __restrict__ per_env, double* __restrict__ mean,
                                                      double* __restrict__ sd) {
#pragma clang fp contract(off)
    __shared__ double s_sum[kSlots * kValues];
    const int g = blockIdx.x, tid = threadIdx.x, v = tid & (kValues - 1), slot = tid / kValues;
    double acc = 0.0;
    for (int e = slot; e < n; e += kSlots) acc += per_env[((size_t)e * G + g) * kValues + v];
    s_sum[tid] = acc;
    __syncthreads();
    for (int s = kSlots / 2; s > 0; s >>= 1) {
        if (slot < s) s_sum[tid] += s_sum[tid + s * kValues];
        __syncthreads();
    }
    const double mu = s_sum[v] / (double)n;
    __syncthreads();
    acc = 0.0;
    for (int e = slot; e < n; e += kSlots) {
        const double d = per_env[((size_t)e * G + g) * kValues + v] - mu;
        acc += d * d;
    }
    s_sum[tid] = acc;
    __syncthreads();
    for (int s = kSlots / 2; s > 0; s >>= 1) {
        if (slot < s) s_sum[tid] += s_sum[tid + s * kValues];
        __syncthreads();
    }
    if (slot == 0) {
        mean[(size_t)g * kValues + v] = mu;
        sd[(size_t)g * kValues + v] = n > 1 ? sqrt(s_sum[v] / (double)(n - 1)) : 0.0;
    }
}

}  // namespace cv
}  // namespace ipp
