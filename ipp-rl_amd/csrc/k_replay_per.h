// Prioritised experience replay over the self-play ring (planning/mcts_zero/replay_buffers.py:104-141, PrioritizedExperienceReplayBuffer),
// on the device from the priorities to the minibatch.  Everything is fp64 and runs in a fixed order (no floating-point atomics), so the
// same ring and priorities give the same draws in every run.  Kernels:
//   k_per_count / k_per_reset   the committed count L (an integer atomic per wave) and priority = 1 / L on the committed rows, 0 elsewhere
//                               (:119)
//   k_per_mass_tile             mass[r] = priority[r]^alpha (:126) where row r is committed and its priority is finite and > 0, else 0; the
//                               mass into cum[r] and each tile's sum into tile_sum[tile]
//   k_per_scan_tiles            one workgroup: the exclusive prefix of the tile sums, in tile order
//   k_per_scan_rows             cum[r] <- the inclusive prefix mass of row r: its tile's offset + the scan inside the tile
//   k_per_draw                  one workgroup: draw i = the first row whose prefix mass exceeds u_i T (np.random.choice(L, p), :129, as
//                               cdf.searchsorted(u, side="right")), P_i from the row's own mass, w_i = (P_i L)^-beta over the minibatch's
//                               maximum, as float32 (:135-136)
//   k_per_update                priority[index[i]] = value[i], the last occurrence of a repeated index wins (NumPy's assignment, :141)
// The minibatch itself is k_sp_gather_rows (k_selfplay.h).
#pragma once
#include "ipp_common.h"
#include "k_selfplay.h"

namespace ipp {

constexpr int kPerThreads = 256;                      // workgroup of every kernel here: 4 waves
constexpr int kPerItems = IPP_REPLAY_SCAN_TILE / kPerThreads;  // consecutive rows per thread of a scan tile
static_assert(kPerItems * kPerThreads == IPP_REPLAY_SCAN_TILE, "scan tile");

// mass of ring row r (0 unless committed with a finite positive priority)
__device__ __forceinline__ double per_mass(const uint8_t* __restrict__ flags, const double* __restrict__ priority, long long r, double alpha) {
    if (flags[r] != kSpCommitted) return 0.0;
    const double p = priority[r];
    if (!(p > 0.0) || !(p < INFINITY)) return 0.0;  // (NaN fails both comparisons)
    return pow(p, alpha);
}

// Scan of one value per thread over the workgroup's kPerThreads threads in thread order: returns the inclusive prefix, *excl = the sum of
// the threads before, *total = the workgroup's sum.  The order of the additions is fixed: a shuffle scan inside each wave, then the
// waves' sums in wave order.  s_wave: 4 doubles of LDS.
__device__ __forceinline__ double per_block_scan(double v, double* s_wave, double* excl, double* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    const double before = __shfl_up(v, 1, 64);
    __syncthreads();  // (s_wave may still be read from an earlier call)
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < kPerThreads / 64; ++w) {
        if (w == wave) off = tot;
        tot += s_wave[w];
    }
    *total = tot;
    *excl = lane ? off + before : off;
    return off + v;
}

__global__ __launch_bounds__(kPerThreads) void k_per_count(const uint8_t* __restrict__ flags, long long cap, unsigned long long* count) {
    const long long r = (long long)blockIdx.x * kPerThreads + threadIdx.x;
    const unsigned long long b = __ballot(r < cap && flags[r] == kSpCommitted);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(kPerThreads) void k_per_reset(const uint8_t* __restrict__ flags, long long cap,
                                                           const unsigned long long* __restrict__ count, double* __restrict__ priority) {
    const long long r = (long long)blockIdx.x * kPerThreads + threadIdx.x;
    if (r >= cap) return;
    priority[r] = flags[r] == kSpCommitted ? 1.0 / (double)*count : 0.0;
}

// tile t = rows [t tile, (t + 1) tile): thread k holds rows t tile + k kPerItems + [0, kPerItems)
__global__ __launch_bounds__(kPerThreads) void k_per_mass_tile(const uint8_t* __restrict__ flags, const double* __restrict__ priority,
                                                               long long cap, double alpha, double* __restrict__ cum,
                                                               double* __restrict__ tile_sum) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kPerThreads / 64];
    const long long r0 = (long long)blockIdx.x * IPP_REPLAY_SCAN_TILE + (long long)threadIdx.x * kPerItems;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kPerItems; ++q) {
        const long long r = r0 + q;
        if (r < cap) {
            const double m = per_mass(flags, priority, r, alpha);
            cum[r] = m;
            s += m;
        }
    }
    double excl, total;
    per_block_scan(s, s_wave, &excl, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum[t] <- the sum of the tiles before t (one workgroup, chunks of kPerThreads tiles in order)
__global__ __launch_bounds__(kPerThreads) void k_per_scan_tiles(double* __restrict__ tile_sum, long long tiles) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kPerThreads / 64];
    double carry = 0.0;
    for (long long t0 = 0; t0 < tiles; t0 += kPerThreads) {
        const long long t = t0 + threadIdx.x;
        const double v = t < tiles ? tile_sum[t] : 0.0;
        double excl, total;
        per_block_scan(v, s_wave, &excl, &total);
        if (t < tiles) tile_sum[t] = carry + excl;
        carry += total;
    }
}

__global__ __launch_bounds__(kPerThreads) void k_per_scan_rows(long long cap, const double* __restrict__ tile_off, double* __restrict__ cum) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kPerThreads / 64];
    const long long r0 = (long long)blockIdx.x * IPP_REPLAY_SCAN_TILE + (long long)threadIdx.x * kPerItems;
    double m[kPerItems];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kPerItems; ++q) {
        m[q] = r0 + q < cap ? cum[r0 + q] : 0.0;
        s += m[q];
    }
    double excl, total;
    per_block_scan(s, s_wave, &excl, &total);
    double run = tile_off[blockIdx.x] + excl;  // the mass in front of this thread's rows
#pragma unroll
    for (int q = 0; q < kPerItems; ++q) {
        run += m[q];
        if (r0 + q < cap) cum[r0 + q] = run;
    }
}

struct PerDraw {
    int n;
    long long cap;
    const double* priority; const double* cum;
    double alpha, beta, L;
    uint64_t seed, subseq;
    int64_t* index; float* weight;
};

// Row of the uniform u: the first row whose inclusive prefix mass exceeds u T.  The prefix sums of neighbouring threads of the scan
// can differ in the last place, so the row found may have no mass: then the next row that has, else the last one before it.
__device__ __forceinline__ long long per_draw_row(const ipp_selfplay& sp, const PerDraw& d, double T, double u, double* mass) {
    const double x = u * T;
    long long lo = 0, hi = d.cap - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (d.cum[mid] > x) hi = mid; else lo = mid + 1;
    }
    double m = per_mass(sp.r_flags, d.priority, lo, d.alpha);
    if (!(m > 0.0)) {
        long long r = lo + 1;
        while (r < d.cap && !((m = per_mass(sp.r_flags, d.priority, r, d.alpha)) > 0.0)) ++r;
        if (r >= d.cap) {
            r = lo - 1;
            while (r >= 0 && !((m = per_mass(sp.r_flags, d.priority, r, d.alpha)) > 0.0)) --r;
        }
        lo = r;  // (-1: no row has mass, although T > 0 promised one)
    }
    *mass = m;
    return lo;
}

__global__ __launch_bounds__(kPerThreads) void k_per_draw(ipp_selfplay sp, PerDraw d) {
#pragma clang fp contract(off)
    __shared__ double s_max[kPerThreads / 64];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double T = d.cum[d.cap - 1];
    const bool any = T > 0.0 && T < INFINITY;
    // pass 1: the rows and the largest raw weight
    double wmax = 0.0;
    for (int i = threadIdx.x; i < d.n; i += kPerThreads) {
        long long row = -1;
        if (any) {
            double m;
            row = per_draw_row(sp, d, T, sp_uniform((uint64_t)i, d.subseq, d.seed), &m);
            if (row >= 0) wmax = fmax(wmax, pow(m / T * d.L, -d.beta));
        }
        d.index[i] = row;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = wmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kPerThreads / 64; ++w) wmax = fmax(wmax, s_max[w]);
    // pass 2: each thread's own rows again, the weights over the maximum
    for (int i = threadIdx.x; i < d.n; i += kPerThreads) {
        const long long row = d.index[i];
        double w = nan;
        if (row >= 0) w = pow(per_mass(sp.r_flags, d.priority, row, d.alpha) / T * d.L, -d.beta) / wmax;
        d.weight[i] = (float)w;
    }
}

// thread i writes value[i] unless index[i] is outside the ring (-1: an empty draw) or comes again later in the minibatch
__global__ __launch_bounds__(kPerThreads) void k_per_update(long long cap, int n, const int64_t* __restrict__ index,
                                                            const double* __restrict__ value, double* __restrict__ priority) {
    const int i = blockIdx.x * kPerThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t r = index[i];
    if (r < 0 || r >= cap) return;
    for (int j = i + 1; j < n; ++j)
        if (index[j] == r) return;
    priority[r] = value[i];
}

}  // namespace ipp
