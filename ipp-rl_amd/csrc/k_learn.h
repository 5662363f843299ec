// The device pieces of the learn loop (planning/mcts_zero/mcts_zero_mission.py:254-398, `learn`) beside the iteration commit
// (k_sp_commit_iter, k_selfplay.h):
//   k_sp_iter_totals              one workgroup: the progress of a self-play iteration -- kept episodes, envs that have all theirs, kept
//                                 rows, the sum of the kept episodes' values -- as one 32-byte record: what the host reads per step to
//                                 know when `num_episodes` episodes per env are played (:320-340) and what the loop reports (:346-362)
//   k_per_count_win / _reset_win  k_per_count / k_per_reset (k_replay_per.h) on the rows whose iteration tag lies in [lo, hi]: the
//                                 off-policy window of ReplayBuffer(self_play_iteration, window_size), replay_buffers.py:34-46, as the
//                                 start priorities of a PrioritizedExperienceReplayBuffer (:119)
// fp64 in a fixed order, integer atomics only: the same inputs give the same bits in every run.
#pragma once
#include "ipp_common.h"
#include "k_replay_per.h"
#include "k_selfplay.h"

namespace ipp {

struct IterTotals {  // the record of ipp_selfplay_iter_totals
    long long episodes_kept, envs_at_cap, examples;
    double value_sum;
};
static_assert(sizeof(IterTotals) == 32, "ipp_selfplay_iter_totals' record is 32 bytes");

// Chunks of kPerThreads envs in ascending order: the chunk's value sums through per_block_scan (the order of k_per_scan_tiles), the
// chunks' totals added in chunk order; the integer sums per thread, then over the workgroup.
__global__ __launch_bounds__(kPerThreads) void k_sp_iter_totals(int num_envs, ipp_selfplay_iter it, IterTotals* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_wave[kPerThreads / 64];
    __shared__ long long s_int[3][kPerThreads / 64];
    double carry = 0.0;
    long long kept = 0, full = 0, rows = 0;
    for (int e0 = 0; e0 < num_envs; e0 += kPerThreads) {
        const int e = e0 + (int)threadIdx.x;
        double v = 0.0;
        if (e < num_envs) {
            const int n = it.iter_episodes[e];
            kept += n < it.episode_cap ? n : it.episode_cap;
            full += n >= it.episode_cap ? 1 : 0;
            rows += it.examples[e];
            v = it.value_sum[e];
        }
        double excl, total;
        per_block_scan(v, s_wave, &excl, &total);
        carry += total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kept += __shfl_xor(kept, o, 64);
        full += __shfl_xor(full, o, 64);
        rows += __shfl_xor(rows, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_int[0][threadIdx.x >> 6] = kept;
        s_int[1][threadIdx.x >> 6] = full;
        s_int[2][threadIdx.x >> 6] = rows;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long t[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q)
        for (int w = 0; w < kPerThreads / 64; ++w) t[q] += s_int[q][w];
    out->episodes_kept = t[0];
    out->envs_at_cap = t[1];
    out->examples = t[2];
    out->value_sum = carry;
}

// row r belongs to the window: committed and tagged with an iteration in [lo, hi]
__device__ __forceinline__ bool per_in_window(const uint8_t* __restrict__ flags, const int32_t* __restrict__ r_iter, long long r, int lo,
                                              int hi) {
    if (flags[r] != kSpCommitted) return false;
    const int32_t t = r_iter[r];
    return t >= lo && t <= hi;
}

__global__ __launch_bounds__(kPerThreads) void k_per_count_win(const uint8_t* __restrict__ flags, const int32_t* __restrict__ r_iter,
                                                               int lo, int hi, long long cap, unsigned long long* count) {
    const long long r = (long long)blockIdx.x * kPerThreads + threadIdx.x;
    const unsigned long long b = __ballot(r < cap && per_in_window(flags, r_iter, r, lo, hi));
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(kPerThreads) void k_per_reset_win(const uint8_t* __restrict__ flags, const int32_t* __restrict__ r_iter,
                                                               int lo, int hi, long long cap,
                                                               const unsigned long long* __restrict__ count,
                                                               double* __restrict__ priority) {
    const long long r = (long long)blockIdx.x * kPerThreads + threadIdx.x;
    if (r >= cap) return;
    priority[r] = per_in_window(flags, r_iter, r, lo, hi) ? 1.0 / (double)*count : 0.0;
}

}  // namespace ipp
