// Batched self-play on the device (planning/mcts_zero/episode_generators.py:102-184 for every env at once) and the replay
// buffer's minibatch (planning/mcts_zero/replay_buffers.py:58-101).  The kernels:
//   k_sp_record   one wave per env: the read-out's post-processing (one-hot arg-max for temperature 0, mcts.py:134-138), the
//                 inverse-CDF draw of np.random.choice(len(policy), p=policy) (:135), the waypoint, the sparse policy / valid set into
//                 the env's ring row, and the episode end of a root without a policy (`policy is None: break`, :130-131)
//   k_sp_commit   one wave per env: the step's reward into its row; for every env whose episode ended the windowed value targets of
//                 all its rows in fp64 (:158-164), the committed flags, the episode's value, the next episode's first waypoint
//                 (sample_init_action, :51, :60-62) and the next step's tie-break uniform
//   k_sp_commit_iter  the same body with the iteration rule of the learn loop (mcts_zero_mission.py:320-340; k_learn.h holds the rest):
//                 an env keeps episode_cap episodes per iteration, their rows tagged with it; later ones are dropped
//   k_sp_gather   store-bound: minibatch rows drawn uniformly from the committed ones, planes shifted by ReplicationPad2d(4) +
//                 RandomCrop (one offset per augmented copy), policies and masks densified to [A]; k_sp_gather_rows: the same rows
//                 for a given index array (the prioritised sampler, k_replay_per.h)
// Every draw is a Philox4x32-10 uniform keyed on the GLOBAL env id (include/ipp_engine.h, IPP_SP_*_STREAM), so shards agree.
#pragma once
#include "ipp_common.h"

namespace ipp {

constexpr int kSpMaxK = 2048;  // widest valid set a ring row holds (dynamic LDS of the record / gather kernels: 12 / 8 bytes per slot)
constexpr uint8_t kSpPending = 1, kSpCommitted = 2;

// Philox4x32-10 of (counter q, subsequence) under `seed`, word 0 as (c + 0.5) / 2^32 (vec_env.philox_uniform on the host)
__device__ __forceinline__ double sp_uniform(uint64_t q, uint64_t subseq, uint64_t seed) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)subseq, (uint32_t)(subseq >> 32)};
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int r = 0; r < 10; ++r) philox_round(c, key);
    return ((double)c[0] + 0.5) * (1.0 / 4294967296.0);
}

// counter of the per-step draws of an env: (global env id, depth in the episode); the episode is the subsequence offset
__device__ __forceinline__ uint64_t sp_step_counter(long long gid, int depth) { return ((uint64_t)gid << 20) + (uint64_t)depth; }

// gamma^j of the discounted sums (episode_generators.py:158, :163; arenas.py:38): one convention for the value targets and the arena's returns
__device__ __forceinline__ double sp_discount(double gamma, int j) { return pow(gamma, (double)j); }

// an env's step without a sample (no policy, or none with mass): a zero budget ends the episode inside the step launch (a reset exactly
// like a budget end), the action is the current waypoint (no cost).  The row's planes were overwritten for this step: it is no longer
// a committed sample; its earlier policy and valid set stay as they were.
__device__ __forceinline__ void sp_end_without_sample(const ipp_selfplay& sp, int e, size_t row) {
    sp.forced[e] = 1;
    sp.budget[e] = 0.0;
    for (int c = 0; c < 3; ++c) sp.action[3 * e + c] = sp.prev[3 * e + c];
    sp.action_idx[e] = -1;
    sp.r_flags[row] = 0;
}

__global__ __launch_bounds__(64) void k_sp_record(ipp_selfplay sp, long long step, const double* __restrict__ pol_t,
                                                  const double* __restrict__ pol_1, const int32_t* __restrict__ vidx,
                                                  const int32_t* __restrict__ ok) {
#pragma clang fp contract(off)
    extern __shared__ double sp_lds[];
    const int kmax = sp.kmax;
    double* s_p = sp_lds;
    int32_t* s_i = reinterpret_cast<int32_t*>(sp_lds + kmax);
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= sp.num_envs) return;
    const size_t row = (size_t)(step % sp.slots) * sp.num_envs + e;
    if (!ok[e]) {  // no policy: no sample
        if (lane == 0) sp_end_without_sample(sp, e, row);
        return;
    }
    const int depth = sp.depth[e];
    const long long ep = sp.episode[e], gid = (long long)e + sp.row_offset;
    const bool t0 = sp.temp_zero || depth >= sp.temp_threshold;
    const double* src = (t0 ? pol_1 : pol_t) + (size_t)e * kmax;
    const int32_t* vi = vidx + (size_t)e * kmax;
    double vmax = -INFINITY;
    bool has_nan = false;
    for (int k = lane; k < kmax; k += 64) {
        const int32_t a = vi[k];
        const double p = a >= 0 ? src[k] : 0.0;
        s_p[k] = p;
        s_i[k] = a;
        if (a >= 0) vmax = fmax(vmax, p);
        has_nan |= p != p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o, 64));
    __syncthreads();
    // ok[] promises a policy with mass on the valid set.  One that has none (an empty valid set, all zeros, a NaN, an infinity) is no
    // sample: np.random.choice raises on it; here the env ends like a root without a policy
    if (__any(has_nan) || !(vmax > 0.0) || vmax == INFINITY) {
        if (lane == 0) sp_end_without_sample(sp, e, row);
        return;
    }
    if (t0) {
        // np.random.choice among the most visited actions (ascending action order), from a counter-based uniform
        int n_ties = 0, best = -1;
        for (int k0 = 0; k0 < kmax; k0 += 64) {
            const int k = k0 + lane;
            n_ties += __popcll(__ballot(k < kmax && s_i[k] >= 0 && s_p[k] == vmax));
        }
        const double u = sp_uniform(sp_step_counter(gid, depth), IPP_SP_ARGMAX_STREAM + (uint64_t)ep, sp.seed);
        long long pick = (long long)(u * (double)n_ties);
        pick = pick < n_ties - 1 ? pick : n_ties - 1;
        int seen = 0;
        for (int k0 = 0; k0 < kmax && best < 0; k0 += 64) {
            const int k = k0 + lane;
            unsigned long long b = __ballot(k < kmax && s_i[k] >= 0 && s_p[k] == vmax);
            const int c = __popcll(b);
            if (pick < seen + c) {
                for (int r = (int)pick - seen; r > 0; --r) b &= b - 1;  // drop the r lowest ties
                best = k0 + (int)__ffsll((long long)b) - 1;
            }
            seen += c;
        }
        __syncthreads();
        for (int k = lane; k < kmax; k += 64) s_p[k] = (k == best) ? 1.0 : 0.0;
        __syncthreads();
    }
    int a = -1;
    if (lane == 0) {
        // inverse CDF in ascending action order: cdf = cumsum(p) / sum(p), the first k with cdf[k] > u (NumPy's sequential cumsum; the
        // actions outside the valid set have p = 0 and leave every partial sum as it is)
        double tot = 0.0;
        for (int k = 0; k < kmax; ++k)
            if (s_i[k] >= 0) tot += s_p[k];
        const double u = sp_uniform(sp_step_counter(gid, depth), IPP_SP_ACTION_STREAM + (uint64_t)ep, sp.seed);
        double c = 0.0;
        int pick = -1, last = 0;
        for (int k = 0; k < kmax; ++k) {
            if (s_i[k] < 0) continue;
            c += s_p[k];
            if (s_p[k] > 0.0) last = k;
            if (c / tot > u) { pick = k; break; }
        }
        if (pick < 0) pick = last;  // (cdf[-1] / cdf[-1] == 1 > u: not reached)
        a = s_i[pick];
        if (!(tot > 0.0) || !(tot < INFINITY) || a >= sp.num_actions) a = -1;  // (a sum without mass; a valid index that is no action)
    }
    a = __shfl(a, 0, 64);
    if (a < 0) {
        if (lane == 0) sp_end_without_sample(sp, e, row);
        return;
    }
    // the sparse sample: fp32 probabilities and the valid indices on the row's kmax slots
    for (int k = lane; k < kmax; k += 64) {
        sp.r_policy[row * kmax + k] = (float)s_p[k];
        sp.r_idx[row * kmax + k] = s_i[k];
    }
    if (lane == 0) {
        sp.action_idx[e] = a;
        for (int q = 0; q < 3; ++q) sp.action[3 * e + q] = sp.actions[3 * (size_t)a + q];
        sp.r_flags[row] = kSpPending;
        sp.ep_len[e] += 1;
        sp.forced[e] = 0;
    }
}

// The commit of env e by its wave.  ITER = false: k_sp_commit.  ITER = true: k_sp_commit_iter, the same with the iteration rule of
// ipp_selfplay_commit_iter (include/ipp_engine.h): an episode past the env's cap is dropped, a kept one tags its rows and counts;
// `it` is read in that instantiation only.
template <bool ITER>
__device__ __forceinline__ void sp_commit_body(const ipp_selfplay& sp, long long step, const ipp_selfplay_iter* it) {
#pragma clang fp contract(off)
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= sp.num_envs) return;
    const int B = sp.num_envs, S = sp.slots;
    const bool forced = sp.forced[e] != 0;
    const double r_now = (double)sp.reward[e];
    if (!forced && lane == 0) sp.r_reward[(size_t)(step % S) * B + e] = r_now;
    const bool ended = forced || sp.done[e] != 0;
    const long long ep = sp.episode[e], gid = (long long)e + sp.row_offset;
    if (ended) {
        const int T = sp.ep_len[e];
        const long long t_last = forced ? step - 1 : step;
        auto row_of = [&](int j) { return (size_t)((t_last - (T - 1 - j)) % S) * B + e; };
        auto r_of = [&](int j) { return (j == T - 1 && !forced) ? r_now : sp.r_reward[row_of(j)]; };
        bool keep = true;
        if constexpr (ITER) keep = it->iter_episodes[e] < it->episode_cap;  // (every lane reads it before lane 0 counts the episode)
        // value_i = sum_{j = i}^{min(i + horizon, T) - 1} gamma^j r_j: the ABSOLUTE step j as exponent (episode_generators.py:163)
        for (int i = lane; i < T; i += 64) {
            if constexpr (ITER) {
                if (!keep) {  // past the cap: the episode is played out but leaves no sample
                    sp.r_flags[row_of(i)] = 0;
                    continue;
                }
            }
            const int hi = min(i + sp.horizon, T);
            double v = 0.0;
            for (int j = i; j < hi; ++j) v += sp_discount(sp.gamma, j) * r_of(j);
            const size_t r = row_of(i);
            sp.r_value[r] = sqrt(1.0 + v) - 1.0;  // scale_value_target (planning/common/rewards.py)
            if constexpr (ITER) it->r_iter[r] = it->iteration;
            sp.r_flags[r] = kSpCommitted;          // (behind its target: a row becomes sampleable with its value written)
        }
        if (lane == 0) {
            double tot = 0.0;  // total_episode_value (:158)
            for (int j = 0; j < T; ++j) tot += sp_discount(sp.gamma, j) * r_of(j);
            sp.episode_value[e] = tot;
            sp.ep_len[e] = 0;
            if constexpr (ITER) {
                if (keep) {
                    it->examples[e] += T;
                    it->value_sum[e] += tot;
                }
                it->iter_episodes[e] += 1;  // (also for T = 0: an env that can never move does not stall the iteration)
            }
            if (sp.random_init) {  // the episode the step's reset started: its first waypoint, uniform over the action set
                const double u = sp_uniform((uint64_t)gid, IPP_SP_INIT_STREAM + (uint64_t)ep, sp.seed);
                int a = (int)(u * (double)sp.num_actions);
                a = a < sp.num_actions - 1 ? a : sp.num_actions - 1;
                for (int q = 0; q < 3; ++q) sp.prev[3 * e + q] = sp.actions[3 * (size_t)a + q];
            }
        }
    } else if (lane == 0) {
        sp.episode_value[e] = __longlong_as_double(0x7ff8000000000000ll);  // NaN: no episode of this env ended
    }
    if (lane == 0) {
        sp.forced[e] = 0;
        sp.tie_u[e] = sp_uniform(sp_step_counter(gid, sp.depth[e]), IPP_SP_TIE_STREAM + (uint64_t)ep, sp.seed);
    }
}

__global__ __launch_bounds__(64) void k_sp_commit(ipp_selfplay sp, long long step) { sp_commit_body<false>(sp, step, nullptr); }

// the commit of a self-play iteration (mcts_zero_mission.py:320-340: num_episodes episodes per worker, here episode_cap per env)
__global__ __launch_bounds__(64) void k_sp_commit_iter(ipp_selfplay sp, long long step, ipp_selfplay_iter it) {
    sp_commit_body<true>(sp, step, &it);
}

// Minibatch row of draw i: the floor(u total)-th committed row (cum = inclusive prefix count of the committed flags), -1 when
// nothing is committed
__device__ __forceinline__ long long sp_draw_row(const int32_t* __restrict__ cum, long long cap, int i, uint64_t subseq, uint64_t seed) {
    const long long total = cum[cap - 1];
    if (total <= 0) return -1;
    const double u = sp_uniform((uint64_t)i, subseq, seed);
    long long r = (long long)(u * (double)total);
    r = r < total - 1 ? r : total - 1;
    long long lo = 0, hi = cap - 1;  // the first row with cum > r
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// shift offset (i, j) in [0, 8]^2 of augmented copy c >= 1, shared by the copy's whole batch (copy 0: the originals, (4, 4) = no shift)
__device__ __forceinline__ int sp_offset(int c, int which, uint64_t subseq, uint64_t seed) {
    if (c == 0) return 4;
    const double u = sp_uniform((1ull << 32) + 2ull * (uint64_t)c + (uint64_t)which, subseq, seed);
    const int o = (int)(u * 9.0);
    return o < 8 ? o : 8;
}

struct SpGather {
    int n, copies, C, side, A, kmax;
    long long cap;
    const int32_t* cum;
    const float* planes;  // [cap][C][side][side] or NULL (C = 0)
    uint64_t seed, subseq;
    float* states; float* policy; uint8_t* mask; double* value; double* reward; int64_t* index; int32_t* offsets;
};

// channel ch of output row o: ring row `row` shifted by the offset (oi, oj) (NaN when row < 0)
__device__ __forceinline__ void sp_gather_plane(const SpGather& g, long long row, int o, int ch, int oi, int oj) {
    const int N = g.side, dy = oi - 4, dx = oj - 4;
    const size_t NN = (size_t)N * N;
    float* dst = g.states + ((size_t)o * g.C + ch) * NN;
    if (row < 0) {
        for (size_t q = threadIdx.x; q < NN; q += blockDim.x) dst[q] = __int_as_float(0x7fc00000);
        return;
    }
    const float* src = g.planes + ((size_t)row * g.C + ch) * NN;
    // out[y][x] = in[clamp(y + i - 4)][clamp(x + j - 4)]: ReplicationPad2d(4), then the crop at (i, j)
    if ((N & 3) == 0) {  // (rows of a multiple of 4 floats: 16-byte stores, 16-byte loads where the row is not shifted)
        for (size_t q = 4 * (size_t)threadIdx.x; q < NN; q += 4 * (size_t)blockDim.x) {
            const int y = (int)(q / N), x = (int)(q % N);
            const int sy = min(max(y + dy, 0), N - 1);
            const float* srow = src + (size_t)sy * N;
            float4 v;
            if (dx == 0) {
                v = *reinterpret_cast<const float4*>(srow + x);
            } else {
                v.x = srow[min(max(x + dx, 0), N - 1)];
                v.y = srow[min(max(x + 1 + dx, 0), N - 1)];
                v.z = srow[min(max(x + 2 + dx, 0), N - 1)];
                v.w = srow[min(max(x + 3 + dx, 0), N - 1)];
            }
            *reinterpret_cast<float4*>(dst + q) = v;
        }
    } else {
        for (size_t q = threadIdx.x; q < NN; q += blockDim.x) {
            const int y = (int)(q / N), x = (int)(q % N);
            dst[q] = src[(size_t)min(max(y + dy, 0), N - 1) * N + min(max(x + dx, 0), N - 1)];
        }
    }
}

// output row o from ring row `row`: dense policy and mask over the A actions from the row's ascending valid set (-1 padding at the end),
// value and reward (zeros / NaN when row < 0).  lds: kmax floats + kmax int32, s_k: one int of LDS
__device__ __forceinline__ void sp_gather_sample(const ipp_selfplay& sp, const SpGather& g, long long row, int o, double* lds, int* s_k) {
    const int kmax = g.kmax;
    float* s_p = reinterpret_cast<float*>(lds);
    int32_t* s_i = reinterpret_cast<int32_t*>(lds) + kmax;
    if (threadIdx.x == 0) *s_k = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < kmax; k += blockDim.x) {
        const int32_t a = row >= 0 ? sp.r_idx[(size_t)row * kmax + k] : -1;
        s_i[k] = a;
        s_p[k] = row >= 0 ? sp.r_policy[(size_t)row * kmax + k] : 0.0f;
        if (a >= 0) atomicMax(s_k, k + 1);
    }
    __syncthreads();
    const int K = *s_k;
    float* pol = g.policy + (size_t)o * g.A;
    uint8_t* msk = g.mask + (size_t)o * g.A;
    for (int a = threadIdx.x; a < g.A; a += blockDim.x) {
        int lo = 0, hi = K;  // the first valid slot with index >= a
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_i[mid] < a) lo = mid + 1; else hi = mid;
        }
        const bool hit = lo < K && s_i[lo] == a;
        pol[a] = hit ? s_p[lo] : 0.0f;
        msk[a] = hit ? 1 : 0;
    }
    if (threadIdx.x == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        g.value[o] = row >= 0 ? sp.r_value[row] : nan;
        g.reward[o] = row >= 0 ? sp.r_reward[row] : nan;
    }
}

// block b: output row o = b / (C + 1) (draw o % n of copy o / n), channel b % (C + 1); channel C = the row's policy, mask, value,
// reward and index
__global__ __launch_bounds__(256) void k_sp_gather(ipp_selfplay sp, SpGather g) {
    extern __shared__ double sp_lds[];
    __shared__ int s_k;
    const long long b = blockIdx.x;
    const int o = (int)(b / (g.C + 1)), ch = (int)(b % (g.C + 1));
    const int copy = o / g.n, i = o % g.n;
    const long long row = sp_draw_row(g.cum, g.cap, i, g.subseq, g.seed);
    const int oi = sp_offset(copy, 0, g.subseq, g.seed), oj = sp_offset(copy, 1, g.subseq, g.seed);
    if (ch < g.C) {
        sp_gather_plane(g, row, o, ch, oi, oj);
        return;
    }
    sp_gather_sample(sp, g, row, o, sp_lds, &s_k);
    if (threadIdx.x == 0) {
        g.index[o] = row;
        if (i == 0) { g.offsets[2 * copy] = oi; g.offsets[2 * copy + 1] = oj; }
    }
}

// The same minibatch for given ring rows (rows[o]; outside [0, cap): an empty row, NaN), unshifted: the prioritised sampler's gather
// (k_replay_per.h draws the rows).  block b: output row b / (C + 1), channel b % (C + 1) as above
__global__ __launch_bounds__(256) void k_sp_gather_rows(ipp_selfplay sp, SpGather g, const int64_t* __restrict__ rows) {
    extern __shared__ double sp_lds[];
    __shared__ int s_k;
    const long long b = blockIdx.x;
    const int o = (int)(b / (g.C + 1)), ch = (int)(b % (g.C + 1));
    long long row = rows[o];
    if (row < 0 || row >= g.cap) row = -1;
    if (ch < g.C) sp_gather_plane(g, row, o, ch, 4, 4);
    else sp_gather_sample(sp, g, row, o, sp_lds, &s_k);
}

}  // namespace ipp
