// Playing with a trained network on the device: the decision of the deployment planner (planning/mcts_zero/mcts_zero_mission.py:516-523,
// replan: the root-parallel workers' policies summed, normalised, arg-max) and the game bookkeeping of the arena gate
// (planning/mcts_zero/arenas.py:32-45) for every env of a budget-mode batch at once.  The kernels:
//   k_play_pick    one wave per env: the ensemble of the env's `workers` search policies on the shared valid set, its normalisation, the
//                  arg-max (deploy: the first maximiser, np.argmax; arena: the temperature-0 choice among equal maxima, mcts.py:134-138,
//                  by the draw k_sp_record makes), the waypoint; an env without a usable policy ends its episode like
//                  sp_end_without_sample
//   k_play_tally   one wave per env: the running discounted return (arenas.py:38), the games that ended into the env's game list, the
//                  next step's tie-break uniform (as k_sp_commit)
//   k_play_totals  one workgroup: the arena's totals over the counted games in a fixed order
// fp64 in a fixed order, no atomics: the same inputs give the same bits in every run.  Draws as in k_selfplay.h (global env id).
#pragma once
#include "ipp_common.h"
#include "k_selfplay.h"

namespace ipp {

// an env's step without a decision: exactly sp_end_without_sample's ledger writes (there is no ring row here)
__device__ __forceinline__ void play_end_without_pick(const ipp_play& pl, int e) {
    pl.forced[e] = 1;
    pl.budget[e] = 0.0;
    for (int c = 0; c < 3; ++c) pl.action[3 * e + c] = pl.prev[3 * e + c];
    pl.action_idx[e] = -1;
}

// policy [B workers][kmax], vidx [B workers][kmax], ok [B workers]: root e workers + w is worker w of env e
__global__ __launch_bounds__(64) void k_play_pick(ipp_play pl, const double* __restrict__ policy, const int32_t* __restrict__ vidx,
                                                  const int32_t* __restrict__ ok) {
#pragma clang fp contract(off)
    extern __shared__ double pl_lds[];
    const int kmax = pl.kmax, W = pl.workers;
    double* s_p = pl_lds;
    int32_t* s_i = reinterpret_cast<int32_t*>(pl_lds + kmax);
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= pl.num_envs) return;
    const int32_t* okr = ok + (size_t)e * W;
    double* ens = pl.ensemble ? pl.ensemble + (size_t)e * kmax : nullptr;
    int w0 = -1;  // the first worker with a policy: its valid set is the env's (same waypoint, same budget)
    for (int w = 0; w < W; ++w)
        if (okr[w]) { w0 = w; break; }
    bool bad = w0 < 0;
    double tot = 0.0, vmax = -INFINITY;
    int best = -1, a = -1;
    if (!bad) {
        const int32_t* vi = vidx + ((size_t)e * W + w0) * kmax;
        bool has_nan = false;
        for (int k = lane; k < kmax; k += 64) {
            const int32_t ai = vi[k];
            double t = 0.0;  // policy_total[k] (:516-519): the workers in order
            if (ai >= 0)
                for (int w = 0; w < W; ++w)
                    if (okr[w]) t += policy[((size_t)e * W + w) * kmax + k];
            s_p[k] = t;
            s_i[k] = ai;
            has_nan |= t != t;
        }
        __syncthreads();
        if (lane == 0)  // np.sum in ascending action order (sequential, as k_sp_record forms `tot`)
            for (int k = 0; k < kmax; ++k)
                if (s_i[k] >= 0) tot += s_p[k];
        tot = __shfl(tot, 0, 64);
        bad = __any(has_nan) || !(tot > 0.0) || !(tot < INFINITY);
    }
    if (!bad) {
        for (int k = lane; k < kmax; k += 64) {  // policy_total /= np.sum(policy_total) (:521); a lane reads back only its own slots
            const double p = s_i[k] >= 0 ? s_p[k] / tot : 0.0;
            s_p[k] = p;
            if (s_i[k] >= 0) vmax = fmax(vmax, p);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o, 64));
        __syncthreads();
        bad = !(vmax > 0.0) || vmax == INFINITY;
    }
    if (!bad) {
        long long pick = 0;  // deploy: np.argmax, the first maximiser in ascending action order (:522)
        if (pl.tie_rule == 1) {
            // arena: np.random.choice among the maxima, the draw of k_sp_record's temperature-0 step
            int n_ties = 0;
            for (int k0 = 0; k0 < kmax; k0 += 64) {
                const int k = k0 + lane;
                n_ties += __popcll(__ballot(k < kmax && s_i[k] >= 0 && s_p[k] == vmax));
            }
            const long long gid = (long long)e + pl.row_offset;
            const double u = sp_uniform(sp_step_counter(gid, pl.depth[e]), IPP_SP_ARGMAX_STREAM + (uint64_t)pl.episode[e], pl.seed);
            pick = (long long)(u * (double)n_ties);
            pick = pick < n_ties - 1 ? pick : n_ties - 1;
        }
        int seen = 0;
        for (int k0 = 0; k0 < kmax && best < 0; k0 += 64) {
            const int k = k0 + lane;
            unsigned long long b = __ballot(k < kmax && s_i[k] >= 0 && s_p[k] == vmax);
            const int c = __popcll(b);
            if (pick < seen + c) {
                for (int r = (int)pick - seen; r > 0; --r) b &= b - 1;  // drop the r lowest maxima
                best = k0 + (int)__ffsll((long long)b) - 1;
            }
            seen += c;
        }
        a = best >= 0 ? s_i[best] : -1;
        bad = a < 0 || a >= pl.num_actions;  // (a valid index that is no action)
    }
    if (ens)
        for (int k = lane; k < kmax; k += 64) ens[k] = bad ? 0.0 : s_p[k];
    if (lane != 0) return;
    if (bad) {
        play_end_without_pick(pl, e);
        return;
    }
    pl.action_idx[e] = a;
    for (int q = 0; q < 3; ++q) pl.action[3 * e + q] = pl.actions[3 * (size_t)a + q];
    pl.forced[e] = 0;
}

__global__ __launch_bounds__(64) void k_play_tally(ipp_play pl) {
#pragma clang fp contract(off)
    const int e = blockIdx.x;
    if (e >= pl.num_envs || threadIdx.x != 0) return;
    const bool forced = pl.forced[e] != 0;
    double ret = pl.ret[e];
    int steps = pl.steps[e];
    if (!forced) {  // total_reward += gamma ** depth * reward (arenas.py:38); a forced step has no reward, as self-play gives it no row
        ret += sp_discount(pl.gamma, steps) * (double)pl.reward[e];
        steps += 1;
    }
    if (forced || pl.done[e] != 0) {
        const int G = pl.games_per_env, g = pl.games[e];
        if (g < G) {  // (an env that has its games plays on, uncounted)
            pl.game_value[(size_t)e * G + g] = ret;
            pl.game_steps[(size_t)e * G + g] = steps;
            pl.games[e] = g + 1;
        }
        ret = 0.0;
        steps = 0;
    }
    pl.ret[e] = ret;
    pl.steps[e] = steps;
    const long long gid = (long long)e + pl.row_offset;
    pl.tie_u[e] = sp_uniform(sp_step_counter(gid, pl.depth[e]), IPP_SP_TIE_STREAM + (uint64_t)pl.episode[e], pl.seed);
}

// out[0] = sum of the counted game values, out[1] = counted games, out[2] = sum of their steps, out[3] = envs that have all their games.
// Item i = e games_per_env + g; lane l adds the counted items l, l + 64, ... in ascending order, lane 0 adds the lanes' sums in lane order.
__global__ __launch_bounds__(64) void k_play_totals(ipp_play pl, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_v[64];
    __shared__ long long s_n[64], s_s[64], s_f[64];
    const int lane = threadIdx.x, G = pl.games_per_env;
    const long long n = (long long)pl.num_envs * G;
    double v = 0.0;
    long long cnt = 0, st = 0, full = 0;
    for (long long i = lane; i < n; i += 64) {
        const int e = (int)(i / G), g = (int)(i % G);
        if (g < pl.games[e]) {
            v += pl.game_value[i];
            st += pl.game_steps[i];
            cnt += 1;
        }
    }
    for (int e = lane; e < pl.num_envs; e += 64) full += pl.games[e] >= G ? 1 : 0;
    s_v[lane] = v; s_n[lane] = cnt; s_s[lane] = st; s_f[lane] = full;
    __syncthreads();
    if (lane != 0) return;
    double tv = 0.0;
    long long tn = 0, ts = 0, tf = 0;
    for (int l = 0; l < 64; ++l) { tv += s_v[l]; tn += s_n[l]; ts += s_s[l]; tf += s_f[l]; }
    out[0] = tv; out[1] = (double)tn; out[2] = (double)ts; out[3] = (double)tf;
}

}  // namespace ipp
