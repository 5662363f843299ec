// The four baseline missions for a batch (planning/baselines/{lawn_mower,conical_spiral,random_discrete,random_continuous}_mission.py
// of the reference): ONE decision per env and call, on the env batch's ledger (ipp_set_budget).  The kernels:
//   k_baseline_table       one thread per env: the next row of the host-built waypoint table while the budget rule of the kind holds
//   k_baseline_discrete    one workgroup per env over the A = levels N cell-centre actions of enumerate_actions (never stored): a count
//                          pass, then the valid action of rank min(floor(u count), count - 1) IN INDEX ORDER (actions_np[msk][k]): ranks
//                          inside a wave by ballot + popcount, across waves and strides through LDS, no atomics
//   k_baseline_continuous  one wave per env: lane = trial in two rounds of 64 (101 trials), ballot, first set bit
// Every kernel starts with the same bookkeeping: an env whose `episode` differs from `seen_episode` (an auto-reset on the device) gets
// cursor 0 and latches its start budget; `decision` counts the calls.  An env without an action keeps its waypoint and gets budget 0
// (VecGreedyPolicy.act's convention: the env's own rule then ends its episode on the next budget step).
// fp64 without fused multiply-adds: the host restatements (planning/vec_baselines.py) give the same bits.
#pragma once
#include "ipp_common.h"

namespace ipp {
namespace bl {

constexpr int kTrials = IPP_BASELINE_TRIALS;
constexpr int kDiscreteThreads = 256;

// action_costs (planning/common/actions.py:8-41): the distance, or the trapezoidal flight time; every operation rounded on its own
__device__ __forceinline__ double distance(double ax, double ay, double az, double px, double py, double pz) {
#pragma clang fp contract(off)
    const double dx = ax - px, dy = ay - py, dz = az - pz;
    return sqrt(dx * dx + dy * dy + dz * dz);
}
__device__ __forceinline__ double flight_time(double dist, double vmax, double amax) {
#pragma clang fp contract(off)
    const double d_acc = fmin(dist * 0.5, vmax * vmax / (2 * amax));
    return (dist - 2 * d_acc) / vmax + 2 * sqrt(2 * d_acc / amax);
}
__device__ __forceinline__ double cost(const ipp_baseline& b, double ax, double ay, double az, double px, double py, double pz) {
    const double d = distance(ax, ay, az, px, py, pz);
    return b.use_flight_time ? flight_time(d, b.max_v, b.max_a) : d;
}

// uniform in (0, 1) of (global env id, decision, trial, component): vec_env.philox_uniform(counter, IPP_BASELINE_STREAM + decision, seed)
// with counter = 512 global id + 4 trial + component -- a value does not depend on which envs share a launch
__device__ __forceinline__ double philox_u(const ipp_baseline& b, int env, long long decision, int trial, int comp) {
    const uint64_t q = (uint64_t)((long long)env + b.row_offset) * 512ull + (uint64_t)(4 * trial + comp);
    const uint64_t sub = (uint64_t)IPP_BASELINE_STREAM + (uint64_t)decision;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)sub, (uint32_t)(sub >> 32)};
    uint32_t k[2] = {(uint32_t)b.seed, (uint32_t)(b.seed >> 32)};
    for (int r = 0; r < 10; ++r) philox_round(c, k);
    return ((double)c[0] + 0.5) * (1.0 / 4294967296.0);
}

// the bookkeeping of one env, by ONE thread: cursor reset on a new episode, the decision counter
__device__ __forceinline__ void begin_decision(const ipp_baseline& b, int e, double budget, long long decision) {
    const long long ep = b.episode[e];
    if (b.seen_episode[e] != ep) {
        b.seen_episode[e] = ep;
        b.cursor[e] = 0;
        b.start_budget[e] = budget;
    }
    b.decision[e] = decision + 1;
}

__device__ __forceinline__ void write_decision(const ipp_baseline& b, int e, bool has, double x, double y, double z) {
    b.action[3 * e + 0] = has ? x : b.prev[3 * e + 0];
    b.action[3 * e + 1] = has ? y : b.prev[3 * e + 1];
    b.action[3 * e + 2] = has ? z : b.prev[3 * e + 2];
    b.has[e] = has ? 1 : 0;
    if (!has) b.budget[e] = 0.0;
}

// LAWNMOWER (lawn_mower_mission.py:93-100,130): cursor < K and budget >= step_size and budget > cost(next, prev)
// SPIRAL (conical_spiral_mission.py:100-106): cursor < K and (cursor == 0 or budget - cost(next, prev) >= 0)
__global__ __launch_bounds__(256) void k_baseline_table(ipp_baseline b) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.n) return;
    const double budget = b.budget[e];
    begin_decision(b, e, budget, b.decision[e]);
    const int cur = b.cursor[e];
    bool has = false;
    double x = 0, y = 0, z = 0;
    if (cur >= 0 && cur < b.table_len) {
        x = b.table[3 * cur + 0]; y = b.table[3 * cur + 1]; z = b.table[3 * cur + 2];
        const double c = cost(b, x, y, z, b.prev[3 * e + 0], b.prev[3 * e + 1], b.prev[3 * e + 2]);
        has = b.kind == IPP_BASELINE_LAWNMOWER ? (budget >= b.step_size && budget > c) : (cur == 0 || budget - c >= 0.0);
    }
    if (has) b.cursor[e] = cur + 1;
    write_decision(b, e, has, x, y, z);
}

// action i of enumerate_actions (actions.py:73-91; square grids): level h = i / N, cell c = i % N with the reference's flattening
// x_dim * (x cell) + (y cell); waypoint (res xc + res / 2, res yc + res / 2, levels[h]).  valid: get_next_actions_mask (:73-79)
__device__ __forceinline__ bool discrete_valid(const ipp_baseline& b, int i, int A, double px, double py, double pz, double budget, double& x,
                                               double& y, double& z) {
#pragma clang fp contract(off)
    if (i >= A) return false;
    const int N = b.grid_w * b.grid_h;
    const int h = i / N, c = i - h * N;
    const int xc = c / b.grid_w, yc = c - xc * b.grid_w;
    const double half = 0.5 * b.resolution;
    x = (double)xc * b.resolution + half;
    y = (double)yc * b.resolution + half;
    z = b.levels[h];
    const double d = distance(x, y, z, px, py, pz);
    if (!b.adaptive) return d > 0.0 && d <= budget && d < 11.5;
    const double t = flight_time(d, b.max_v, b.max_a);
    return t > 0.0 && t <= budget;
}

// Cost: the mask is evaluated over the WHOLE action set twice per decision (count pass, select pass; the select pass stops at the stride
// that holds the pick) -- per env 2 A distances with an fp64 square root, not stored in between because A has no bound that fits LDS.
// 4096 envs x 25 000 actions: 0.40 ms beside a 0.15 ms env step (profiles/baselines_bench.txt); left untuned.
__global__ __launch_bounds__(kDiscreteThreads) void k_baseline_discrete(ipp_baseline b) {
#pragma clang fp contract(off)
    __shared__ int s_wave[kDiscreteThreads / kWave];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kDiscreteThreads / kWave;
    const int A = b.n_levels * b.grid_w * b.grid_h;
    const double budget = b.budget[e];
    const long long decision = b.decision[e];
    const double px = b.prev[3 * e + 0], py = b.prev[3 * e + 1], pz = b.prev[3 * e + 2];
    const double u = b.uniforms ? b.uniforms[e] : philox_u(b, e, decision, 0, 0);
    // count pass: every wave's share by ballot + popcount, the waves' shares through LDS
    int mine = 0;
    for (int base = 0; base < A; base += kDiscreteThreads) {
        double x, y, z;
        const bool ok = discrete_valid(b, base + tid, A, px, py, pz, budget, x, y, z);
        mine += __popcll(__ballot(ok));  // (wave-uniform)
    }
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    int count = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) count += s_wave[w];
    __syncthreads();  // (s_wave is reused below; every thread has read `decision` and the env's row: thread 0 may write them now)
    if (tid == 0) begin_decision(b, e, budget, decision);
    if (count == 0) {
        if (tid == 0) write_decision(b, e, false, 0, 0, 0);
        return;
    }
    int k = (int)floor(u * (double)count);
    k = k < 0 ? 0 : (k > count - 1 ? count - 1 : k);
    // select pass: the strides in index order; `before` = valid actions of lower index
    int before = 0;
    for (int base = 0; base < A; base += kDiscreteThreads) {
        double x, y, z;
        const bool ok = discrete_valid(b, base + tid, A, px, py, pz, budget, x, y, z);
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int below = before, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int cw = s_wave[w];
            below += w < wave ? cw : 0;
            total += cw;
        }
        const int rank = below + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && rank == k) write_decision(b, e, true, x, y, z);
        before += total;
        __syncthreads();
        if (before > k) break;  // (block-uniform: `before` is the same number in every thread)
    }
}

// RANDOM_CONTINUOUS (random_continuous_mission.py:68-101,118): up to 101 trials low + (high - low) u_t; the first with budget - cost >= 0
// wins, else the 101st; has = budget >= 0 and budget > cost(chosen).  uniforms [n][101][3]
__global__ __launch_bounds__(kWave) void k_baseline_continuous(ipp_baseline b) {
#pragma clang fp contract(off)
    const int e = blockIdx.x, lane = threadIdx.x;
    const double budget = b.budget[e];
    const long long decision = b.decision[e];
    const double px = b.prev[3 * e + 0], py = b.prev[3 * e + 1], pz = b.prev[3 * e + 2];
    const double lx = b.low[0], ly = b.low[1], lz = b.low[2];
    const double sx = b.high[0] - lx, sy = b.high[1] - ly, sz = b.high[2] - lz;
    int win = -1;
    double x = 0, y = 0, z = 0, c = 0;
    for (int round = 0; round < 2 && win < 0; ++round) {
        const int t = round * kWave + lane;
        bool ok = false;
        if (t < kTrials) {
            double u0, u1, u2;
            if (b.uniforms) {
                const double* ut = b.uniforms + ((size_t)e * kTrials + t) * 3;
                u0 = ut[0]; u1 = ut[1]; u2 = ut[2];
            } else {
                u0 = philox_u(b, e, decision, t, 0); u1 = philox_u(b, e, decision, t, 1); u2 = philox_u(b, e, decision, t, 2);
            }
            x = lx + sx * u0; y = ly + sy * u1; z = lz + sz * u2;
            c = cost(b, x, y, z, px, py, pz);
            ok = budget - c >= 0.0;
        }
        const unsigned long long m = __ballot(ok);
        if (m) win = round * kWave + (__ffsll((long long)m) - 1);
        else if (round == 1) win = kTrials - 1;
    }
    if (lane == 0) begin_decision(b, e, budget, decision);
    if (lane == (win & (kWave - 1))) write_decision(b, e, budget >= 0.0 && budget > c, x, y, z);
}

}  // namespace bl
}  // namespace ipp
