// Classic MCTS for a batch (planning/mcts_mission.py of the reference): candidate scoring from MANY tree nodes in one call
// (ipp_tree_score_nodes) and the rollout policy on the device (ipp_rollout_*: MCTSMission.rollout / gcb_rollout / eps_greedy_policy /
// gcb_policy / get_next_actions_mask, :167-256).  The kernels:
//   k_nodes_expand       one thread per (node, candidate): the item lists of the predict-only tree-step launches (root id, path, start
//                        waypoint of every candidate, in the caller's scratch) and the action cost in fp64
//   k_rollout_candidates one thread per (rollout, candidate): the get_actions-ordered waypoints around the rollout's current cell
//                        (planning/vec_greedy.py radius_candidates); NaN rows outside the grid, at 3-D distance >= radius, for a dead rollout
//   k_rollout_pick       one wave per rollout, candidates strided over the lanes: the availability mask, the greedy first maximiser /
//                        the u1-th available candidate / the softmax draw, the picked waypoint and the node id of its recorded step
//   k_rollout_advance    one thread per rollout: return, discount, budget (charged from the GRANDPARENT's waypoint, :226), waypoint, path
// "No candidate" rows are not compacted away: they become items whose non-finite action ends them in the step kernel's header
// (k_prepare.h make_item_header; k_tree_patch.h, k_tree.h m == 0) before any address is formed from the action.
// fp64 without fused multiply-adds (the host restatements in planning/device_rollout.py give the same bits), sums in a stated
// order, no atomics, lowest index wins ties.  k_score_expand (k_score_batch.h) keeps its own, contracted, cost arithmetic: sharing
// one helper would change either its bits or the rollout's.
#pragma once
#include "ipp_common.h"

namespace ipp {

// bytes of caller scratch per candidate: root id (int32) + path (kTreeDepth int32) + start waypoint (3 doubles), each array 256-byte aligned
inline uint64_t nodes_scratch_align(uint64_t b) { return (b + 255) / 256 * 256; }
inline uint64_t nodes_scratch_bytes(uint64_t items) {
    return nodes_scratch_align(items * 4) + nodes_scratch_align(items * 4 * kTreeDepth) + nodes_scratch_align(items * 24);
}

__device__ __forceinline__ double rollout_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// action_costs (planning/common/actions.py:8-41): the distance, or the trapezoidal flight time; every operation rounded on its own
__device__ __forceinline__ double rollout_cost(double ax, double ay, double az, double px, double py, double pz, bool flight, double vmax,
                                               double amax) {
#pragma clang fp contract(off)
    const double dx = ax - px, dy = ay - py, dz = az - pz;
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    if (!flight) return dist;
    const double d_acc = fmin(dist * 0.5, vmax * vmax / (2 * amax));
    return (dist - 2 * d_acc) / vmax + 2 * sqrt(2 * d_acc / amax);
}

__global__ __launch_bounds__(256) void k_nodes_expand(int n, int k, const int* __restrict__ root_ids, const int* __restrict__ path_ids,
                                                      const double* __restrict__ actions, const double* __restrict__ prev_action,
                                                      unsigned flags, double vmax, double amax, int* __restrict__ roots_out,
                                                      int* __restrict__ paths_out, double* __restrict__ prev_out, double* __restrict__ cost_out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)n * k) return;
    const size_t item = c / (size_t)k;
    roots_out[c] = root_ids[item];
#pragma unroll
    for (int d = 0; d < kTreeDepth; ++d) paths_out[c * kTreeDepth + d] = path_ids[item * kTreeDepth + d];
    const double px = prev_action[3 * item + 0], py = prev_action[3 * item + 1], pz = prev_action[3 * item + 2];
    prev_out[3 * c + 0] = px; prev_out[3 * c + 1] = py; prev_out[3 * c + 2] = pz;
    if (!cost_out) return;
    const double ax = actions[3 * c + 0], ay = actions[3 * c + 1], az = actions[3 * c + 2];
    const bool finite_action = isfinite(ax) && isfinite(ay) && isfinite(az);
    cost_out[c] = finite_action ? rollout_cost(ax, ay, az, px, py, pz, (flags & IPP_USE_FLIGHT_TIME) != 0, vmax, amax) : rollout_nan();
}

// candidate j of the (2 half + 1)^2 n_levels square around (cx, cy, cz): its waypoint, and whether it is a candidate at all (in the grid,
// 3-D distance < radius).  Shared by k_rollout_candidates and the tree kernels' count of available actions (k_ctree.h).
__device__ __forceinline__ bool rollout_candidate(const ipp_rollout& ro, int j, double cx, double cy, double cz, double& x, double& y,
                                                  double& z) {
#pragma clang fp contract(off)
    const int side = 2 * ro.half + 1;
    const int off = j / ro.n_levels, lev = j - off * ro.n_levels;
    const int drow = off / side - ro.half, dcol = off - (off / side) * side - ro.half;
    const double res = ro.resolution;
    const double row = floor(cy / res) + (double)drow, col = floor(cx / res) + (double)dcol;
    x = res * col + 0.5 * res; y = res * row + 0.5 * res; z = ro.levels[lev];
    const double dx = x - cx, dy = y - cy, dz = z - cz;
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);  // (np.linalg.norm over the last axis: the three squares in order)
    return row >= 0.0 && row < (double)ro.grid_h && col >= 0.0 && col < (double)ro.grid_w && dist < ro.radius;
}

__global__ __launch_bounds__(256) void k_rollout_candidates(ipp_rollout ro) {
#pragma clang fp contract(off)
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)ro.n * ro.kmax) return;
    const int i = (int)(c / (size_t)ro.kmax), j = (int)(c - (size_t)i * ro.kmax);
    double x, y, z;
    const bool inside = rollout_candidate(ro, j, ro.cur[3 * i + 0], ro.cur[3 * i + 1], ro.cur[3 * i + 2], x, y, z);
    const bool keep = ro.live[i] != 0 && inside;
    const double nan = rollout_nan();
    ro.cand[3 * c + 0] = keep ? x : nan;
    ro.cand[3 * c + 1] = keep ? y : nan;
    ro.cand[3 * c + 2] = keep ? z : nan;
}

// LDS: double[kmax] exp(reward) of the available candidates (cost-benefit mode)
__global__ __launch_bounds__(64) void k_rollout_pick(ipp_rollout ro, int level) {
#pragma clang fp contract(off)
    extern __shared__ double ro_lds[];
    const int i = blockIdx.x, lane = threadIdx.x, kmax = ro.kmax;
    if (i >= ro.n) return;
    const double nan = rollout_nan();
    int end_flag = -1;  // >= 0: the rollout ends here with this flag
    const bool live = ro.live[i] != 0;
    const double budget = ro.budget[i];
    if (live && (ro.depth_left[i] == 0 || budget < ro.resolution)) end_flag = IPP_ROLLOUT_END;  // (no uniform is consumed)
    int best = -1;
    if (live && end_flag < 0) {
        const double* cand = ro.cand + (size_t)i * kmax * 3;
        const float* rw = ro.reward + (size_t)i * kmax;
        const double* cs = ro.cost + (size_t)i * kmax;
        const int* st = ro.status + (size_t)i * kmax;
        const double u0 = ro.u[((size_t)i * ro.max_depth + level) * 2 + 0], u1 = ro.u[((size_t)i * ro.max_depth + level) * 2 + 1];
        // availability (get_next_actions_mask, :167-173): a candidate row, 0 < cost <= budget
        int count = 0;
        bool bad = false, any_nan = false;
        float bv = -INFINITY;  // this lane's first maximiser over its candidates, ascending
        int bi = 0x7fffffff;
        for (int k0 = 0; k0 < kmax; k0 += 64) {
            const int k = k0 + lane;
            bool av = false;
            if (k < kmax) {
                const double c = cs[k];
                av = isfinite(cand[3 * k]) && isfinite(cand[3 * k + 1]) && isfinite(cand[3 * k + 2]) && c > 0.0 && c <= budget;
                if (av) {
                    const float r = rw[k];
                    bad |= st[k] == IPP_STATUS_BAD_FOOTPRINT;
                    any_nan |= r != r;
                    if (r > bv) { bv = r; bi = k; }
                    if (ro.gcb) ro_lds[k] = exp((double)r);
                } else if (ro.gcb) {
                    ro_lds[k] = -1.0;  // (exp >= 0: marks "not available" for lane 0's passes below)
                }
            }
            count += __popcll(__ballot(av));
        }
        bad = __any(bad);
        any_nan = __any(any_nan);
        if (bad) end_flag = IPP_ROLLOUT_ERR_FOOTPRINT;
        else if (count == 0) end_flag = IPP_ROLLOUT_NO_ACTION;  // (np.random.choice(0) raises in the reference)
        else if (ro.gcb) {
            // gcb_policy (:204-221): p = exp(r) / sum exp(r) over the available candidates in ascending order; np.random.choice(n, p = p) =
            // cdf.searchsorted(u, side = "right") on cdf = cumsum(p) / cumsum(p)[-1].  Lane 0 adds in ascending order.
            if (any_nan) end_flag = IPP_ROLLOUT_ERR_NAN;
            else {
                __syncthreads();
                if (lane == 0) {
                    double s = 0.0, tot = 0.0, cum = 0.0;
                    int last = -1;
                    for (int k = 0; k < kmax; ++k)
                        if (ro_lds[k] >= 0.0) s += ro_lds[k];
                    for (int k = 0; k < kmax; ++k)
                        if (ro_lds[k] >= 0.0) tot += ro_lds[k] / s;
                    for (int k = 0; k < kmax && best < 0; ++k)
                        if (ro_lds[k] >= 0.0) {
                            cum += ro_lds[k] / s;
                            last = k;
                            if (cum / tot > u1) best = k;
                        }
                    if (best < 0) best = last;  // (u1 < 1 = cdf[-1]: not reached with finite sums)
                }
                best = __shfl(best, 0, 64);
                if (best < 0) end_flag = IPP_ROLLOUT_ERR_NAN;
            }
        } else if (u0 > ro.epsilon) {
            // greedy_action (:232-246): the first maximiser, strict >, a NaN never wins; rewards as the fp32 the step kernel returned
            float m = bv;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            int idx = (bi != 0x7fffffff && bv == m) ? bi : 0x7fffffff;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) idx = min(idx, __shfl_xor(idx, o, 64));
            if (idx == 0x7fffffff) end_flag = IPP_ROLLOUT_ERR_NAN;  // (every reward NaN: the reference returns None and fails)
            else best = idx;
        } else {
            // np.random.choice(count): available candidate number min(floor(u1 count), count - 1) in ascending order
            long long pick = (long long)(u1 * (double)count);
            pick = pick < count - 1 ? pick : count - 1;
            int seen = 0;
            for (int k0 = 0; k0 < kmax && best < 0; k0 += 64) {
                const int k = k0 + lane;
                bool av = false;
                if (k < kmax) {
                    const double c = cs[k];
                    av = isfinite(cand[3 * k]) && isfinite(cand[3 * k + 1]) && isfinite(cand[3 * k + 2]) && c > 0.0 && c <= budget;
                }
                unsigned long long b = __ballot(av);
                const int c = __popcll(b);
                if (pick < seen + c) {
                    for (int r = (int)pick - seen; r > 0; --r) b &= b - 1;  // drop the r lowest available
                    best = k0 + (int)__ffsll((long long)b) - 1;
                }
                seen += c;
            }
        }
    }
    if (lane != 0) return;
    if (best >= 0) {
        for (int q = 0; q < 3; ++q) ro.action[3 * i + q] = ro.cand[((size_t)i * kmax + best) * 3 + q];
        ro.new_id[i] = ro.node_base + i * ro.max_depth + level;
        ro.pick_idx[(size_t)i * ro.max_depth + level] = best;
        return;
    }
    for (int q = 0; q < 3; ++q) ro.action[3 * i + q] = nan;  // (the step below applies nothing for it)
    ro.new_id[i] = -1;
    if (live) { ro.live[i] = 0; ro.flag[i] = end_flag; }
}

__global__ __launch_bounds__(64) void k_rollout_advance(ipp_rollout ro) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ro.n || ro.live[i] == 0) return;
    const int st = ro.step_status[i];
    if (st != IPP_STATUS_OK && st != IPP_STATUS_RANK_FULL) { ro.live[i] = 0; ro.flag[i] = IPP_ROLLOUT_ERR_STEP; return; }
    const double disc = ro.disc[i];
    ro.value[i] = ro.value[i] + disc * (double)ro.step_reward[i];  // reward + gamma rollout(...) unrolled from the top (:226)
    ro.disc[i] = disc * ro.gamma;
    if (st == IPP_STATUS_RANK_FULL) { ro.live[i] = 0; ro.flag[i] = IPP_ROLLOUT_RANK_FULL; return; }  // (no node was written)
    const double ax = ro.action[3 * i + 0], ay = ro.action[3 * i + 1], az = ro.action[3 * i + 2];
    ro.budget[i] = ro.budget[i] - rollout_cost(ax, ay, az, ro.charge_from[3 * i + 0], ro.charge_from[3 * i + 1], ro.charge_from[3 * i + 2],
                                               (ro.flags & IPP_USE_FLIGHT_TIME) != 0, ro.vmax, ro.amax);
    for (int q = 0; q < 3; ++q) ro.charge_from[3 * i + q] = ro.cur[3 * i + q];  // previous_action of the next level = this node's waypoint
    ro.cur[3 * i + 0] = ax; ro.cur[3 * i + 1] = ay; ro.cur[3 * i + 2] = az;
    const int pl = ro.plen[i];
    if (pl < kTreeDepth) { ro.path[(size_t)i * kTreeDepth + pl] = ro.new_id[i]; ro.plen[i] = pl + 1; }
    ro.depth_left[i] = ro.depth_left[i] - 1;
}

}  // namespace ipp
