// Candidate-action scoring for MANY envs in one call (ipp_score_actions_envs): the reward of k candidates from the current state of
// each of n env slots of a patch-layout engine, nothing written to any env (planning/common/optimization.py:33-104 asks for exactly
// this per reachable action, planning/mcts_mission.py:232-246 as the rollout policy).
//
// The rewards come from the predict-only covariance-only launches of k_step_patch.h, one item per (env, candidate).  A kernel that
// streamed an env's stored columns once per GROUP of candidates (one wave per candidate, the group's patches staged in LDS, the
// window's accumulators in registers) was built and measured for this call: bit-identical rewards, but 2.4 x SLOWER than the repeated
// predict steps at 64, 256 and 1024 candidates per env (profiles/vec_greedy_bench.txt), so it is not part of the library.
// What is left here is the per-candidate part that the step launches do not return: the item lists (env id and start waypoint of every
// candidate, in the caller's scratch) and the action cost in fp64 (planning/common/actions.py:8-41) for the budget filter of get_actions.
#pragma once
#include "ipp_common.h"

namespace ipp {

// bytes of caller scratch per candidate: env id (int32) + start waypoint (3 doubles), each array 256-byte aligned
inline uint64_t score_batch_ids_bytes(uint64_t items) { return (items * 4 + 255) / 256 * 256; }
inline uint64_t score_batch_scratch_bytes(uint64_t items) { return score_batch_ids_bytes(items) + (items * 24 + 255) / 256 * 256; }

__global__ __launch_bounds__(256) void k_score_expand(View v, const int* __restrict__ env_ids, int n, int k, const double* __restrict__ actions,
                                                      const double* __restrict__ prev_action, unsigned flags, int* __restrict__ ids_out,
                                                      double* __restrict__ prev_out, double* __restrict__ cost_out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)n * k) return;
    const int item = (int)(c / (size_t)k);
    ids_out[c] = env_ids ? env_ids[item] : item;
    const double px = prev_action[3 * (size_t)item + 0], py = prev_action[3 * (size_t)item + 1], pz = prev_action[3 * (size_t)item + 2];
    prev_out[3 * c + 0] = px; prev_out[3 * c + 1] = py; prev_out[3 * c + 2] = pz;
    if (!cost_out) return;
    const double ax = actions[3 * c + 0], ay = actions[3 * c + 1], az = actions[3 * c + 2];
    const double dx = ax - px, dy = ay - py, dz = az - pz;
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);                        // actions.py:15-16
    double cost = dist;
    if (flags & IPP_USE_FLIGHT_TIME) {                                            // actions.py:32-41 (make_item_header, k_prepare.h)
        const double d_acc = fmin(dist * 0.5, v.vmax * v.vmax / (2 * v.amax));
        cost = (dist - 2 * d_acc) / v.vmax + 2 * sqrt(2 * d_acc / v.amax);
    }
    const bool finite_action = isfinite(ax) && isfinite(ay) && isfinite(az);
    cost_out[c] = finite_action ? cost : __longlong_as_double(0x7ff8000000000000ll);  // a NaN row = no candidate
}

}  // namespace ipp
