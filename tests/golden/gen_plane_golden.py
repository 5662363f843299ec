#!/usr/bin/env python3
"""
Generate tests/golden/planes.npz by IMPORTING the reference (/root/reference, read-only) and running its
generate_input_feature_planes (planning/common/features.py:83-151) on the 10x10 example grid, always on COPIES of its
arguments (the reference masks the history's states and overwrites positions[0][2] in place, features.py:64 / :98-99).

Inputs: one short budget-mode episode (the loop of planning/mcts_zero/episode_generators.py:109-150 with fixed actions):
"states" [T+1, N, N] fp64 (state k = the covariance before action k), "positions" [T+1, 3] (the waypoint pushed with state k:
init_action, then the actions), "budgets" [T+1] (remaining / initial), "mean" [N] (the map mean after the episode), and a
three-level descent of simulate_prediction_step states below the last state ("descent_states", "descent_positions",
"descent_budgets").  "proj" [N] is a fixed vector.

Cases, under "<case>_": "idx" (state indices of the history, newest first, into states or descent_states), "fov", "costs",
"adaptive", "thr", "kf", "descent" (1: descent states), "planes" fp32 [C, N, N] (not for grow*: the file stays under 1 MiB) and "proj" fp64 [C, N] =
planes @ proj of the fp64 planes (NaN where the plane is NaN).  Cases:
  final_f{fov}c{costs}a{adaptive}  the last three states, every use_fov x use_costs x adaptive
  grow{t}                          the history after state t (t < 2: shorter than H = 3), position mode with costs, adaptive
  descent                          leaf, parent, grand-parent of the descent, masked with the current mean
  nanmask                          one state, threshold above every mean + k diag: empty mask, NaN state plane
Numeric arrays only.

Usage:  python tests/golden/gen_plane_golden.py        (writes tests/golden/planes.npz; the other fixtures are not touched)
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_golden  # noqa: E402,F401  (puts the reference on sys.path and stubs cv2 / imageio; generates nothing on import)
from gen_golden import build, load_params, save  # noqa: E402
from planning.common.actions import action_costs  # noqa: E402
from planning.common.features import EpisodeHistory, generate_input_feature_planes  # noqa: E402
from planning.common.optimization import simulate_prediction_step  # noqa: E402

DIM, SEED, H = 10, 11, 3
UAV = {"max_v": 2, "max_a": 2}
MIN_ALT, MAX_ALT = 8.0, 14.0
INITIAL_BUDGET = 100.0
THR, KF = 0.5, 0.05
INIT = np.array([2.0, 2.0, 14.0])
ACTIONS = [np.array([18.0, 22.0, 8.0]), np.array([30.0, 10.0, 9.0]), np.array([6.0, 34.0, 12.0]), np.array([26.0, 26.0, 8.0])]
DESCENT = [np.array([14.0, 6.0, 10.0]), np.array([38.0, 38.0, 8.0]), np.array([2.0, 18.0, 14.0])]


def run_planes(mapping, states, positions, budgets, mean, fov, costs, adaptive, thr=THR, kf=KF):
    hist = EpisodeHistory(H)
    for s, p, b in zip(states[::-1], positions[::-1], budgets[::-1]):  # push oldest first: history.states[0] is the newest
        hist.push(s.copy(), copy.deepcopy(p), b)
    info = {"mean": mean.copy(), "value_threshold": thr, "interval_factor": kf} if adaptive else None
    lo, hi = (None, None) if fov else (MIN_ALT, MAX_ALT)
    return np.asarray(generate_input_feature_planes(mapping, hist, lo, hi, info, UAV, use_action_costs_input=costs), dtype=np.float64)


def main():
    params = load_params(DIM, DIM)
    gm, sensor, sim, mapping = build(params, seed=SEED)
    states, positions, budgets = [gm.cov_matrix.copy()], [INIT.copy()], [1.0]
    prev, remaining = INIT.copy(), INITIAL_BUDGET
    for a in ACTIONS:
        z = sensor.take_measurement(a, verbose=False)  # altitudes <= rf_altitude: no resize stub involved
        mapping.update_grid_map(a, z)
        remaining -= action_costs(a, prev, UAV)
        prev = a
        states.append(gm.cov_matrix.copy())
        positions.append(a.copy())
        budgets.append(remaining / INITIAL_BUDGET)
    mean = gm.mean.copy()
    info = {"mean": mean.copy(), "value_threshold": THR, "interval_factor": KF}
    d_states, d_pos, d_bud = [], [], []
    st, pv, rem = states[-1].copy(), positions[-1].copy(), remaining
    for a in DESCENT:
        _, _, st = simulate_prediction_step(st.copy(), pv.copy(), a, mapping, UAV, copy.deepcopy(info))
        rem -= action_costs(a, pv, UAV)
        pv = a
        d_states.append(st.copy())
        d_pos.append(a.copy())
        d_bud.append(rem / INITIAL_BUDGET)
    rs = np.random.RandomState(5)
    proj = rs.normal(size=DIM * DIM)
    out = dict(states=np.array(states), positions=np.array(positions), budgets=np.array(budgets), mean=mean,
               descent_states=np.array(d_states), descent_positions=np.array(d_pos), descent_budgets=np.array(d_bud), proj=proj,
               initial_budget=np.float64(INITIAL_BUDGET), min_altitude=np.float64(MIN_ALT), max_altitude=np.float64(MAX_ALT),
               max_v=np.float64(UAV["max_v"]), max_a=np.float64(UAV["max_a"]), history=np.int32(H))

    def case(name, idx, fov, costs, adaptive, descent=False, thr=THR, kf=KF, keep_planes=True):
        src_s, src_p, src_b = (d_states, d_pos, d_bud) if descent else (states, positions, budgets)
        planes = run_planes(mapping, [src_s[i] for i in idx], [src_p[i] for i in idx], [src_b[i] for i in idx], mean, fov, costs,
                            adaptive, thr, kf)
        out.update({f"{name}_idx": np.array(idx, dtype=np.int32), f"{name}_fov": np.int32(fov), f"{name}_costs": np.int32(costs),
                    f"{name}_adaptive": np.int32(adaptive), f"{name}_thr": np.float64(thr), f"{name}_kf": np.float64(kf),
                    f"{name}_descent": np.int32(descent), f"{name}_proj": planes @ proj})
        if keep_planes:
            out[f"{name}_planes"] = planes.astype(np.float32)
        return planes

    T = len(ACTIONS)
    for fov in (0, 1):
        for costs in (0, 1):
            for adaptive in (0, 1):
                case(f"final_f{fov}c{costs}a{adaptive}", [T, T - 1, T - 2], fov, costs, adaptive)
    for t in range(T + 1):
        case(f"grow{t}", list(range(t, max(t - H, -1), -1)), 0, 1, 1, keep_planes=False)
    case("descent", [2, 1, 0], 0, 1, 1, descent=True)
    nan = case("nanmask", [T], 0, 0, 1, thr=50.0)
    assert np.isnan(nan[0]).all()
    m = mean.ravel() + KF * np.diag(states[T]) >= THR
    print(f"  final-state mask keeps {int(m.sum())} of {m.size} cells")
    save("planes", **out)


if __name__ == "__main__":
    main()
