#!/usr/bin/env python3
"""
Generate tests/golden/cmaes.npz: recorded values of the reference's CMA-ES trajectory objective, IPPMashaMission.simulate_trajectory
(planning/ipp_masha.py:102-140), with the per-waypoint rewards and costs it was made of.  Numeric arrays only.

The reference is imported the way gen_golden.py imports it (that module's cv2 / imageio stubs and builders are reused); the `cma`
package is not installed here and planning/ipp_masha.py imports it at module level, so an empty stub module takes its place --
simulate_trajectory never touches it.

Missions: 10x10 and 20x20 grids, seed 3, altitudes 8..14, horizon 3, uav = {max_v: 2, max_a: 2}, adaptive (threshold 0.4, factor 0) and
non-adaptive, from the prior state at the mission's start waypoint.  Per grid the same trajectories are recorded with a remaining
budget of 200 and of 12:
  * random interior trajectories with off-centre positions and off-level altitudes,
  * a waypoint exactly on the far edge (legal) and one a hair outside (100),
  * three copies of the start waypoint (path cost 0: 100), a repeated interior waypoint (a zero-cost live step),
  * a trajectory that stays near the start (budget 12 leaves it unaffected) and one whose first step budget 12 cannot pay (0.0).

Usage:  python tests/golden/gen_cmaes_golden.py        (writes tests/golden/cmaes.npz)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402  (stubs cv2 / imageio, puts the reference on sys.path)
import numpy as np  # noqa: E402

sys.modules.setdefault("cma", types.ModuleType("cma"))

from planning import ipp_masha as ref_masha  # noqa: E402
from planning.common import actions as ref_actions  # noqa: E402

UAV = {"max_v": 2, "max_a": 2}
MIN_ALT, MAX_ALT, SPACING, HORIZON = 8, 14, 6, 3
BUDGETS = (200.0, 12.0)


def trajectories(dim, rs):
    far = 4.0 * dim
    out = []
    for _ in range(4):
        out.append(np.stack([rs.uniform(1.0, far - 1.0, 3), rs.uniform(1.0, far - 1.0, 3), rs.uniform(MIN_ALT, MAX_ALT, 3)], axis=1))
    out.append(np.array([[far, 10.3, 9.5], [17.7, far, 13.25], [21.1, 18.6, 8.0]]))          # on the far edge: legal
    out.append(np.array([[9.2, 10.3, 9.5], [far + 1e-9, 14.4, 13.25], [21.1, 18.6, 8.0]]))   # a hair outside
    out.append(np.array([[9.2, 10.3, 9.5], [17.7, 14.4, 14.0 + 1e-9], [21.1, 18.6, 8.0]]))   # a hair too high
    out.append(np.tile(np.array([2.0, 2.0, 14.0]), (3, 1)))                                  # the start waypoint three times
    out.append(np.array([[13.4, 9.9, 11.7], [13.4, 9.9, 11.7], [22.3, 17.1, 9.2]]))          # a repeated waypoint
    out.append(np.array([[4.1, 3.2, 13.5], [6.3, 5.4, 12.2], [7.6, 7.3, 11.1]]))             # near the start: 12 pays for all of it
    out.append(np.array([[far - 3.3, far - 5.1, 9.4], [far - 9.0, far - 7.7, 12.8], [far - 14.2, far - 6.1, 8.6]]))  # 12 pays for none
    return np.array(out)


def main():
    out = {"prev": np.array([2.0, 2.0, 14.0]), "budgets": np.array(BUDGETS), "uav": np.array([UAV["max_v"], UAV["max_a"]], dtype=np.float64),
           "alts": np.array([MIN_ALT, MAX_ALT, SPACING], dtype=np.float64), "adaptive_info": np.array([0.4, 0.0])}
    recorded = []
    real_step = ref_masha.simulate_prediction_step

    def recording_step(*args, **kwargs):
        res = real_step(*args, **kwargs)
        recorded.append(float(res[0]))
        return res

    ref_masha.simulate_prediction_step = recording_step
    for dim in (10, 20):
        wps = trajectories(dim, np.random.RandomState(40 + dim))
        K = len(wps)
        out[f"waypoints_{dim}"] = wps
        for adaptive in (1, 0):
            params = gg.load_params(dim, dim)
            gm, sensor, sim, mapping = gg.build(params, seed=3)
            mis = ref_masha.IPPMashaMission(mapping, UAV, dist_to_boundaries=10, min_altitude=MIN_ALT, max_altitude=MAX_ALT,
                                            episode_horizon=HORIZON, altitude_spacing=SPACING, budget=BUDGETS[0], adaptive=bool(adaptive),
                                            value_threshold=0.4, interval_factor=0)
            assert np.array_equal(mis.previous_replan_action, out["prev"])
            f = np.empty((len(BUDGETS), K))
            rewards = np.full((len(BUDGETS), K, HORIZON), np.nan)
            costs = np.full((K, HORIZON), np.nan)
            for b, budget in enumerate(BUDGETS):
                mis.remaining_budget = budget
                for k in range(K):
                    del recorded[:]
                    f[b, k] = mis.simulate_trajectory(mis.flatten_waypoints(wps[k]))
                    rewards[b, k, : len(recorded)] = recorded
                    assert np.isfinite(f[b, k])
            for k in range(K):
                p = out["prev"]
                for t in range(HORIZON):
                    costs[k, t] = ref_actions.action_costs(wps[k, t], p, UAV)
                    p = wps[k, t]
            out[f"objective_{dim}_a{adaptive}"] = f
            out[f"rewards_{dim}_a{adaptive}"] = rewards
            out[f"costs_{dim}"] = costs
            print(f"{dim}x{dim} adaptive {adaptive}:")
            for b, budget in enumerate(BUDGETS):
                print(f"  budget {budget}: f = {np.array2string(f[b], precision=4)}")
                print(f"      live steps {np.sum(~np.isnan(rewards[b]), axis=1)}")
    ref_masha.simulate_prediction_step = real_step
    gg.save("cmaes", **out)


if __name__ == "__main__":
    main()
