#!/usr/bin/env python3
"""
Generate tests/golden/baselines.npz by IMPORTING the reference's four baseline missions (planning/baselines/*.py) and its np.interp
resampling (experiments/experiments.py:227-229) and recording their outputs: numeric arrays only, no reference source text.

The missions' create_waypoints functions are called unbound on a SimpleNamespace that carries the attributes they read (no Mapping, no
sensor): they plan from the grid's dimensions, the altitudes and the budget alone.  cv2 / imageio are stubbed like in gen_golden.py.

Groups of keys (g = 10: the 10x10 grid of the kernel and host tests; g = 50: the smallest grid a budget-mode VecIPPEnv accepts, for the
end-to-end tests):
  lawn_g{g}_{uav}_{cut|all}, spiral_g{g}_{uav}_{cut|all}   create_waypoints' output; *_budget the budgets, uav in {dist, time}
  disc_g{g}_{na|ad}_s{seed}_*     per draw: prev, budget (remaining before the draw), count (msk.sum()), idx (the drawn action_idx),
                                  way (the waypoint); the replayed uniform is (idx + 0.5) / count
  cont_g{g}_s{seed}_*             per outer iteration: prev, budget, used (uniform triples consumed), way; u: the consumed triples in order
  curve_*                         three synthetic runs, np.interp on the axis of experiments.py:227-228

The generator ASSERTS a condition on its own inputs: no recorded decision lies within 1e-9 (relative) of the threshold it is compared
against (a cost against the budget, a distance against 11.5, the remaining budget against 0 or step_size); seeds or budgets are moved
until it holds, so a last-bit difference between np.linalg.norm and the device's sqrt cannot flip a recorded decision.

Usage:  python tests/golden/gen_golden_baselines.py
"""
import os
import sys
import types
from types import SimpleNamespace

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "baselines.npz")

if not os.path.isdir(REF):
    sys.exit("reference checkout not present: golden vectors can only be generated in the build container")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import matplotlib  # noqa: E402

matplotlib.use("Agg")
for name in ("cv2", "imageio"):
    sys.modules.setdefault(name, types.ModuleType(name))

from planning.common import actions as ref_actions  # noqa: E402
from planning.baselines.lawn_mower_mission import LawnMowerMission  # noqa: E402
from planning.baselines.conical_spiral_mission import ConicalSpiralMission  # noqa: E402
from planning.baselines.random_discrete_mission import RandomDiscreteMission  # noqa: E402
from planning.baselines.random_continuous_mission import RandomContinuousMission  # noqa: E402

UAV = {"max_v": 2, "max_a": 2, "sampling_time": 2}  # config/example.yaml
RES, DTB, ALT_LO, ALT_HI, SPACING = 4, 4, 8, 14, 3
STEP_SIZE, NUM_WAYPOINTS, SLOPE = 8, 40, 10
MARGIN = 1e-9


class NearThreshold(Exception):
    pass


def clear(a, b):
    """a is compared against b: not within MARGIN (relative) of it."""
    if abs(a - b) <= MARGIN * max(abs(a), abs(b), 1.0):
        raise NearThreshold(f"{a!r} against {b!r}")


def mission(dim, budget, uav, **kw):
    gm = SimpleNamespace(x_dim=dim, y_dim=dim, resolution=RES, num_grid_cells=dim * dim)
    return SimpleNamespace(mapping=SimpleNamespace(grid_map=gm), uav_specifications=uav, dist_to_boundaries=DTB, min_altitude=ALT_LO,
                           max_altitude=ALT_HI, budget=budget, init_action=np.array([2, 2, 14]), **kw)


def lawnmower(dim, budget, uav):
    m = mission(dim, budget, uav, step_size=STEP_SIZE, altitude_spacing=SPACING)
    way, _ = LawnMowerMission.create_waypoints(m)
    # the thresholds create_waypoints and execute compare against, walked again with the reference's cost
    left, prev = budget, m.init_action
    for w in way:
        clear(left, STEP_SIZE)
        c = ref_actions.action_costs(w, prev, uav)
        clear(left, c)
        left, prev = left - c, w
    clear(left, STEP_SIZE)
    return way.astype(np.float64)


def spiral(dim, budget, uav):
    m = mission(dim, budget, uav, num_waypoints=NUM_WAYPOINTS, slope_factor=SLOPE)
    way, _ = ConicalSpiralMission.create_waypoints(m)
    full, _ = ConicalSpiralMission.create_waypoints(mission(dim, np.inf, uav, num_waypoints=NUM_WAYPOINTS, slope_factor=SLOPE))
    left = budget - ref_actions.action_costs(m.init_action, full[0], uav)
    for i in range(1, min(len(way) + 1, len(full))):
        left -= ref_actions.action_costs(full[i - 1], full[i], uav)
        clear(left, 0.0)
    return way


def discrete(dim, budget, adaptive, seed):
    m = mission(dim, budget, UAV, adaptive=adaptive, altitude_spacing=SPACING)
    m.actions_np = ref_actions.action_dict_to_np_array(ref_actions.enumerate_actions(m.mapping.grid_map, ALT_LO, ALT_HI, SPACING))
    rec = dict(prev=[], budget=[], count=[], idx=[], way=[])

    def mask(position, left):
        msk = RandomDiscreteMission.get_next_actions_mask(m, position, left)
        clear(left, 0.0)
        d = np.linalg.norm(m.actions_np - position, ord=2, axis=1)
        t = ref_actions.compute_flight_times(m.actions_np, position, UAV)
        for v in (t if adaptive else d):
            clear(v, left)
            clear(v, 0.0) if v != 0 else None
        if not adaptive:
            for v in d:
                clear(v, 11.5)
        if msk.sum() > 0:
            rec["prev"].append(np.array(position, dtype=np.float64)); rec["budget"].append(float(left)); rec["count"].append(int(msk.sum()))
        return msk

    m.get_next_actions_mask = mask
    choice = np.random.choice

    def recording_choice(n):
        k = choice(n)
        rec["idx"].append(int(k))
        return k

    np.random.seed(seed)
    np.random.choice = recording_choice
    try:
        way, _ = RandomDiscreteMission.create_waypoints(m)
    finally:
        np.random.choice = choice
    rec["way"] = way
    assert len(way) == len(rec["idx"]) == len(rec["count"])
    if len(way) < 3:
        raise NearThreshold("a mission of fewer than three draws")
    return {k: np.array(v) for k, v in rec.items()}


def continuous(dim, budget, seed):
    m = mission(dim, budget, UAV)
    np.random.seed(seed)
    way, _ = RandomContinuousMission.create_waypoints(m)
    low = np.array([DTB, DTB, ALT_LO], dtype=np.float64)
    high = np.array([dim * RES - DTB, dim * RES - DTB, ALT_HI], dtype=np.float64)
    twin = np.random.RandomState(seed)
    rec = dict(prev=[], budget=[], used=[], u=[])
    left, prev = float(budget), m.init_action
    for w in way:
        clear(left, 0.0)
        used = 0
        while True:
            u = twin.random_sample(3)
            used += 1
            trial = low + (high - low) * u
            rec["u"].append(u)
            c = ref_actions.action_costs(trial, prev, UAV)
            clear(left, c)
            if np.array_equal(trial, w):
                break
            assert left - c < 0 and used < 101, "the twin stream left the reference's"
        assert used == 101 or left - c >= 0
        rec["prev"].append(np.array(prev, dtype=np.float64)); rec["budget"].append(left); rec["used"].append(used)
        left, prev = left - c, w
    assert left < 0 and rec["used"][-1] == 101  # (the mission ends only behind an iteration that exhausts its trials)
    if len(way) < 3:
        raise NearThreshold("a mission of fewer than three iterations")
    rec["way"] = way
    return {k: np.array(v) for k, v in rec.items()}


def first_clear(fn, candidates):
    for c in candidates:
        try:
            return c, fn(c)
        except NearThreshold:
            continue
    raise SystemExit("no candidate clears the thresholds")


def main():
    out = {}
    for dim in (10, 50):
        for tag, uav in (("dist", None), ("time", UAV)):
            for kind, fn, cuts in (("lawn", lawnmower, (150.0, 151.5, 153.0)), ("spiral", spiral, (60.0, 61.5, 63.0))):
                # (the 50x50 spiral starts at the map's centre, 139 m from the start: a cut below that leaves one waypoint)
                scale = (1.0 if tag == "dist" else 0.6) * (1.0 if dim == 10 else (3.5 if kind == "spiral" else 2.0))
                b, way = first_clear(lambda x: fn(dim, x, uav), [c * scale for c in cuts])
                out[f"{kind}_g{dim}_{tag}_cut"], out[f"{kind}_g{dim}_{tag}_cut_budget"] = way, np.float64(b)
                b, way = first_clear(lambda x: fn(dim, x, uav), [1.0e5, 1.1e5])
                out[f"{kind}_g{dim}_{tag}_all"], out[f"{kind}_g{dim}_{tag}_all_budget"] = way, np.float64(b)
                assert len(out[f"{kind}_g{dim}_{tag}_cut"]) < len(way)
        for adaptive, tag in ((False, "na"), (True, "ad")):
            found, seed = 0, 0
            while found < 3:
                try:
                    rec = discrete(dim, 40.25 if adaptive else 60.25, adaptive, seed)
                    for k, v in rec.items():
                        out[f"disc_g{dim}_{tag}_s{found}_{k}"] = v
                    found += 1
                except NearThreshold:
                    pass
                seed += 1
        found, seed = 0, 0
        while found < 3:
            try:
                rec = continuous(dim, (25.25, 40.25, 12.25)[found], seed)
                for k, v in rec.items():
                    out[f"cont_g{dim}_s{found}_{k}"] = v
                found += 1
            except NearThreshold:
                pass
            seed += 1
    # curves: three runs of unequal length, the second with a repeated time; experiments.py:227-229
    rs = np.random.RandomState(7)
    xs = [np.cumsum(np.r_[0.0, rs.uniform(0.5, 6.0, n)]) for n in (5, 11, 1)]
    xs[1][4] = xs[1][3]
    ys = [rs.uniform(-3.0, 3.0, (len(x), 8)) for x in xs]
    budget = 30.0
    max_x = min(max(np.max(x) for x in xs), budget)
    axis = np.linspace(0, max_x, int(np.ceil(max_x)))
    for i, (x, y) in enumerate(zip(xs, ys)):
        out[f"curve_xs{i}"], out[f"curve_ys{i}"] = x, y
        out[f"curve_interp{i}"] = np.stack([np.interp(axis, x, y[:, v]) for v in range(8)], axis=1)
    out["curve_budget"], out["curve_axis"] = np.float64(budget), axis
    np.savez_compressed(OUT, **out)
    print(f"baselines.npz  {os.path.getsize(OUT) / 1024:.1f} KiB  ({len(out)} arrays)")


if __name__ == "__main__":
    main()
