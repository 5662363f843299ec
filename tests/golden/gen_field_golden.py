#!/usr/bin/env python3
"""
Generate tests/golden/fields.npz by IMPORTING the reference (/root/reference, read-only) and running its HotspotRandomField and
SplitRandomField (simulations/simulations.py:50-123) under sensor.simulation.type = hotspot_random_field / split_random_field.

Recorded per kind ("hotspot_" / "split_"):
  * for each grid in GRIDS, cluster_radius in RADII (the hotspot combinations whose rejection loop terminates) and seed in SEEDS,
    under "<kind>_<dim>_r<radius>_s<seed>_": the map ("map"), the next np.random.random() after the constructor ("next": the
    stream was consumed identically), and the record the reference drew ("inside", "outside", "rect" [2][4] = {y0, y1, x0, x1},
    rect[1] empty for split), reconstructed from the values its np.random calls returned (logged while it ran);
  * one episode on 20x20 (seed EPISODE_SEED, cluster_radius 5, mixed altitudes 5..14 so that both resolution factors occur) through
    the reference's Mapping / take_measurement / simulate_prediction_step, under "<kind>_episode_": actions, gt, per step the reward,
    z (zero padded to 9), m and rf, and the final mean and diagonal.
Numeric arrays only.

Usage:  python tests/golden/gen_field_golden.py        (writes tests/golden/fields.npz; the other fixtures are not touched)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_golden  # noqa: E402,F401  (puts the reference on sys.path and stubs cv2 / imageio; generates nothing on import)
from gen_golden import action_list, build, load_params  # noqa: E402
from planning.common.optimization import simulate_prediction_step  # noqa: E402

KINDS = (("hotspot_", "hotspot_random_field"), ("split_", "split_random_field"))
GRIDS = (20, 50, 100)
RADII = (3, 5, 2.5)
SEEDS = (0, 1, 2)
EPISODE_DIM, EPISODE_SEED, EPISODE_STEPS, EPISODE_RADIUS = 20, 7, 10, 5


def params_for(dim, sim_type, radius):
    p = load_params(dim, dim)
    p["sensor"]["simulation"] = {"type": sim_type, "cluster_radius": radius}
    return p


def radius_tag(r):
    return str(r).replace(".", "p")


class DrawLog:
    """Logs what np.random.uniform / randint / rand return while the reference's constructor runs."""
    NAMES = ("uniform", "randint", "rand")

    def __enter__(self):
        self.values, self.saved = [], {n: getattr(np.random, n) for n in self.NAMES}
        for n in self.NAMES:
            fn = self.saved[n]
            setattr(np.random, n, (lambda f: lambda *a, **k: self._log(f(*a, **k)))(fn))
        return self

    def _log(self, v):
        self.values.append(v)
        return v

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(np.random, n, fn)


def record_from_draws(prefix, draws, dim, r):
    """The reference's field as (inside, outside, rect[2][4]) from its logged draws (simulations/simulations.py:56-123)."""
    rect = np.zeros((2, 4), dtype=np.int32)
    if prefix == "hotspot_":
        high, low, yc, xc = draws[:4]
        yc2, xc2 = draws[-2:]  # (the pair the rejection loop accepted)
        for q, (cy, cx) in enumerate(((yc, xc), (yc2, xc2))):
            rect[q] = (int(max(cy - r, 0)), int(min(cy + r, dim)), int(max(cx - r, 0)), int(min(cx + r, dim)))
        return high, low, rect
    high, low, swap, axis, s = draws
    first, second = (low, high) if swap > 0.5 else (high, low)
    rect[0] = (0, s, 0, dim) if axis > 0.5 else (0, dim, 0, s)
    return first, second, rect


def hotspot_terminates(dim, r):
    """The reference's rejection loop ends for every first centre (else it hangs: such combinations are not recorded)."""
    lo = int(r)
    if lo >= dim:
        return False
    for c in range(lo, dim):
        if not any(abs(c2 - c) > r for c2 in range(lo, dim)):
            return False
    return True


def maps(prefix, sim_type):
    out = {}
    for dim in GRIDS:
        for r in RADII:
            if prefix == "hotspot_" and not hotspot_terminates(dim, r):
                continue
            for seed in SEEDS:
                np.random.seed(seed)
                with DrawLog() as log:
                    gm, sensor, sim, _ = build(params_for(dim, sim_type, r))
                nxt = np.random.random()
                inside, outside, rect = record_from_draws(prefix, log.values, dim, r)
                key = f"{prefix}{dim}_r{radius_tag(r)}_s{seed}_"
                out[key + "map"] = sim.ground_truth_map
                out[key + "next"] = np.array(nxt)
                out[key + "inside"], out[key + "outside"], out[key + "rect"] = np.array(inside), np.array(outside), rect
    return out


def episode(prefix, sim_type):
    dim, seed = EPISODE_DIM, EPISODE_SEED
    np.random.seed(seed)
    gm, sensor, sim, mapping = build(params_for(dim, sim_type, EPISODE_RADIUS))
    acts = action_list(dim, dim, 4, EPISODE_STEPS, 1000 + seed, list(range(5, 15)))
    uav = {"max_v": 2, "max_a": 2}
    prev = np.array([2.0, 2.0, 14.0])
    rec = {k: [] for k in ("reward", "z", "m", "rf")}
    for a in acts:
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        reward, _, _ = simulate_prediction_step(gm.cov_matrix, prev, a, mapping, uav, info)
        rf = sensor.get_resolution_factor(a)
        z = sensor.take_measurement(a, verbose=False)
        mapping.update_grid_map(a, z)
        zp = np.zeros(9)
        zp[: z.size] = z.ravel()
        rec["reward"].append(reward)
        rec["z"].append(zp)
        rec["m"].append(z.size)
        rec["rf"].append(rf)
        prev = a
    assert set(rec["rf"]) == {1, 2}, rec["rf"]
    out = {prefix + "episode_" + k: np.array(v) for k, v in rec.items()}
    out.update({prefix + "episode_actions": acts, prefix + "episode_gt": sim.ground_truth_map, prefix + "episode_seed": np.array(seed),
                prefix + "episode_radius": np.array(float(EPISODE_RADIUS)), prefix + "episode_mean": gm.mean.copy(),
                prefix + "episode_diag": np.diag(gm.cov_matrix).copy()})
    return out


def main():
    arrays = {}
    for prefix, sim_type in KINDS:
        print(sim_type)
        arrays.update(maps(prefix, sim_type))
        arrays.update(episode(prefix, sim_type))
    path = os.path.join(HERE, "fields.npz")
    np.savez_compressed(path, **arrays)
    print(f"  fields.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
