#!/usr/bin/env python3
"""
Generate tests/golden/priors_nu.npz by IMPORTING the reference (/root/reference, read-only) with mapping.nu set to each of the
Matern smoothness values other than the example config's 1.5 that sklearn evaluates in closed form: 0.5, 2.5 and inf (RBF).
The prior is the reference Mapping's ConstantKernel(sigma^2) * Matern(length_scale, nu) through an unfitted
GaussianProcessRegressor (mapping/mappings.py:236-261).

Recorded per nu, under the key prefix "nu05_", "nu25_" or "nuinf_":
  * priors, as gen_golden.gen_priors records them for nu = 1.5: P0_10 (the full prior on 10x10), P0_50_rows (rows 0, 1234,
    2499 on 50x50), P0_50_diag, and shuffle: four shuffle_prior_cov draws on 10x10, rows of (sigma^2, l, P0[0,0], P0[0,1],
    P0[0,11], P0[5,99]);
  * the episodes episode_rf1_20_s0, episode_mixed_20_s4 and episode_rf1_50_s0 rerun by gen_golden.run_episode's procedure
    (same seeds, altitudes and actions), as "<prefix><episode>_<field>": per step the reward of simulate_prediction_step,
    trace, diag, mean, z, m and rf, then P_final_rows and P_final_proj = P_final @ proj_vectors(N): the whole final matrix
    seen through four fixed random vectors (the full matrices of the 20x20 episodes would be 3.6 MB); diag, mean and
    P_final_rows in fp32.  The observations do not depend on the prior:
    z and the actions are asserted equal to the nu = 1.5 fixture's.
Numeric arrays only.

Usage:  python tests/golden/gen_prior_golden.py        (writes tests/golden/priors_nu.npz; gen_golden.py is not touched)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_golden  # noqa: E402,F401  (puts the reference on sys.path and stubs cv2; generates nothing on import)
from gen_golden import action_list, build, load_params  # noqa: E402
from mapping.grid_maps import GridMap  # noqa: E402
from mapping.mappings import Mapping  # noqa: E402
from sensors.models.sensor_model_factories import SensorModelFactory  # noqa: E402
from sensors.sensor_factories import SensorFactory  # noqa: E402
from simulations.simulation_factories import SimulationFactory  # noqa: E402
from planning.common.optimization import simulate_prediction_step  # noqa: E402

NUS = (("nu05_", 0.5), ("nu25_", 2.5), ("nuinf_", float("inf")))
EPISODES = (("episode_rf1_20_s0", 20, 0, list(range(5, 11))), ("episode_mixed_20_s4", 20, 4, list(range(5, 15))),
            ("episode_rf1_50_s0", 50, 0, list(range(5, 11))))


def params_nu(dim, nu):
    p = load_params(dim, dim)
    p["mapping"]["nu"] = nu
    return p


def priors(nu):
    _, _, _, mp10 = build(params_nu(10, nu), seed=0)
    _, _, _, mp50 = build(params_nu(50, nu), seed=0)
    P50 = mp50.grid_map.cov_matrix
    draws = []
    for seed in range(4):  # (gen_golden.gen_priors)
        np.random.seed(seed)
        params = params_nu(10, nu)
        gm = GridMap(params)
        sm = SensorModelFactory(params).create_sensor_model()
        sensor = SensorFactory(params, sm, gm).create_sensor()
        sim = SimulationFactory(params, sensor).create_sensor_simulation()
        sensor.set_sensor_simulation(sim)
        np.random.seed(100 + seed)
        mp = Mapping(gm, sensor, shuffle_prior_cov=True)
        np.random.seed(100 + seed)
        sv = np.random.uniform(low=0.8 * 1.82, high=1.2 * 1.82)
        ls = np.random.uniform(low=0.8 * 3.67, high=1.2 * 3.67)
        P = mp.grid_map.cov_matrix
        draws.append([sv, ls, P[0, 0], P[0, 1], P[0, 11], P[5, 99]])
    return {"P0_10": mp10.grid_map.cov_matrix, "P0_50_rows": P50[[0, 1234, 2499]], "P0_50_diag": np.diag(P50).copy(),
            "shuffle": np.array(draws)}


def episode(tag, dim, seed, altitudes, nu):
    """gen_golden.run_episode (:266-323) with mapping.nu = nu."""
    ref = np.load(os.path.join(HERE, tag + ".npz"))
    steps = len(ref["actions"])
    params = params_nu(dim, nu)
    np.random.seed(seed)
    st0 = np.random.get_state()
    gm, sensor, sim, mapping = build(params)  # consumes dim*dim normals for the GRF
    np.random.set_state(st0)
    np.random.normal(size=(dim, dim))  # the white-noise draw run_episode observes: the stream is where it is there
    acts = action_list(dim, dim, 4, steps, 1000 + seed, altitudes)
    assert np.array_equal(acts, ref["actions"]), tag
    uav = {"max_v": 2, "max_a": 2}
    prev = np.array([2.0, 2.0, 14.0])
    rec = {k: [] for k in ("reward", "trace", "diag", "mean", "z", "m", "rf")}
    for a in acts:
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        reward, _, P_pred = simulate_prediction_step(gm.cov_matrix, prev, a, mapping, uav, info)
        rf = sensor.get_resolution_factor(a)
        st = np.random.get_state()
        z = sensor.take_measurement(a, verbose=False)
        np.random.set_state(st)
        np.random.normal(0, 1, z.shape)  # (run_episode draws eps at the same stream position)
        mapping.update_grid_map(a, z)
        assert np.array_equal(gm.cov_matrix, P_pred)
        zp = np.zeros(9)
        zp[: z.size] = z.ravel()
        rec["reward"].append(reward)
        rec["trace"].append(np.trace(gm.cov_matrix))
        rec["diag"].append(np.diag(gm.cov_matrix).copy())
        rec["mean"].append(gm.mean.copy())
        rec["z"].append(zp)
        rec["m"].append(z.size)
        rec["rf"].append(rf)
        prev = a
    out = {k: np.array(v) for k, v in rec.items()}
    assert np.array_equal(out["z"], ref["z"]) and np.array_equal(out["m"], ref["m"]), tag  # observations are prior-free
    out["actions"] = acts
    out["P_final_rows"] = gm.cov_matrix[ref["sample_rows"]]
    if dim <= 20:
        out["P_final_proj"] = gm.cov_matrix @ proj_vectors(dim * dim)
    return out


def proj_vectors(n):
    """The probe vectors of P_final_proj (tests/test_hip_prior_kernels.py draws the same ones)."""
    return np.random.RandomState(12345).standard_normal((n, 4))


def main():
    arrays = {}
    for prefix, nu in NUS:
        print(f"nu = {nu}")
        for k, v in priors(nu).items():
            arrays[prefix + k] = np.asarray(v, dtype=np.float64)
        for tag, dim, seed, alts in EPISODES:
            for k, v in episode(tag, dim, seed, alts, nu).items():
                # (the per-step maps and the final matrix in fp32: the engine is checked against them to 1e-5, and they are
                # most of the file)
                arrays[f"{prefix}{tag}_{k}"] = np.asarray(v, dtype=np.float32) if k in ("diag", "mean", "P_final_rows") else np.asarray(v)
    path = os.path.join(HERE, "priors_nu.npz")
    np.savez_compressed(path, **arrays)
    print(f"  priors_nu.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
