#!/usr/bin/env python3
"""
Generate the golden vectors under tests/golden/ by IMPORTING the reference
(/root/reference, read-only) in this container and recording its outputs.

The reference is Python and cannot travel to the GPU box; these small .npz
fixtures (inputs + expected outputs only -- no reference source text) can.
Vector list: SURVEY.md section 8(c), items 1-11.

cv2 / imageio are not installed here.  The reference imports them at module
level (simulations/simulations.py:4-5, simulations/sensor_manipulations.py:1),
so stub modules are injected.  The cv2.resize stub is this repo's own
restatement of INTER_AREA (oracle.ipp_oracle.area_resize); therefore every
fixture value that passed through it (rf=2 observations ``z`` and anything
downstream of them) is tagged ``unpinned_*`` -- it pins nothing about OpenCV.

Usage:  python tests/golden/gen_golden.py        (writes tests/golden/*.npz)
"""
import os
import sys
import types

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden")

if not os.path.isdir(REF):
    sys.exit("reference checkout not present: golden vectors can only be generated in the build container")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import yaml  # noqa: E402
import matplotlib  # noqa: E402

matplotlib.use("Agg")

from oracle import ipp_oracle as orc  # noqa: E402

cv2 = types.ModuleType("cv2")
cv2.INTER_AREA = 3
RESIZE_CALLS = []


def _resize(src, dsize=None, interpolation=None):
    RESIZE_CALLS.append((tuple(src.shape), tuple(int(v) for v in dsize)))
    return orc.area_resize(np.asarray(src, dtype=np.float64), dsize)


cv2.resize = _resize
sys.modules["cv2"] = cv2
sys.modules["imageio"] = types.ModuleType("imageio")

from mapping.grid_maps import GridMap  # noqa: E402
from mapping.mappings import Mapping  # noqa: E402
from sensors.models.sensor_model_factories import SensorModelFactory  # noqa: E402
from sensors.sensor_factories import SensorFactory  # noqa: E402
from simulations.simulation_factories import SimulationFactory  # noqa: E402
from simulations import ground_truths  # noqa: E402
from planning.common.optimization import simulate_prediction_step, greedy_search  # noqa: E402
from planning.common.rewards import compute_adaptive_msk, compute_reward  # noqa: E402
from planning.common import actions as ref_actions  # noqa: E402
from planning import evaluation_metrics as ref_metrics  # noqa: E402


def load_params(x_dim, y_dim, resolution=4):
    with open(os.path.join(REF, "config", "example.yaml")) as fh:
        params = yaml.safe_load(fh)
    params["environment"].update(x_dim=x_dim, y_dim=y_dim, resolution=resolution)
    return params


def build(params, seed=None, shuffle_prior_cov=False):
    if seed is not None:
        np.random.seed(seed)
    gm = GridMap(params)
    sm = SensorModelFactory(params).create_sensor_model()
    sensor = SensorFactory(params, sm, gm).create_sensor()
    sim = SimulationFactory(params, sensor).create_sensor_simulation()
    sensor.set_sensor_simulation(sim)
    mapping = Mapping(gm, sensor, shuffle_prior_cov=shuffle_prior_cov)
    return gm, sensor, sim, mapping


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


# ----------------------------------------------------------------------------- 1. footprint table
def gen_footprints():
    rows = []
    for res in (1, 4):
        params = load_params(400, 400, res)
        gm = GridMap(params)
        sm = SensorModelFactory(params).create_sensor_model()
        sensor = SensorFactory(params, sm, gm).create_sensor()
        for alt in range(4, 31):
            pos = np.array([200.0 * res + 0.5 * res, 200.0 * res + 0.5 * res, float(alt)])
            rx, ry = sensor.field_of_view_range(pos[2])
            xl, xr, yu, yd = sensor.project_field_of_view(pos)
            rows.append([res, alt, rx, ry, (xr - xl) // 2, (yd - yu) // 2, sensor.get_resolution_factor(pos),
                         sm.get_noise_variance(pos)])
    table = np.array(rows, dtype=np.float64)

    params = load_params(50, 50, 4)
    gm = GridMap(params)
    sm = SensorModelFactory(params).create_sensor_model()
    sensor = SensorFactory(params, sm, gm).create_sensor()
    positions, fovs = [], []
    W = 50 * 4
    xy = [2.0, 6.0, 98.0, 102.0, 190.0, 194.0, 198.0, 199.99, float(W), 0.0, 3.999, 4.0, 57.3, 123.456]
    for alt in (5.0, 8.0, 10.0, 10.000001, 11.0, 13.0, 14.0, 20.0, 27.0, 30.0):
        for x in xy:
            for y in (2.0, 102.0, 198.0, float(W), 0.0, 77.7):
                p = np.array([x, y, alt])
                positions.append(p)
                fovs.append(sensor.project_field_of_view(p))
    save("footprints", table=table, positions=np.array(positions), fovs=np.array(fovs, dtype=np.int64))


# ----------------------------------------------------------------------------- 2. H rows
def gen_measurement_model():
    params = load_params(10, 12, 4)  # non-square on purpose: flat index = x_dim * row + col
    gm = GridMap(params)
    sm = SensorModelFactory(params).create_sensor_model()
    fovs, rfs, ms, Hs, R00 = [], [], [], [], []
    for rf in (1, 2):
        for w in range(1, 6):
            for h in range(1, 6):
                xl, yu = 2, 3
                fov = (xl, xl + w - 1, yu, yu + h - 1)
                m = int(np.ceil(w / rf) * np.ceil(h / rf))
                H = sm.measurement_model_matrix(gm, fov, m, rf)
                pos = np.array([0.0, 0.0, 14.0 if rf == 2 else 8.0])
                R = sm.measurement_variance_matrix(pos, m, rf)
                fovs.append(fov)
                rfs.append(rf)
                ms.append(m)
                Hpad = np.zeros((25, gm.num_grid_cells))
                Hpad[:m] = H
                Hs.append(Hpad)
                R00.append(R[0, 0])
    save("measurement_model", fovs=np.array(fovs), rfs=np.array(rfs), ms=np.array(ms), H=np.array(Hs),
         R00=np.array(R00), x_dim=np.array(10), y_dim=np.array(12))


# ----------------------------------------------------------------------------- 3. priors
def gen_priors():
    _, _, _, mp10 = build(load_params(10, 10), seed=0)
    _, _, _, mp50 = build(load_params(50, 50), seed=0)
    P50 = mp50.grid_map.cov_matrix
    draws = []
    for seed in range(4):
        np.random.seed(seed)
        params = load_params(10, 10)
        gm = GridMap(params)
        sm = SensorModelFactory(params).create_sensor_model()
        sensor = SensorFactory(params, sm, gm).create_sensor()
        sim = SimulationFactory(params, sensor).create_sensor_simulation()
        sensor.set_sensor_simulation(sim)
        np.random.seed(100 + seed)
        mp = Mapping(gm, sensor, shuffle_prior_cov=True)
        # recover the drawn (sigma^2, l): P0[0,0] = sigma^2 ; then solve l from P0[0,1]
        np.random.seed(100 + seed)
        sv = np.random.uniform(low=0.8 * 1.82, high=1.2 * 1.82)
        ls = np.random.uniform(low=0.8 * 3.67, high=1.2 * 3.67)
        draws.append([sv, ls, mp.grid_map.cov_matrix[0, 0], mp.grid_map.cov_matrix[0, 1], mp.grid_map.cov_matrix[0, 11],
                      mp.grid_map.cov_matrix[5, 99]])
    # non-GP branch (mappings.py:219-233) on a tiny grid
    params = load_params(6, 6)
    params["mapping"]["fit_gaussian_process"] = False
    np.random.seed(7)
    _, _, _, mp_rand = build(params)  # GRF draw first, then the N x N normal draw
    save("priors", P0_10=mp10.grid_map.cov_matrix, mean_10=mp10.grid_map.mean, P0_50_rows=P50[[0, 1234, 2499]],
         P0_50_diag=np.diag(P50).copy(), shuffle=np.array(draws), P0_rand_6=mp_rand.grid_map.cov_matrix)


# ----------------------------------------------------------------------------- 4. predict steps
def action_list(x_dim, y_dim, res, n, seed, altitudes):
    rs = np.random.RandomState(seed)
    acts = []
    for _ in range(n):
        j, i = rs.randint(0, x_dim), rs.randint(0, y_dim)
        acts.append([res * j + 0.5 * res, res * i + 0.5 * res, float(altitudes[rs.randint(0, len(altitudes))])])
    return np.array(acts)


def gen_predict():
    uav = {"max_v": 2, "max_a": 2}
    for tag, dim, n in (("10", 10, 36), ("50", 50, 8)):
        params = load_params(dim, dim)
        gm, sensor, sim, mapping = build(params, seed=11)
        acts = action_list(dim, dim, 4, n, 5, list(range(5, 15)))
        # border / corner / boundary cases up front
        acts[0] = [2, 2, 14]
        acts[1] = [4 * dim - 2, 4 * dim - 2, 14]
        acts[2] = [2, 4 * dim - 2, 8]
        acts[3] = [4 * dim - 2, 2, 11]
        acts[4] = [4 * (dim // 2) + 2, 2, 13]
        acts[5] = [2, 4 * (dim // 2) + 2, 5]
        P = gm.cov_matrix.copy()
        mean = gm.mean.copy()
        rs = np.random.RandomState(3)
        prev = np.array([2.0, 2.0, 14.0])
        rec = {k: [] for k in ("reward", "mask", "S", "Wc", "diag", "trace", "cost", "m", "fov", "rf", "mode")}
        P_seq = []
        sample_rows = np.array([0, dim, dim * dim // 2 + 3, dim * dim - 1, 7, 3 * dim + 1, dim * dim // 3, dim * dim - dim])
        rows_seq = []
        for t, a in enumerate(acts):
            mode = t % 4
            # mode 0: adaptive k=0 + flight time; 1: non-adaptive + distance; 2: adaptive k=2 + flight time; 3: adaptive k=0 + distance
            mean_t = np.clip(mean + 0.25 * rs.standard_normal(mean.shape), 0, 1) if mode != 1 else mean
            info = None
            if mode in (0, 3):
                info = {"mean": mean_t, "value_threshold": 0.4, "interval_factor": 0}
            elif mode == 2:
                info = {"mean": mean_t, "value_threshold": 0.9, "interval_factor": 2}
            u = uav if mode in (0, 2) else None
            reward, _, P_next = simulate_prediction_step(P, prev, a, mapping, u, info)
            mask = np.ones(dim * dim, bool) if info is None else compute_adaptive_msk(
                info["mean"], P, info["value_threshold"], info["interval_factor"])
            rf = sensor.get_resolution_factor(a)
            fov = sensor.project_field_of_view(a)
            xl, xr, yu, yd = fov
            m = int(np.ceil((xr - xl + 1) / rf) * np.ceil((yd - yu + 1) / rf))
            H = sensor.sensor_model.measurement_model_matrix(gm, fov, m, rf)
            R = sensor.sensor_model.measurement_variance_matrix(a, m, rf)
            S = H @ P @ H.T + R
            S = 0.5 * (S + S.T)
            Lu = np.linalg.cholesky(S).T
            Wc = P @ (H.T @ np.linalg.inv(Lu))
            Wpad = np.zeros((dim * dim, 9))
            Wpad[:, :m] = Wc
            Spad = np.zeros((9, 9))
            Spad[:m, :m] = S
            rec["reward"].append(reward)
            rec["mask"].append(mask)
            rec["S"].append(Spad)
            rec["Wc"].append(Wpad)
            rec["diag"].append(np.diag(P_next).copy())
            rec["trace"].append(np.trace(P_next))
            rec["cost"].append(ref_actions.action_costs(a, prev, u))
            rec["m"].append(m)
            rec["fov"].append(fov)
            rec["rf"].append(rf)
            rec["mode"].append(mode)
            rows_seq.append(P_next[sample_rows].copy())
            if dim == 10 and t < 12:
                P_seq.append(P_next.copy())
            rec.setdefault("mean_used", []).append(mean_t.copy())
            P, prev = P_next, a
        out = {k: np.array(v) for k, v in rec.items()}
        out.update(actions=acts, P0=gm.cov_matrix if dim == 10 else gm.cov_matrix[sample_rows],
                   sample_rows=sample_rows, rows=np.array(rows_seq), checksum=np.array([P.sum(), (P ** 2).sum()]))
        if dim == 10:
            out["P_seq"] = np.array(P_seq)
            out["P_final"] = P
        save(f"predict_{tag}", **out)


# ----------------------------------------------------------------------------- 5/6. episodes (predict + observe + update)
def run_episode(dim, seed, steps, altitudes, tag):
    params = load_params(dim, dim)
    np.random.seed(seed)
    st0 = np.random.get_state()
    gm, sensor, sim, mapping = build(params)  # consumes dim*dim normals for the GRF
    np.random.set_state(st0)
    white = np.random.normal(size=(dim, dim))  # identical draw, now observed
    acts = action_list(dim, dim, 4, steps, 1000 + seed, altitudes)
    uav = {"max_v": 2, "max_a": 2}
    prev = np.array([2.0, 2.0, 14.0])
    rec = {k: [] for k in ("reward", "trace", "diag", "mean", "z", "eps", "m", "rf", "unpinned_z")}
    Wcs = []
    for a in acts:
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        reward, _, P_pred = simulate_prediction_step(gm.cov_matrix, prev, a, mapping, uav, info)
        rf = sensor.get_resolution_factor(a)
        st = np.random.get_state()
        z = sensor.take_measurement(a, verbose=False)
        np.random.set_state(st)
        eps = np.random.normal(0, 1, z.shape)  # same stream position: z = clip(ds + nv * eps)
        P_before = gm.cov_matrix
        mapping.update_grid_map(a, z)
        assert np.array_equal(gm.cov_matrix, P_pred)
        d = np.diag(P_before) - np.diag(gm.cov_matrix)
        zp, ep = np.zeros(9), np.zeros(9)
        zp[: z.size], ep[: z.size] = z.ravel(), eps.ravel()
        rec["reward"].append(reward)
        rec["trace"].append(np.trace(gm.cov_matrix))
        rec["diag"].append(np.diag(gm.cov_matrix).copy())
        rec["mean"].append(gm.mean.copy())
        rec["z"].append(zp)
        rec["eps"].append(ep)
        rec["m"].append(z.size)
        rec["rf"].append(rf)
        rec["unpinned_z"].append(rf > 1)
        Wcs.append(d)
        prev = a
    gt = sim.ground_truth_map
    m_rmse = ref_metrics.root_mean_squared_error(gt, gm.mean)
    msk = gt.flatten(order="C") >= 0.4
    metrics = np.array([
        m_rmse,
        ref_metrics.root_mean_squared_error(gt, gm.mean, msk),
        ref_metrics.weighted_root_mean_squared_error(gt, gm.mean),
        ref_metrics.mean_log_loss(gt, gm.mean, gm.cov_matrix),
        ref_metrics.weighted_mean_log_loss(gt, gm.mean, gm.cov_matrix),
        ref_metrics.map_uncertainty(gm.cov_matrix),
        ref_metrics.map_uncertainty(gm.cov_matrix, msk),
        ref_metrics.map_uncertainty_difference(gm.cov_matrix, msk),
    ])
    out = {k: np.array(v) for k, v in rec.items()}
    sample_rows = np.array([0, dim + 1, dim * dim // 2 + 3, dim * dim - 1])
    out.update(actions=acts, white=white, gt=gt, metrics=metrics, P_final_rows=gm.cov_matrix[sample_rows],
               sample_rows=sample_rows, seed=np.array(seed))
    if dim <= 20 and seed in (0, 4):
        out["P_final"] = gm.cov_matrix
    save(tag, **out)


def gen_episodes():
    for seed in range(4):
        run_episode(20, seed, 40, list(range(5, 11)), f"episode_rf1_20_s{seed}")  # fully pinned (rf = 1 only)
    run_episode(20, 4, 40, list(range(5, 15)), "episode_mixed_20_s4")  # rf=2 observations unpinned
    run_episode(50, 0, 40, list(range(5, 11)), "episode_rf1_50_s0")
    run_episode(50, 1, 40, list(range(5, 15)), "episode_mixed_50_s1")


# ----------------------------------------------------------------------------- 7. GRF
def gen_grf():
    out = {}
    for n in (10, 50, 100):
        np.random.seed(20 + n)
        st = np.random.get_state()
        fld = ground_truths.gaussian_random_field(lambda k: k ** (-5), n, n)
        np.random.set_state(st)
        white = np.random.normal(size=(n, n))
        out[f"white_{n}"] = white
        out[f"field_{n}"] = fld
    # odd size: last row / column of the amplitude stay zero (ground_truths.py:7-11)
    np.random.seed(77)
    st = np.random.get_state()
    fld = ground_truths.gaussian_random_field(lambda k: k ** (-5), 9, 9)
    np.random.set_state(st)
    out["white_9"] = np.random.normal(size=(9, 9))
    out["field_9"] = fld
    out["fft_indices_8"] = np.array(ground_truths.fft_indices(8))
    out["fft_indices_9"] = np.array(ground_truths.fft_indices(9))
    save("grf", **out)


# ----------------------------------------------------------------------------- 10. Cholesky fallback
def gen_fallback():
    params = load_params(6, 6)
    gm, sensor, sim, mapping = build(params, seed=5)
    P = gm.cov_matrix.copy()
    H = np.zeros((3, 36))
    H[0, [7, 8]] = 0.5
    H[1, [7, 8]] = 0.5  # duplicated row
    H[2, 14] = 1.0
    R = np.zeros((3, 3))  # R = 0 -> S singular -> LinAlgError or garbage-free fallback
    mean = gm.mean.copy()
    z = np.array([0.7, 0.7, 0.2])
    # make S exactly singular-indefinite so cholesky raises deterministically
    R[0, 0] = -1e-3
    import logging
    logging.disable(logging.CRITICAL)
    x, Pn = Mapping.kalman_filter_update(P, H, R, grid_mean=mean, observation=z, cov_only=False)
    logging.disable(logging.NOTSET)
    save("fallback", P=P, H=H, R=R, mean=mean, z=z, x_new=x, P_new=Pn)


# ----------------------------------------------------------------------------- 11. greedy harness pin (config 1 plumbing)
def gen_greedy():
    out = {}
    for dim, seed in ((10, 3), (20, 3)):
        params = load_params(dim, dim)
        gm, sensor, sim, mapping = build(params, seed=seed)
        uav = {"max_v": 2, "max_a": 2}
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        prev = np.array([2.0, 2.0, 14.0])
        wps = greedy_search(prev, 200, gm.cov_matrix, 3, mapping, 8, 14, 6, uav, info)
        cands = ref_actions.get_actions(prev, 200, gm, 8, 14, 6, uav)
        rewards = [simulate_prediction_step(gm.cov_matrix, prev, a, mapping, uav, info)[0] for a in cands]
        out[f"waypoints_{dim}"] = np.array(wps)
        out[f"candidates_{dim}"] = np.array(cands)
        out[f"rewards_{dim}"] = np.array(rewards)

    # full rf=1-only greedy mission loop (planning/greedy_mission.py:73-110 restated as a driver; budget 60)
    dim = 10
    params = load_params(dim, dim)
    np.random.seed(9)
    st0 = np.random.get_state()
    gm, sensor, sim, mapping = build(params)
    np.random.set_state(st0)
    white = np.random.normal(size=(dim, dim))
    uav = {"max_v": 2, "max_a": 2}
    prev = np.array([2.0, 2.0, 14.0])
    budget = 60.0
    wps, traces, rmses, budgets, eps_all = [], [], [], [], []
    while budget >= 0:
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        w = greedy_search(prev, budget, gm.cov_matrix, 1, mapping, 6, 10, 2, uav, info)
        if len(w) == 0:
            break
        nxt = np.array(w[0])
        st = np.random.get_state()
        z = sensor.take_measurement(nxt, verbose=False)
        np.random.set_state(st)
        eps = np.random.normal(0, 1, z.shape)
        mapping.update_grid_map(nxt, z)
        budget -= ref_actions.action_costs(nxt, prev, uav)
        prev = nxt
        wps.append(nxt)
        traces.append(np.trace(gm.cov_matrix))
        rmses.append(ref_metrics.root_mean_squared_error(sim.ground_truth_map, gm.mean))
        budgets.append(budget)
        ep = np.zeros(9)
        ep[: eps.size] = eps.ravel()
        eps_all.append(ep)
    out.update(mission_white=white, mission_waypoints=np.array(wps), mission_traces=np.array(traces),
               mission_rmse=np.array(rmses), mission_budget=np.array(budgets), mission_eps=np.array(eps_all),
               mission_final_mean=gm.mean)
    save("greedy", **out)


# ----------------------------------------------------------------------------- flight time table (a13)
def gen_costs():
    rs = np.random.RandomState(2)
    a = rs.uniform(0, 200, size=(64, 3))
    b = rs.uniform(0, 200, size=(64, 3))
    b[:8] = a[:8] + rs.uniform(-0.5, 0.5, size=(8, 3))  # short hops: d/2 < v^2/(2a)
    b[8] = a[8]  # zero distance
    uav = {"max_v": 2, "max_a": 2}
    uav2 = {"max_v": 5.0, "max_a": 1.5}
    save("costs", a=a, b=b,
         dist=np.array([ref_actions.action_costs(x, y, None) for x, y in zip(a, b)]),
         t_v2a2=np.array([ref_actions.action_costs(x, y, uav) for x, y in zip(a, b)]),
         t_v5a15=np.array([ref_actions.action_costs(x, y, uav2) for x, y in zip(a, b)]),
         t_vec=ref_actions.compute_flight_times(a, b[0], uav))


# ----------------------------------------------------------------------------- NN input feature planes (8(f) rank 3)
def gen_features():
    """planning/common/features.py:83-151 on a 10x10 grid: history of covariance states -> masked, min-max
    normalised N x N planes + position / budget / cost planes.  The reference masks the history's arrays IN PLACE
    (features.py:98-99); copies are passed so that the recorded `states` are the unmasked inputs."""
    from planning.common.features import EpisodeHistory, generate_input_feature_planes

    dim = 10
    params = load_params(dim, dim)
    gm, sensor, sim, mapping = build(params, seed=4)
    uav = {"max_v": 2, "max_a": 2}
    acts = [np.array([2.0, 2.0, 14.0]), np.array([18.0, 22.0, 8.0]), np.array([30.0, 10.0, 9.0])]
    budgets = [200.0, 171.5, 160.25]
    states, means = [gm.cov_matrix.copy()], [gm.mean.copy()]
    for a in acts[1:]:
        z = sensor.take_measurement(a, verbose=False)  # rf = 1 altitudes: pinned
        mapping.update_grid_map(a, z)
        states.append(gm.cov_matrix.copy())
        means.append(gm.mean.copy())
    out = dict(states=np.array(states), positions=np.array(acts), budgets=np.array(budgets), mean=gm.mean.copy())

    def planes(n_hist, adaptive, costs):
        hist = EpisodeHistory(3)
        for k in range(n_hist):  # push order: oldest first, so states[0] of the history is the newest
            hist.push(states[k].copy(), acts[k].copy(), budgets[k])
        info = {"mean": gm.mean.copy(), "value_threshold": 0.4, "interval_factor": 0} if adaptive else None
        return generate_input_feature_planes(mapping, hist, 8, 14, info, uav, use_action_costs_input=costs)

    out["planes_full_adaptive_costs"] = planes(3, True, True)
    out["planes_two_plain"] = planes(2, False, False)
    out["planes_one_adaptive"] = planes(1, True, False)
    save("features", **out)



# ----------------------------------------------------------------------------- 12. MCTS-zero tree search (8(f) rank 1)
class _StubQueues:
    """Stand-in for the inference worker's queues (planning/mcts_zero/inference_workers.py): uniform policy over all
    actions and a value that is a pure function of the request's action mask, so the build's driver can use the same
    stub.  Records every request."""

    def __init__(self, num_actions):
        self.num_actions = num_actions
        self.pending = None
        self.masks = []

    # request queue
    def put(self, msg):
        self.pending = msg
        self.masks.append(np.array(msg["action_msk"], dtype=bool))

    # reply queue
    def get(self):
        msk = np.asarray(self.pending["action_msk"], dtype=bool)
        return {"policy": np.ones(self.num_actions) / self.num_actions, "value": stub_value(msk)}

    def empty(self):
        return False

    get_nowait = get


def stub_value(mask):
    """Leaf value of the stubbed network: depends on the valid-action mask only."""
    return 0.05 * float(int(mask.sum()) % 7) + 0.3


def _record_mcts(cases, **hyper_over):
    """The reference's search on each case (stubbed inference queues) with the example configuration's hyper-parameters, `hyper_over`
    on top: the arrays of the mcts*.npz fixtures."""
    import planning.mcts_zero.mcts as ref_mcts
    from planning.common.features import EpisodeHistory

    out = {}
    for name, dim, adaptive, root_steps, sims, (amin, amax, aspc), budget, horizon, seed in cases:
        params = load_params(dim, dim)
        gm, sensor, sim, mapping = build(params, seed=seed)
        uav = {"max_v": 2, "max_a": 2}
        # the root: a few executed rf = 1 measurements (noisy observations), so that mean and covariance are generic
        rs = np.random.RandomState(100 + seed)
        prev = np.array([2.0, 2.0, 14.0])
        root_actions, root_eps = [], []
        for _ in range(root_steps):
            a = np.array([4.0 * rs.randint(0, dim) + 2.0, 4.0 * rs.randint(0, dim) + 2.0, 8.0])
            st = np.random.get_state()
            z = sensor.take_measurement(a, verbose=False)
            np.random.set_state(st)
            eps = np.random.normal(0, 1, z.shape)
            mapping.update_grid_map(a, z)
            root_actions.append(a)
            ep = np.zeros(9)
            ep[: eps.size] = eps.ravel()
            root_eps.append(ep)
            prev = a
        hyper = dict(params["experiment"]["missions"][0]["hyper_params"])
        hyper.update(num_mcts_simulations=sims, non_blocking_read=False)
        hyper.update(hyper_over)
        scenario = {"value_threshold": 0.4, "interval_factor": 0} if adaptive else None
        meta = {"budget": budget, "initial_budget": budget, "episode_horizon": horizon, "min_altitude": amin,
                "max_altitude": amax, "altitude_spacing": aspc, "uav_specifications": uav, "scenario_info": scenario}
        num_actions = dim * dim * (int((amax - amin) / aspc) + 1)
        queues = _StubQueues(num_actions)
        # The reference's state key is hash(str(P)) (mcts.py:20-21).  NumPy abbreviates arrays of more than 1000 elements to
        # their corners, which makes almost all states of a 10x10 map (100x100 matrix) collide; with the print threshold
        # raised the key sees the whole matrix (printed to 8 digits: states reached by the same measurements in a
        # different order are one node).  The fixtures are recorded in that well-defined regime.
        np.set_printoptions(threshold=sys.maxsize)
        # features.py:98-99 zeroes rows / columns of the LIVE node states in place when adaptive (an aliasing side effect of
        # building network inputs, which the stub ignores anyway): recorded with a non-mutating stand-in.
        ref_mcts.generate_input_feature_planes = lambda *a, **k: None
        mcts = ref_mcts.MCTS(mapping, hyper, meta, queues, queues)
        root = ref_mcts.Node(gm.cov_matrix.copy())
        np.random.seed(1000 + seed)
        policy, valid = mcts.get_policy(root, 0, prev.copy(), budget, EpisodeHistory(hyper["input_history_length"]), temperature=1)
        rep = root.state_representation()
        np.set_printoptions(threshold=1000)
        out.update({
            f"{name}_white": None, f"{name}_dim": dim, f"{name}_adaptive": adaptive, f"{name}_sims": sims, f"{name}_budget": budget,
            f"{name}_horizon": horizon, f"{name}_alts": np.array([amin, amax, aspc], dtype=np.float64), f"{name}_seed": 1000 + seed,
            f"{name}_gt": sim.ground_truth_map, f"{name}_root_actions": np.array(root_actions), f"{name}_root_eps": np.array(root_eps),
            f"{name}_root_mean": gm.mean, f"{name}_root_diag": np.diag(gm.cov_matrix), f"{name}_prev": prev,
            f"{name}_policy": np.array(policy), f"{name}_valid": np.array(valid),
            f"{name}_root_Nsa": mcts.Nsa[rep], f"{name}_root_Qsa": mcts.Qsa[rep], f"{name}_root_Ps": mcts.Ps[rep],
            f"{name}_root_Ns": mcts.Ns[rep], f"{name}_num_nodes": len(mcts.Ps), f"{name}_inferences": mcts.inference_counter,
            f"{name}_revisits": mcts.revisits_counter, f"{name}_new_visits": mcts.new_visits_counter,
            f"{name}_total_Ns": sum(mcts.Ns.values()), f"{name}_mask_sums": np.array([m.sum() for m in queues.masks]),
        })
        out.pop(f"{name}_white")
        print(f"  mcts {name}: {len(mcts.Ps)} nodes, {mcts.inference_counter} inferences, root visits {int(mcts.Ns[rep])}, "
              f"max Nsa {int(mcts.Nsa[rep].max())}, revisits {mcts.revisits_counter}")
    out["hyper_puct_init"] = hyper["puct_init"]
    out["hyper_puct_base"] = hyper["puct_base"]
    out["hyper_forced_playout_factor"] = hyper["forced_playout_factor"]
    out["hyper_max_valid_action_distance"] = hyper["max_valid_action_distance"]
    out["hyper_gamma"] = hyper["gamma"]
    out["hyper_dirichlet_alpha"] = hyper["dirichlet_alpha"]
    out["hyper_dirichlet_eps"] = hyper["dirichlet_eps"]
    return out


def gen_mcts():
    save("mcts", **_record_mcts([
        # name, grid, adaptive, root steps, sims, altitudes (min, max, spacing), budget, horizon, seed
        ("a5", 5, False, 2, 96, (8, 14, 6), 30.0, 3, 3),
        ("b10", 10, True, 3, 80, (8, 14, 6), 40.0, 5, 5),
    ]))


def gen_mcts_decayed():
    """One search with the hyper-parameters training reaches, not the ones it starts from: the discount below 1 and the Dirichlet
    shape at the floor of its schedule (config/example.yaml: dirichlet_alpha decays from 1.0 by 0.8 per iteration down to 0.3), so
    that the noise comes from the shape < 1 branch of the gamma sampler.  Written to its own file: mcts.npz stays as recorded."""
    save("mcts_decayed", **_record_mcts([("d10", 10, True, 3, 80, (8, 14, 6), 40.0, 5, 6)],
                                        gamma=0.9, dirichlet_alpha=0.3, dirichlet_eps=0.25))


def gen_mcts_mission():
    """Recorded searches of the reference's classic MCTS planner (planning/mcts_mission.py: run_simulations_proxy on a root
    with a generic state): eps-greedy rollouts on an adaptive mission and generalised cost-benefit rollouts on a
    non-adaptive one.  The build's ClassicMCTS (ipp-rl_amd/planning/mcts_mission.py) must rebuild the same trees from the
    same seeds (np.random.seed(worker_id * 42 + 1) inside the proxy, random.seed(py_seed) for the UCT ties)."""
    import random

    from planning import mcts_mission as ref_mm

    out = {}
    cases = [
        # name, grid, adaptive, gcb, root steps, sims, (min, max, spacing), budget, horizon, greedy radius [m], seed
        ("eps10", 10, True, False, 3, 40, (8, 14, 6), 60.0, 3, 9.0, 3),
        ("gcb10", 10, False, True, 2, 24, (8, 14, 6), 50.0, 3, 9.0, 5),
    ]
    for name, dim, adaptive, gcb, root_steps, sims, (amin, amax, aspc), budget, horizon, radius, seed in cases:
        params = load_params(dim, dim)
        gm, sensor, sim, mapping = build(params, seed=seed)
        uav = {"max_v": 2, "max_a": 2}
        rs = np.random.RandomState(200 + seed)
        prev = np.array([2.0, 2.0, 14.0])
        root_actions, root_eps = [], []
        for _ in range(root_steps):  # the root: a few executed rf = 1 measurements, so that mean and covariance are generic
            a = np.array([4.0 * rs.randint(0, dim) + 2.0, 4.0 * rs.randint(0, dim) + 2.0, 8.0])
            st = np.random.get_state()
            z = sensor.take_measurement(a, verbose=False)
            np.random.set_state(st)
            eps = np.random.normal(0, 1, z.shape)
            mapping.update_grid_map(a, z)
            root_actions.append(a)
            ep = np.zeros(9)
            ep[: eps.size] = eps.ravel()
            root_eps.append(ep)
            prev = a
        hp = dict(k=4.0, alpha=0.75, epsilon_expand=0.2, epsilon_rollout=0.5, gamma=0.95, c=2.0)
        mis = ref_mm.MCTSMission(mapping, uav, dist_to_boundaries=10, min_altitude=amin, max_altitude=amax, budget=budget,
                                 altitude_spacing=aspc, num_simulations=sims, gamma=hp["gamma"], c=hp["c"], episode_horizon=horizon,
                                 k=hp["k"], alpha=hp["alpha"], epsilon_expand=hp["epsilon_expand"], epsilon_rollout=hp["epsilon_rollout"],
                                 max_greedy_radius=radius, use_gcb_rollout=gcb, adaptive=adaptive, value_threshold=0.4, interval_factor=0)
        root = ref_mm.Node(state=gm.cov_matrix.copy(), parent=None, action=prev.copy())
        py_seed = 50 + seed
        random.seed(py_seed)
        mis.run_simulations_proxy(root, budget, horizon, sims, 0)

        def count(n):
            return 1 + sum(count(c) for c in n.children)

        best = ref_mm.MCTSMission.select_best_child(root)
        out.update({
            f"{name}_dim": dim, f"{name}_adaptive": adaptive, f"{name}_gcb": gcb, f"{name}_sims": sims, f"{name}_budget": budget,
            f"{name}_horizon": horizon, f"{name}_alts": np.array([amin, amax, aspc], dtype=np.float64), f"{name}_radius": radius,
            f"{name}_py_seed": py_seed, f"{name}_gt": sim.ground_truth_map, f"{name}_root_actions": np.array(root_actions),
            f"{name}_root_eps": np.array(root_eps), f"{name}_root_mean": gm.mean, f"{name}_root_diag": np.diag(gm.cov_matrix),
            f"{name}_prev": prev, f"{name}_root_visits": root.visits, f"{name}_root_value_sum": root.value_sum,
            f"{name}_child_actions": np.array([c.action for c in root.children]),
            f"{name}_child_visits": np.array([c.visits for c in root.children]),
            f"{name}_child_value_sums": np.array([c.value_sum for c in root.children], dtype=np.float64),
            f"{name}_child_children": np.array([len(c.children) for c in root.children]),
            f"{name}_tree_nodes": count(root), f"{name}_tree_depth": mis.get_depth(root), f"{name}_best_action": best.action,
        })
        print(f"  mcts_mission {name}: {count(root)} tree nodes, depth {mis.get_depth(root)}, {len(root.children)} root children, "
              f"root value sum {root.value_sum:.4f}, best {best.action}")
    for k2, v2 in dict(k=4.0, alpha=0.75, epsilon_expand=0.2, epsilon_rollout=0.5, gamma=0.95, c=2.0).items():
        out[f"hyper_{k2}"] = v2
    save("mcts_mission", **out)


# ----------------------------------------------------------------------------- 14. call trace of the planners on the class surface
class _Recorder:
    """Ordered record of everything the reference's planners do to the Mapping / GridMap / sensor / simulation objects (and to the
    planning.common reward helpers): attribute reads, assignments, calls -- arguments and results as literals or as numbered
    arrays.  An array OBJECT keeps its number (data flow: a state a call returned and a later call receives is one number),
    so the replay can hand its own earlier results on the way the planner does."""

    def __init__(self):
        self.events, self.arrays, self.by_id, self.keep, self.on = [], [], {}, [], False
        self.as_arg = set()   # arrays first met as an ARGUMENT: the replay needs their values (results only need a digest)
        self.in_args = False

    @staticmethod
    def digest(a):
        """Large results are kept as a digest the replay recomputes on its own result: diagonal, row sums, 64 entries at fixed places."""
        a = np.asarray(a, dtype=np.float64)
        flat = a.ravel()
        idx = np.random.RandomState(a.size).randint(0, a.size, 64)
        parts = [flat[idx], a.reshape(a.shape[0], -1).sum(axis=1)]
        if a.ndim == 2 and a.shape[0] == a.shape[1]:
            parts.append(np.diag(a))
        return np.concatenate(parts)

    def save_into(self, out, prefix):
        for i, a in enumerate(self.arrays):
            if a.size > 400 and i not in self.as_arg:
                out[f"{prefix}_d{i:04d}"] = self.digest(a)
                out[f"{prefix}_s{i:04d}"] = np.array(a.shape, dtype=np.int64)
            else:
                out[f"{prefix}_a{i:04d}"] = a

    def val(self, x):
        if isinstance(x, np.ndarray):
            i = self.by_id.get(id(x))
            if i is not None and not (self.arrays[i].shape == x.shape and np.array_equal(self.arrays[i], x)):
                i = None  # (the object was rewritten in place since: a new value)
            if i is None:
                i = len(self.arrays)
                self.arrays.append(np.array(x, copy=True))
                self.by_id[id(x)] = i
                self.keep.append(x)
                if self.in_args:
                    self.as_arg.add(i)
            return {"a": i}
        if isinstance(x, (tuple, list)):
            return {"t": [self.val(v) for v in x]}
        if isinstance(x, dict):
            return {"d": {str(k): self.val(v) for k, v in x.items()}}
        if x is None or isinstance(x, (bool, str)):
            return {"v": x}
        if isinstance(x, (int, np.integer)):
            return {"v": int(x)}
        if isinstance(x, (float, np.floating)):
            return {"v": float(x)}
        return {"o": type(x).__name__}

    def add(self, kind, obj, name, args=None, kwargs=None, result=None, rng=None):
        if not self.on:
            return
        ev = {"k": kind, "o": obj, "n": name}
        self.in_args = True
        if args is not None:
            ev["args"] = [self.val(a) for a in args]
        if kwargs:
            ev["kw"] = {k: self.val(v) for k, v in kwargs.items()}
        self.in_args = False
        if kind != "set":
            ev["r"] = self.val(result)
        if rng is not None:
            ev["rng"] = rng
        self.events.append(ev)


class _Proxy:
    """Recording stand-in for one object of the class surface; the named children come back wrapped as well."""
    _CHILDREN = {"mapping": ("grid_map", "sensor"), "mapping.sensor": ("sensor_simulation", "sensor_model"), "mapping.grid_map": (),
                 "mapping.sensor.sensor_simulation": (), "mapping.sensor.sensor_model": ()}

    def __init__(self, target, name, rec):
        object.__setattr__(self, "_t", target)
        object.__setattr__(self, "_n", name)
        object.__setattr__(self, "_r", rec)

    def __getattr__(self, k):
        t, n, r = object.__getattribute__(self, "_t"), object.__getattribute__(self, "_n"), object.__getattribute__(self, "_r")
        v = getattr(t, k)
        if k in _Proxy._CHILDREN.get(n, ()):
            return _Proxy(v, n + "." + k, r)
        if callable(v):
            def call(*args, **kwargs):
                rng = None
                if k == "take_measurement" and r.on:  # the observation noise comes from NumPy's global stream: where it stood
                    st = np.random.get_state()
                    rng = len(r.arrays)
                    r.arrays.append(np.array(st[1], dtype=np.uint32))
                    r.arrays.append(np.array([st[2], st[3]], dtype=np.int64))
                    r.arrays.append(np.array([st[4]], dtype=np.float64))
                    r.as_arg.update((rng, rng + 1, rng + 2))  # (stored whole: the replay sets the stream to this state)
                was = r.on
                r.on = False  # (what the call does inside the reference is not the planner's business)
                try:
                    out = v(*args, **kwargs)
                finally:
                    r.on = was
                r.add("call", n, k, args, kwargs, out, rng)
                return out
            return call
        r.add("get", n, k, result=v)
        return v

    def __setattr__(self, k, v):
        t, n, r = object.__getattribute__(self, "_t"), object.__getattribute__(self, "_n"), object.__getattribute__(self, "_r")
        r.add("set", n, k, args=[v])
        setattr(t, k, v)


def _record_fn(rec, module, name):
    """Wrap module.name (a planning.common helper the planner imported by name) so that its calls land in the trace."""
    fn = getattr(module, name)

    def wrapped(*args, **kwargs):
        was = rec.on
        rec.on = False
        try:
            out = fn(*args, **kwargs)
        finally:
            rec.on = was
        rec.add("call", "fn", name, args, kwargs, out)
        return out

    setattr(module, name, wrapped)
    return fn


def gen_call_trace():
    """What planning/mcts_mission.py and the self-play loop of planning/mcts_zero/episode_generators.py DO to the class surface: (i) one
    MCTSMission replan (run_simulations_proxy + select_best_child, the body of replan, :352-389, in this process -- the reference
    pickles the mission into a worker pool, where a recorder would be lost) and the executed step behind it (:404-413, with the
    metric reads of eval, missions.py:176-197); (ii) one self-play episode step (episode_generators.py:112-155) with the
    reference's MCTS (planning/mcts_zero/mcts.py) on stubbed inference queues.  The -m gpu test tests/test_hip_call_trace.py replays the
    events against this repo's classes and compares every result."""
    import json
    import random

    from planning import mcts_mission as ref_mm
    import planning.mcts_zero.mcts as ref_mcts
    import planning.common.optimization as ref_opt
    from planning.common.features import EpisodeHistory

    out = {}
    uav = {"max_v": 2, "max_a": 2}
    dim = 10
    # ---------------------------------------------------------------- (i) classic planner
    rec = _Recorder()
    seed = 21
    params = load_params(dim, dim)
    gm, sensor, sim, mapping = build(params, seed=seed)
    pm = _Proxy(mapping, "mapping", rec)
    restore = [(m, n, _record_fn(rec, m, n)) for m, n in ((ref_mm, "compute_reward"), (ref_mm, "compute_adaptive_msk"), (ref_mm, "action_costs"))]
    mis = ref_mm.MCTSMission(pm, uav, dist_to_boundaries=10, min_altitude=8, max_altitude=14, budget=40.0, altitude_spacing=6,
                             num_simulations=6, gamma=0.95, c=2.0, episode_horizon=2, k=4.0, alpha=0.75, epsilon_expand=0.2,
                             epsilon_rollout=0.5, max_greedy_radius=5.0, use_gcb_rollout=False, adaptive=True, value_threshold=0.4, interval_factor=0)
    rec.on = True
    mis.eval(run_time=0, flight_time=0)
    previous_waypoint = mis.init_action
    remaining_budget = mis.budget
    for step in range(2):  # two rounds of the mission loop (mcts_mission.py:396-414): the second replans from an updated map
        root = ref_mm.Node(state=pm.grid_map.cov_matrix, parent=None, action=previous_waypoint)
        assert remaining_budget >= pm.grid_map.resolution
        random.seed(70 + step)
        merged_root = mis.run_simulations_proxy(root, remaining_budget, mis.episode_horizon, mis.num_simulations, 0)
        waypoint = ref_mm.MCTSMission.select_best_child(merged_root).action
        remaining_budget -= ref_mm.action_costs(waypoint, previous_waypoint, mis.uav_specifications)
        simulated_raw_measurement = pm.sensor.take_measurement(waypoint)
        pm.update_grid_map(waypoint, simulated_raw_measurement)
        previous_waypoint = waypoint
        mis.eval(run_time=0.0, flight_time=0.0)
    rec.on = False
    for m, n, fn in restore:
        setattr(m, n, fn)
    out["mission_trace"] = np.frombuffer(json.dumps(rec.events).encode(), dtype=np.uint8)
    rec.save_into(out, "mission")
    out["mission_seed"] = seed
    out["mission_metrics"] = np.array([mis.root_mean_squared_errors, mis.weighted_root_mean_squared_errors, mis.mean_log_losses,
                                       mis.weighted_mean_log_losses, mis.map_uncertainties, mis.map_uncertainty_differences], dtype=np.float64)
    print(f"  call trace (mcts_mission): {len(rec.events)} events, {len(rec.arrays)} arrays")

    # ---------------------------------------------------------------- (ii) self-play episode steps
    rec = _Recorder()
    seed = 33
    params = load_params(dim, dim)
    gm, sensor, sim, mapping = build(params, seed=seed)
    pm = _Proxy(mapping, "mapping", rec)
    restore = [(m, n, _record_fn(rec, m, n)) for m, n in ((ref_opt, "compute_reward"), (ref_opt, "compute_adaptive_msk"))]
    hyper = dict(params["experiment"]["missions"][0]["hyper_params"])
    hyper.update(num_mcts_simulations=12, non_blocking_read=False)
    budget = 40.0
    scenario = {"value_threshold": 0.4, "interval_factor": 0}
    meta = {"budget": budget, "initial_budget": budget, "episode_horizon": 3, "min_altitude": 8, "max_altitude": 14, "altitude_spacing": 6,
            "uav_specifications": uav, "scenario_info": scenario}
    num_actions = dim * dim * 2
    queues = _StubQueues(num_actions)
    np.set_printoptions(threshold=sys.maxsize)  # (the node key hash(str(P)) sees the whole matrix: gen_mcts)
    keep_planes = ref_mcts.generate_input_feature_planes
    ref_mcts.generate_input_feature_planes = lambda *a, **k: None  # (stubbed network; features.py:98-99 would zero live states in place)
    mcts = ref_mcts.MCTS(pm, hyper, meta, queues, queues)
    actions_np = mcts.actions_np
    rec.on = True

    def get_adaptive_info():
        return {"mean": pm.grid_map.mean, "value_threshold": 0.4, "interval_factor": 0}

    node = ref_mcts.Node(pm.grid_map.cov_matrix)
    previous_action = np.array([2.0, 2.0, 14.0])
    history = EpisodeHistory(hyper["input_history_length"])
    remaining_budget = budget
    np.random.seed(5000 + seed)
    chosen = []
    for depth in range(2):  # two steps of the loop episode_generators.py:112-155
        assert remaining_budget >= pm.grid_map.resolution
        history.push(node.state, previous_action, remaining_budget / budget)
        policy, valid = mcts.get_policy(node, 0, previous_action, remaining_budget, history, temperature=1)
        action_idx = np.random.choice(len(policy), p=policy)
        action = actions_np[action_idx, :]
        reward, _, next_state = ref_opt.simulate_prediction_step(node.state, previous_action, action, pm, uav, get_adaptive_info())
        rec.add("call", "fn", "simulate_prediction_step", [node.state, previous_action, action, uav, get_adaptive_info()], None, (reward, next_state))
        simulated_raw_measurement = pm.sensor.take_measurement(action, verbose=False)
        pm.update_grid_map(action, simulated_raw_measurement)
        remaining_budget -= ref_actions.action_costs(action, previous_action, uav)
        node = ref_mcts.Node(next_state)
        previous_action = action
        chosen.append(action_idx)
    rec.on = False
    np.set_printoptions(threshold=1000)
    ref_mcts.generate_input_feature_planes = keep_planes
    for m, n, fn in restore:
        setattr(m, n, fn)
    out["selfplay_trace"] = np.frombuffer(json.dumps(rec.events).encode(), dtype=np.uint8)
    rec.save_into(out, "selfplay")
    out["selfplay_seed"] = seed
    out["selfplay_chosen"] = np.array(chosen)
    print(f"  call trace (self-play): {len(rec.events)} events, {len(rec.arrays)} arrays")
    save("call_trace", **out)



def main():
    os.makedirs(OUT, exist_ok=True)
    print("writing golden vectors to", OUT)
    only = sys.argv[1:]
    if only:  # e.g. `python tests/golden/gen_golden.py features`: regenerate the named fixtures only
        for name in only:
            globals()["gen_" + name]()
        return
    gen_footprints()
    gen_measurement_model()
    gen_priors()
    gen_predict()
    gen_episodes()
    gen_grf()
    gen_fallback()
    gen_greedy()
    gen_costs()
    gen_features()
    gen_mcts()
    gen_mcts_decayed()
    gen_mcts_mission()
    gen_call_trace()
    shapes = sorted(set(RESIZE_CALLS))
    print("cv2.resize stub was called with (src shape, dsize):", shapes)


if __name__ == "__main__":
    main()
