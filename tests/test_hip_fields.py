"""
GPU tests of the hotspot and split ground truths (csrc/k_fields.h; ipp_fill_fields, ipp_generate_field_groups / _refill; VecIPPEnv with
cfg.simulation; the drop-in HotspotRandomField / SplitRandomField) against the reference's maps (tests/golden/fields.npz) and the
host copy of the device draws (ipp_rl_amd.fields).
"""
import os

import numpy as np
import pytest

from tests.params import example_params

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fields.npz")
INIT = np.array([2.0, 2.0, 14.0])
UAV = {"max_v": 2, "max_a": 2}
KIND_NAMES = {"hotspot": "hotspot_random_field", "split": "split_random_field"}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def host(t):
    return t.detach().cpu().numpy()


def fixture_records(g):
    """{dim: [(key, record, map)]} of every recorded map."""
    from ipp_rl_amd import fields

    out = {}
    for key in g.files:
        if key.endswith("_map"):
            k = key[:-len("map")]
            rec = np.zeros((), dtype=fields.RECORD_DTYPE)
            rec["inside"], rec["outside"], rec["rect"] = g[k + "inside"], g[k + "outside"], g[k + "rect"]
            out.setdefault(int(k.split("_")[1]), []).append((k, rec, g[key]))
    return out


def test_fill_fields_reproduces_reference_maps(golden):
    """Caller records into a caller buffer and into the envs' alternate planes (flipped in by a folded reset, then read back)."""
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine

    for dim, items in sorted(fixture_records(golden).items()):
        n = len(items)
        cfg = EngineConfig(x_dim=dim, y_dim=dim)
        eng = IPPEngine(cfg, capacity=n, state="factor", rank_cap=27, window_rows=-1, fixed_prior=True)
        recs = np.stack([r for _, r, _ in items])
        want = np.stack([np.float32(m) for _, _, m in items])
        out = eng.fill_fields(recs)
        torch.cuda.synchronize()
        assert np.array_equal(host(out).reshape(n, dim, dim), want), dim
        # odd-sized, unaligned destination rows: the scalar store path
        big = torch.full((n * dim * dim + 1,), -1.0, device=eng.device)
        eng.fill_fields(recs, out=big[1:].view(n, dim * dim))
        torch.cuda.synchronize()
        assert np.array_equal(host(big[1:]).reshape(n, dim, dim), want) and float(big[0]) == -1.0, dim
        # alternate planes: every env stages its record, a step with a folded reset flips to it
        eng.reset(gt=np.zeros((n, dim * dim), dtype=np.float32))
        eng.fill_fields(recs, row_ids=np.arange(n, dtype=np.int32))
        prev = torch.as_tensor(np.tile(INIT, (n, 1)), device=eng.device)
        acts = np.tile([4.0 * (dim // 2) + 2.0, 4.0 * (dim // 2) + 2.0, 8.0], (n, 1))
        _, status = eng.step(acts, prev, meas_noise=np.zeros((n, 9)), update_prev=True, reset_src=np.arange(n, dtype=np.int32),
                             reset_gt=None, init_action=INIT)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        for e, (key, _, m) in enumerate(items):
            assert np.array_equal(host(eng.read_gt(e)).reshape(dim, dim), np.float32(m)), key
            assert np.all(np.isfinite(host(eng.read_diag(e))))  # (the flip found a staged plane: no poisoned env)
        eng.close()


@pytest.mark.parametrize("dim", [40, 50, 100])
def test_device_draws_equal_host_copy(dim):
    """4096 fields x 3 episodes x both kinds, straight from Philox on the device, bit for bit against fields.draw_records + fill."""
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine, _ffi, fields

    cfg = EngineConfig(x_dim=dim, y_dim=dim, cluster_radius=5.0)
    B, seed, off, gt_stream = 4096, 77, 1000, 1 << 40
    eng = IPPEngine(cfg, capacity=8, state="factor", rank_cap=9, max_batch=B, window_rows=-1, fixed_prior=True)
    out = torch.empty((B, dim * dim), dtype=torch.float32, device=eng.device)
    for kind in (_ffi.IPP_FIELD_HOTSPOT, _ffi.IPP_FIELD_SPLIT):
        for ep in range(3):
            out.fill_(-1.0)
            assert eng.generate_fields_rows(kind, B, seed, gt_stream + ep, out, row_offset=off)
            torch.cuda.synchronize()
            rec = fields.draw_records(kind, dim, dim, 5.0, np.arange(B) + off, gt_stream + ep, seed)
            want = np.float32(fields.fill(rec, dim, dim)).reshape(B, -1)
            assert np.array_equal(host(out), want), (kind, ep)
    # GRF keeps its own grids: kind 0 forwards to the GRF generator (False where it cannot draw its own noise)
    assert eng.generate_fields_rows(_ffi.IPP_FIELD_GRF, 4, seed, gt_stream, out[:4]) == (dim in (50, 100))
    eng.close()


def test_device_field_invariants():
    """32768 device fields per kind on 50x50: two values in the reference's ranges; hotspot clusters inside the bounds formula and
    more than r apart on both axes; split index within its bounds; swap / axis frequencies within 5 sigma of 1/2."""
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine, _ffi, fields

    dim, r, B = 50, 5.0, 4096
    cfg = EngineConfig(x_dim=dim, y_dim=dim, cluster_radius=r)
    eng = IPPEngine(cfg, capacity=8, state="factor", rank_cap=9, max_batch=B, window_rows=-1, fixed_prior=True)
    out = torch.empty((B, dim * dim), dtype=torch.float32, device=eng.device)
    yy = torch.arange(dim, device=eng.device).view(1, dim, 1)
    xx = torch.arange(dim, device=eng.device).view(1, 1, dim)
    swaps = ysplits = total = 0
    for kind in (_ffi.IPP_FIELD_HOTSPOT, _ffi.IPP_FIELD_SPLIT):
        for launch in range(8):
            rows = np.arange(B) + launch * B
            assert eng.generate_fields_rows(kind, B, 3, 11, out, row_offset=launch * B)
            f = out.view(B, dim, dim)
            lo, hi = f.amin(dim=(1, 2)), f.amax(dim=(1, 2))
            assert bool(((f == lo.view(B, 1, 1)) | (f == hi.view(B, 1, 1))).all())
            rec = fields.draw_records(kind, dim, dim, r, rows, 11, 3)
            if kind == _ffi.IPP_FIELD_HOTSPOT:
                assert bool(((hi >= 0.7) & (hi <= 1.0) & (lo >= 0.0) & (lo <= 0.3)).all())
                R = rec["rect"].astype(np.int64)
                # bounds formula: a cluster is int(max(c - r, 0)) .. int(min(c + r, dim)) for an integer centre c in [trunc(r), dim)
                for q in range(2):
                    for a in (0, 2):
                        b0, b1 = R[:, q, a], R[:, q, a + 1]
                        ok = np.zeros(B, dtype=bool)
                        for c in range(int(r), dim):
                            ok |= (b0 == int(max(c - r, 0))) & (b1 == int(min(c + r, dim)))
                        assert ok.all()
                # centres (the midpoints of interior bounds; edge clusters give their bounds only) more than r apart: no cluster
                # overlap along an axis can come from centres closer than r
                for a in (0, 2):
                    c1 = np.where(R[:, 0, a] > 0, R[:, 0, a] + r, R[:, 0, a + 1] - r)
                    c2 = np.where(R[:, 1, a] > 0, R[:, 1, a] + r, R[:, 1, a + 1] - r)
                    assert np.all(np.abs(c1 - c2) > r)
                Rt = torch.as_tensor(R, device=eng.device)
                inside = torch.zeros((B, dim, dim), dtype=torch.bool, device=eng.device)
                for q in range(2):
                    inside |= ((yy >= Rt[:, q, 0].view(B, 1, 1)) & (yy < Rt[:, q, 1].view(B, 1, 1)) &
                               (xx >= Rt[:, q, 2].view(B, 1, 1)) & (xx < Rt[:, q, 3].view(B, 1, 1)))
                assert bool((f == torch.where(inside, hi.view(B, 1, 1), lo.view(B, 1, 1))).all())
            else:
                first = f[:, 0, 0]
                second = torch.where(first == lo, hi, lo)
                assert bool(((hi >= 0.65) & (hi <= 1.0) & (lo >= 0.0) & (lo <= 0.35)).all())
                ysplit = (f == f[:, :, :1]).all(dim=2).all(dim=1)
                s = torch.where(ysplit, (f[:, :, 0] == first.view(B, 1)).sum(dim=1), (f[:, 0, :] == first.view(B, 1)).sum(dim=1))
                sy_ok = (s >= int(np.ceil(dim * 0.33))) & (s <= int(np.ceil(dim * 0.66)))
                sx_ok = (s >= int(np.floor(dim * 0.33))) & (s <= int(np.ceil(dim * 0.66)))
                assert bool(torch.where(ysplit, sy_ok, sx_ok).all())
                assert bool((f[:, -1, -1] == second).all())
                swaps += int((first == lo).sum())
                ysplits += int(ysplit.sum())
                total += B
    for count in (swaps, ysplits):
        assert abs(count - total / 2) <= 5 * np.sqrt(total / 4), (count, total)
    eng.close()


def test_staggered_parts_follow_the_host_copy():
    """VecIPPEnv(stagger=True, parts=2) with hotspot fields on configs[1]'s shape: every scheduled reset installs the host copy's field
    for the env's global id and episode; rewards and diagonals equal the single launch's and those of a run that installs the same
    fields through reset(gt=...), bit for bit."""
    import torch
    from ipp_rl_amd import EngineConfig, fields
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions

    cfg = EngineConfig(x_dim=50, y_dim=50, simulation="hotspot_random_field", cluster_radius=5.0)
    B, T, seed, steps = 4096, 40, 31, 50
    two = VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=seed, parts=2)
    one = VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=seed, parts=1)
    man = VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=seed, parts=1)
    assert two.parts == 2
    gs = VecIPPEnv.GT_STREAM

    def host_fields(ids, episode):
        rec = fields.draw_records(fields.field_kind(cfg.simulation), 50, 50, 5.0, np.asarray(ids), gs + np.asarray(episode), seed)
        return np.float32(fields.fill(rec, 50, 50)).reshape(len(ids), -1)

    for env in (two, one, man):
        env.reset()
    torch.cuda.synchronize()
    for e in (0, 1, 2047, 4095):
        assert np.array_equal(host(two.ground_truth(e)).reshape(-1), host_fields([e], [0])[0])
    sample = [0, 5, 1234, 4095]
    checked = 0
    for t in range(steps):
        a = torch.as_tensor(cell_centre_actions(cfg, t, 0, B, B, [float(x) for x in range(5, 15)]), device=two.device)
        r2, _ = two.step(a)
        r1, _ = one.step(a)
        rm, _ = man.step(a, auto_reset=False)
        p = man._phase_ending_at(t)
        ids = man._reset_ids_host[p]
        if len(ids):
            man.reset(env_ids=ids, gt=host_fields(ids, man.episode[ids]))
        torch.cuda.synchronize()
        assert torch.equal(r2, r1) and torch.equal(r2, rm), t
        assert np.array_equal(two.episode, man.episode) and np.array_equal(one.episode, man.episode), t
        for e in list(ids[:3]) + sample:
            e = int(e)
            want = host_fields([e], [two.episode[e] - 1])[0]
            assert np.array_equal(host(two.ground_truth(e)).reshape(-1), want), (t, e)
            assert torch.equal(two.diag(e), one.diag(e)) and torch.equal(two.diag(e), man.diag(e)), (t, e)
            checked += 1
    assert two.alt_blocks > 0 and checked > 100
    for env in (two, one, man):
        env.close()


@pytest.mark.parametrize("flip,T", [("0", 6), ("1", 1)])
def test_staged_buffers_follow_the_host_copy(monkeypatch, flip, T):
    """The other staging mode -- fields into staged buffers, copied in by the resets (IPP_GT_FLIP=0, or one-step episodes where
    2 K > episode_steps) -- with split fields on a 40x40 grid: every env's field is the host copy's for its global id and episode."""
    import torch
    from ipp_rl_amd import EngineConfig, fields
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions

    monkeypatch.setenv("IPP_GT_FLIP", flip)
    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    B, seed, off = 256, 23, 5
    env = VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=seed, env_id_offset=off)
    env.reset()
    for t in range(2 * T + 3):
        a = torch.as_tensor(cell_centre_actions(cfg, t, 0, B, B, [8.0, 14.0]), device=env.device)
        _, status = env.step(a)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        for e in (0, 1, 100, 255):
            rec = fields.draw_records(fields.field_kind(cfg.simulation), 40, 40, cfg.cluster_radius, [e + off],
                                      VecIPPEnv.GT_STREAM + int(env.episode[e]) - 1, seed)
            assert np.array_equal(host(env.ground_truth(e)).reshape(-1), np.float32(fields.fill(rec, 40, 40)).reshape(-1)), (t, e)
    assert env.alt_blocks == 0 and env.episode.min() >= 2
    env.close()


@pytest.mark.parametrize("parts", [1, 2])
def test_budget_mode_split_fields_on_40x40(parts):
    """Budget mode with split fields on a 40x40 grid (patch layout, no self-drawing GRF: GRF budget mode raises there): envs end at
    different steps, and each env's field equals the host copy for the episode the ledger reports."""
    import torch
    from ipp_rl_amd import EngineConfig, fields
    from ipp_rl_amd.vec_env import VecIPPEnv

    with pytest.raises(ValueError):
        VecIPPEnv(EngineConfig(x_dim=40, y_dim=40), 8, episode_steps=4, window_rows=-1, budget=100.0)
    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    B, T, seed, off = 2048, 40, 17, 96
    env = VecIPPEnv(cfg, B, episode_steps=T, window_rows=-1, seed=seed, budget=150.0, shuffle_budget=True, parts=parts, env_id_offset=off)
    assert int(env.engine.info.patch_layout) == 1 and env.parts == parts
    env.reset()
    rs = np.random.RandomState(4)
    depths, twice, checked = set(), 0, 0
    for t in range(16):
        a = np.stack([4.0 * rs.randint(0, 40, B) + 2.0, 4.0 * rs.randint(0, 40, B) + 2.0, rs.choice([8.0, 14.0], B)], axis=1)
        dep_before = host(env.depth).astype(np.int64)
        _, status = env.step(torch.as_tensor(a, device=env.device))
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        done = host(env.done).astype(bool)
        ep = host(env.episode)
        depths.update(int(x) for x in (dep_before + 1)[done])
        ids = np.nonzero(done)[0][:6]
        for e in ids:
            rec = fields.draw_records(fields.field_kind(cfg.simulation), 40, 40, cfg.cluster_radius, [int(e) + off],
                                      VecIPPEnv.GT_STREAM + int(ep[e]), seed)
            want = np.float32(fields.fill(rec, 40, 40)).reshape(-1)
            assert np.array_equal(host(env.ground_truth(int(e))).reshape(-1), want), (t, e, ep[e])
            twice += int(ep[e] >= 2)  # (episode 2 and later: fields staged by the refill generator behind a budget step)
            checked += 1
        if len(ids):
            assert np.all(np.isfinite(host(env.diag(int(ids[0])))))
    assert len(depths) >= 3 and twice >= 5 and checked >= 30, (depths, twice, checked)
    env.close()


@pytest.mark.parametrize("prefix", ["hotspot", "split"])
def test_drop_in_classes_match_reference(golden, prefix):
    """np.random.seed(s) -> the project's HotspotRandomField / SplitRandomField: the reference's map (fp32) and the next draw of the
    stream; the recorded episode through Mapping + the drop-in: z, rewards, final mean and diagonal within 1e-5."""
    from ipp_rl_amd.mapping.grid_maps import GridMap
    from ipp_rl_amd.mapping.mappings import Mapping
    from ipp_rl_amd.planning.common.optimization import simulate_prediction_step
    from ipp_rl_amd.sensors.cameras import RGBCamera
    from ipp_rl_amd.sensors.models.sensor_models import AltitudeSensorModel
    from ipp_rl_amd.simulations import simulations as sims

    cls = sims.HotspotRandomField if prefix == "hotspot" else sims.SplitRandomField

    def build(dim, r, seed):
        params = example_params(dim)
        params["sensor"]["simulation"] = {"type": KIND_NAMES[prefix], "cluster_radius": r}
        np.random.seed(seed)
        gm = GridMap(params)
        sensor = RGBCamera(params["sensor"]["field_of_view"], AltitudeSensorModel(0.05, 0.2), gm)
        sim = cls(sensor, r)
        sensor.set_sensor_simulation(sim)
        return gm, sensor, sim, params

    for key in golden.files:
        if key.startswith(prefix + "_") and key.endswith("_map") and "_episode_" not in key:
            _, dim, rt, st = key[:-len("_map")].split("_")
            r = float(rt[1:].replace("p", "."))
            r = int(r) if r == int(r) else r
            gm, sensor, sim, _ = build(int(dim), r, int(st[1:]))
            assert np.random.random() == float(golden[key[:-3] + "next"]), key
            assert np.array_equal(sim.ground_truth_map, np.float32(golden[key]).astype(np.float64)), key
    g = {k[len(prefix) + len("_episode_"):]: golden[k] for k in golden.files if k.startswith(prefix + "_episode_")}
    gm, sensor, sim, params = build(20, int(g["radius"]), int(g["seed"]))
    assert np.array_equal(sim.ground_truth_map, np.float32(g["gt"]).astype(np.float64))
    mapping = Mapping(gm, sensor)
    prev = INIT.copy()
    for t, a in enumerate(g["actions"]):
        info = {"mean": gm.mean, "value_threshold": 0.4, "interval_factor": 0}
        reward, _, _ = simulate_prediction_step(gm.cov_matrix, prev, a, mapping, UAV, info)
        z = sensor.take_measurement(a, verbose=False)
        m = int(g["m"][t])
        assert z.size == m and np.max(np.abs(z.ravel() - g["z"][t][:m])) < 1e-5, t
        mapping.update_grid_map(a, z)
        assert abs(reward - g["reward"][t]) < 1e-5, t
        prev = a
    assert np.max(np.abs(gm.mean - g["mean"])) < 1e-5
    assert np.max(np.abs(np.diag(gm.cov_matrix) - g["diag"])) < 1e-5
