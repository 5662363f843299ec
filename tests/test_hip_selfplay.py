"""
GPU tests of the batched self-play (planning/mcts_zero/selfplay.py; ipp_selfplay_record / _commit, ipp_replay_gather in csrc/k_selfplay.h):
  * every step, against host restatements: the device read-out equals the host read-out of the same trees (DeviceMCTS._policies_rows,
    VectorMCTS's arithmetic) to 1e-12, on a 40x40 split field (3200 actions: a read-out that ran on the host before) and a 50x50 GRF;
    the action is the inverse CDF of the policy at the env's Philox uniform (one-hot arg-max at temperature 0); the ring row holds the
    fp32 policy, the valid set and the pre-step planes bit for bit; the value targets of every ended episode equal value_targets to
    1e-12; the next episode starts at the drawn waypoint;
  * minibatches: rows, offsets, shifted planes, dense policies and masks equal the host restatement exactly; wrap-around of a ring just
    above its minimum never returns a pending or overwritten row, and the draws are uniform over the committed rows;
  * the episode end of a root without a policy (ok == 0) at kernel level; two shards = one process; VecIPPEnv defaults unchanged.
"""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

UAV = {"max_v": 2.0, "max_a": 2.0}


def host(t):
    return t.detach().cpu().numpy()


def _params(**over):
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=24, temperature_scale=1.0, temperature_threshold=3, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=40.0, max_episode_steps=6, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications=UAV, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    for k, v in over.items():
        (md if k in md else hp)[k] = v
    return hp, md


class _Shared:
    """The shared generator of the host read-out, drawing the device's tie uniforms."""

    def __init__(self, u):
        self.u = u

    def random_sample(self, n):
        return self.u[:n].copy()


class Tracker:
    """Host bookkeeping of the rows of every env's running episode, checked against the device after each step."""

    def __init__(self, sp):
        self.sp, self.B = sp, sp.num_envs
        self.rows = {e: [] for e in range(self.B)}
        self.rew = {e: [] for e in range(self.B)}
        self.ended_episodes = 0
        self.forced = 0

    def step(self, check_readout=True, check_planes=True):
        import torch

        from ipp_rl_amd.planning.mcts_zero.selfplay import (ACTION_STREAM, ARGMAX_STREAM, init_action_index, inverse_cdf, step_uniform,
                                                            value_targets)

        sp, env, r, B = self.sp, self.sp.env, self.sp.replay, self.B
        gid = np.arange(B) + env.env_id_offset
        ep0, d0, tie = host(env.episode).copy(), host(env.depth).copy(), host(sp.tie_u).copy()
        want_planes = host(env.feature_planes(sp.spec)) if (check_planes and r.channels) else None
        t = sp.t
        slot = t % sp.slots
        sp.step()
        torch.cuda.synchronize()
        pol_t, pol_1 = host(sp.last["policy_t"]), host(sp.last["policy_1"])
        vidx, ok = host(sp.last["valid_idx"]), host(sp.last["ok"])
        if check_readout:
            m = sp.mcts
            m._shared_rng = _Shared(tie)
            for T, pol in ((float(sp.hp["temperature_scale"]), pol_t), (1.0, pol_1)):
                rows = m._policies_rows(B, T, False, None)
                for e in range(B):
                    if rows[e] is None:
                        assert not ok[e]
                        continue
                    assert ok[e]
                    dense = np.zeros(m.num_actions)
                    dense[list(rows[e][0].keys())] = list(rows[e][0].values())
                    K = int((vidx[e] >= 0).sum())
                    np.testing.assert_allclose(pol[e, :K], dense[vidx[e, :K]], rtol=0, atol=1e-12)
                    assert abs(pol[e, :K].sum() - 1.0) < 1e-12 and np.all(pol[e, K:] == 0)
        act_idx, rew = host(sp.action_idx), host(env.reward).astype(np.float64)
        done, ev = host(env.done), host(sp.episode_values)
        prev_after, ep1 = host(env.prev), host(env.episode)
        rp, ri, rf = host(r.policy), host(r.idx), host(r.flags)
        rv = host(r.value)
        for e in range(B):
            row = slot * B + e
            if not ok[e]:
                self.forced += 1
                assert act_idx[e] == -1 and rf[row] == 0
            else:
                K = int((vidx[e] >= 0).sum())
                t0 = d0[e] >= int(sp.hp["temperature_threshold"])
                p = pol_1[e, :K] if t0 else pol_t[e, :K]
                if t0:
                    ties = np.nonzero(p == p.max())[0]
                    u = step_uniform(ARGMAX_STREAM, sp.seed, gid[e], ep0[e], d0[e])
                    best = ties[min(int(u * len(ties)), len(ties) - 1)]
                    p = np.zeros(K)
                    p[best] = 1.0
                k = inverse_cdf(p, step_uniform(ACTION_STREAM, sp.seed, gid[e], ep0[e], d0[e]))
                assert act_idx[e] == vidx[e, k]
                assert np.array_equal(rp[row, :K], p.astype(np.float32)) and np.array_equal(ri[row], vidx[e])
                if want_planes is not None:
                    assert np.array_equal(np.nan_to_num(host(r.planes[row]), nan=-7), np.nan_to_num(want_planes[e], nan=-7))
                self.rows[e].append(row)
                self.rew[e].append(rew[e])
            ended = (not ok[e]) or bool(done[e])
            assert np.isnan(ev[e]) != ended
            if ended:
                vals, tot = value_targets(self.rew[e], float(sp.hp["gamma"]), int(sp.md["episode_horizon"]))
                np.testing.assert_allclose(rv[self.rows[e]], vals, rtol=0, atol=1e-12)
                assert np.all(rf[self.rows[e]] == 2)
                np.testing.assert_allclose(ev[e], tot, rtol=0, atol=1e-12)
                if sp.random_init:
                    a0 = init_action_index(sp.seed, gid[e], ep1[e], sp.num_actions)
                    assert np.array_equal(prev_after[e], host(sp.actions[int(a0)]))
                self.rows[e], self.rew[e] = [], []
                self.ended_episodes += 1
            else:
                assert np.all(rf[self.rows[e]] == 1)  # (the running episode's rows: pending)

    def pending(self):
        return {row for rows in self.rows.values() for row in rows}


def _check_sample(sp, batch, k):
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import replay_draws, shift_planes

    r = sp.replay
    committed = np.nonzero(host(r.flags) == 2)[0]
    draw = r.draws
    states, pol, val, rew, msk, idx, w = r.sample(batch, num_augmented_samples=k)
    torch.cuda.synchronize()
    n = max(1, batch // (k + 1))
    rows, offs = replay_draws(n, k + 1, r.seed, draw, committed)
    assert np.array_equal(host(idx), np.tile(rows, k + 1)) and np.array_equal(host(r.last_offsets), offs)
    assert np.array_equal(host(val), np.tile(host(r.value)[rows], k + 1)) and np.array_equal(host(rew), np.tile(host(r.reward)[rows], k + 1))
    A = sp.num_actions
    dense_p, dense_m = np.zeros((n, A), np.float32), np.zeros((n, A), np.uint8)
    ri, rp = host(r.idx)[rows], host(r.policy)[rows]
    for q in range(n):
        ok = ri[q] >= 0
        dense_p[q, ri[q][ok]] = rp[q][ok]
        dense_m[q, ri[q][ok]] = 1
    assert np.array_equal(host(pol), np.tile(dense_p, (k + 1, 1))) and np.array_equal(host(msk), np.tile(dense_m, (k + 1, 1)))
    assert np.all(host(w) == 1.0) and len(w) == n * (k + 1)
    if states is not None:
        src = host(r.planes[torch.as_tensor(rows, device=r.planes.device)])
        got = host(states)
        for c in range(k + 1):
            assert np.array_equal(np.nan_to_num(got[c * n:(c + 1) * n], nan=-7), np.nan_to_num(shift_planes(src, offs[c]), nan=-7))
    return host(idx)


def _selfplay(cfg, B, planes, **kw):
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    over = {k: kw.pop(k) for k in list(kw) if k in ("temperature_threshold", "temperature_scale", "max_episode_steps", "initial_budget",
                                                   "gamma", "num_mcts_simulations", "input_history_length")}
    hp, md = _params(**over)
    return SelfPlay(cfg, B, hp, md, planes=planes, **kw)


@pytest.mark.parametrize("grid", ["split40", "grf50"])
def test_selfplay_steps_match_host_restatements(grid):
    from ipp_rl_amd import EngineConfig

    # (the issue's 10x10 split field cannot run: budget mode needs patch-layout engines, square grids from 40x40; a 40x40 split field
    # has 3200 <= DENSE_ACTIONS actions, so its read-out also ran on the host before)
    if grid == "split40":  # 3200 actions: the device read-out is new here; planes kept (history 1: 6 channels of 1600^2)
        cfg, B, planes = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field"), 4, True
    else:
        cfg, B, planes = EngineConfig(x_dim=50, y_dim=50), 16, False
    sp = _selfplay(cfg, B, planes, seed=5, env_id_offset=3)
    assert sp.num_actions == 2 * cfg.n_cells
    tr = Tracker(sp)
    for _ in range(14):
        tr.step()
    assert tr.ended_episodes >= B and tr.ended_episodes > tr.forced  # (6-step episodes: every env has committed rows)
    for k in (0, 2):
        got = _check_sample(sp, 9, k)
        assert not (set(got.tolist()) & tr.pending())
    sp.close()


def test_ring_wrap_around_and_uniform_draws():
    import torch

    from ipp_rl_amd import EngineConfig

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    B = 32
    sp = _selfplay(cfg, B, False, seed=2, max_episode_steps=4, initial_budget=200.0)  # 5 step slots: the minimum
    assert sp.slots == 5
    tr = Tracker(sp)
    for _ in range(23):
        tr.step(check_readout=False)
        if sp.t % 4 == 0:
            got = _check_sample(sp, 64, 1)
            assert not (set(got.tolist()) & tr.pending())
    # frequency test: 64 minibatches of 2048 rows over the committed rows
    committed = np.nonzero(host(sp.replay.flags) == 2)[0]
    assert len(committed) >= 2 * B  # (lock-step 4-step episodes: after 23 steps the slots of steps 18, 19 hold committed rows)
    counts = np.zeros(sp.replay.capacity)
    for _ in range(64):
        _, _, _, _, _, idx, _ = sp.replay.sample(2048)
        counts += np.bincount(host(idx), minlength=sp.replay.capacity)
    torch.cuda.synchronize()
    assert counts[np.setdiff1d(np.arange(sp.replay.capacity), committed)].sum() == 0
    c = counts[committed]
    expect = c.sum() / len(committed)
    chi2 = ((c - expect) ** 2 / expect).sum()
    dof = len(committed) - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)
    sp.close()


def test_no_policy_ends_the_episode_at_kernel_level():
    """ok == 0 rows (the reference's `policy is None: break`): no sample, the env starts its next episode in the step launch, its value
    covers the samples recorded before."""
    import ctypes as C

    import torch

    from ipp_rl_amd import EngineConfig, _ffi
    from ipp_rl_amd.planning.mcts_zero.selfplay import value_targets

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    B = 4
    sp = _selfplay(cfg, B, False, seed=8, max_episode_steps=10, initial_budget=400.0)
    tr = Tracker(sp)
    tr.step()
    tr.step()
    env, r = sp.env, sp.replay
    rewards_before = {e: list(tr.rew[e]) for e in range(B)}
    ep0, d0 = host(env.episode).copy(), host(env.depth).copy()
    out = sp.mcts.search_device(sp._roots, env.prev, env.budget, sp._temps, sp.tie_u)
    ok = out["ok"].clone()
    ok[1] = 0
    ok[3] = 0
    t = sp.t
    lib = sp._lib
    _ffi.check(lib.ipp_selfplay_record(C.byref(sp._sp), t, out["policy"][0].data_ptr(), out["policy"][0].data_ptr(), out["valid_idx"].data_ptr(),
                                       ok.data_ptr(), env.engine.stream))
    env.step(sp.action)
    _ffi.check(lib.ipp_selfplay_commit(C.byref(sp._sp), t, env.engine.stream))
    sp.t += 1
    torch.cuda.synchronize()
    ep1, d1, ev, flags = host(env.episode), host(env.depth), host(sp.episode_values), host(r.flags)
    for e in (1, 3):
        assert ep1[e] == ep0[e] + 1 and d1[e] == 0 and host(sp.ep_len)[e] == 0 and host(sp.action_idx)[e] == -1
        assert flags[(t % sp.slots) * B + e] == 0
        _, tot = value_targets(rewards_before[e], 0.9, 3)
        np.testing.assert_allclose(ev[e], tot, rtol=0, atol=1e-12)
        assert np.all(flags[tr.rows[e]] == 2)
    for e in (0, 2):
        assert np.isnan(ev[e]) and d1[e] == d0[e] + 1 and flags[(t % sp.slots) * B + e] == 1
    sp.close()


def test_two_shards_give_the_samples_of_one_process():
    import torch

    from ipp_rl_amd import EngineConfig

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    B = 8
    one = _selfplay(cfg, B, False, seed=4, temperature_threshold=2)
    two = [_selfplay(cfg, B // 2, False, seed=4, env_id_offset=o, temperature_threshold=2) for o in (0, B // 2)]
    for t in range(10):
        one.step()
        for s in two:
            s.step()
        torch.cuda.synchronize()
        assert np.array_equal(host(one.action_idx), np.concatenate([host(s.action_idx) for s in two]))
        assert np.array_equal(host(one.env.reward), np.concatenate([host(s.env.reward) for s in two]))
        assert np.array_equal(host(one.episode_values), np.concatenate([host(s.episode_values) for s in two]), equal_nan=True)
        rows_one = host(one.replay.policy).reshape(one.slots, B, -1)[t % one.slots]
        rows_two = np.concatenate([host(s.replay.policy).reshape(s.slots, B // 2, -1)[t % s.slots] for s in two])
        assert np.array_equal(rows_one, rows_two)
    for s in [one] + two:
        s.close()


def test_vec_env_defaults_build_the_same_engine():
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    a = VecIPPEnv(cfg, 16, episode_steps=6, window_rows=-1, budget=40.0)
    b = IPPEngine(cfg, capacity=16, state="factor", rank_cap=9 * 6, window_rows=-1, fixed_prior=True)
    c = VecIPPEnv(cfg, 16, episode_steps=6, window_rows=-1, budget=40.0, node_capacity=64, max_batch=64)
    fields = [f[0] for f in type(a.engine.info)._fields_]
    assert all(getattr(a.engine.info, f) == getattr(b.info, f) for f in fields)
    assert a.engine._c.node_capacity == 0 and a.engine.max_batch == 16
    assert c.engine._c.node_capacity == 64 and c.engine.max_batch == 64 and c.engine.info.arena_bytes > a.engine.info.arena_bytes
    for x in (a.engine, b, c.engine):
        x.close()


def _reference_loop_check(sims, seed):
    """Replay episode_generators.py:112-170 per env on the host with the drop-in classes (GridMap, Mapping, RGBCamera,
    simulate_prediction_step, action_costs, EpisodeHistory, generate_input_feature_planes) and the device's chosen actions.
    Non-adaptive (scenario_info None): the device draws its measurement noise from its own Philox stream, which the host stream
    cannot reproduce, and with the adaptive mask the map mean -- hence rewards and planes -- would depend on that noise."""
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.mapping.grid_maps import GridMap
    from ipp_rl_amd.mapping.mappings import Mapping
    from ipp_rl_amd.planning.common.actions import action_costs
    from ipp_rl_amd.planning.common.features import EpisodeHistory, generate_input_feature_planes
    from ipp_rl_amd.planning.common.optimization import simulate_prediction_step
    from ipp_rl_amd.planning.common.rewards import scale_value_target
    from ipp_rl_amd.planning.mcts_zero import SelfPlay
    from ipp_rl_amd.sensors.cameras import RGBCamera
    from ipp_rl_amd.sensors.models.sensor_models import AltitudeSensorModel
    from tests.params import example_params

    dim, B, TOL = 40, 3, 1e-5
    cfg = EngineConfig(x_dim=dim, y_dim=dim, simulation="split_random_field")
    hp, md = _params(num_mcts_simulations=sims, max_episode_steps=5, initial_budget=24.0)
    md["scenario_info"] = None
    sp = SelfPlay(cfg, B, hp, md, planes=True, seed=seed)
    params = example_params(dim)
    gm = GridMap(params)
    mapping = Mapping(gm, RGBCamera(params["sensor"]["field_of_view"], AltitudeSensorModel(0.05, 0.2), gm))
    prior = np.array(gm.cov_matrix, dtype=np.float64, copy=True)
    B0, res, T_max, gamma, horizon = 24.0, float(cfg.resolution), 5, float(hp["gamma"]), int(md["episode_horizon"])
    env, r = sp.env, sp.replay
    ep = [None] * B
    stats = {"normal": 0, "no_policy": 0, "planes": 0}

    def finish(e):
        x = ep[e]
        rewards = x["rewards"]
        total = sum([gamma ** j * rewards[j] for j in range(len(rewards))])  # :158
        np.testing.assert_allclose(host(sp.episode_values)[e], total, rtol=0, atol=TOL)
        hist = EpisodeHistory(int(hp["input_history_length"]))
        for i, reward in enumerate(rewards):  # :159-182
            state, action, budget, row = x["examples"][i]
            bootstrapped_idx = min(i + horizon, len(rewards))
            value = scale_value_target(sum([gamma ** j * rewards[j] for j in range(i, bootstrapped_idx)]))
            np.testing.assert_allclose(host(r.value[row]), value, rtol=0, atol=TOL)
            np.testing.assert_allclose(host(r.reward[row]), reward, rtol=0, atol=TOL)
            hist.push(state, action, budget / B0)
            if e == 0 and i < 2:  # (planes of 40 x 40 are 10 MB per channel: the first samples of env 0's episodes)
                want = generate_input_feature_planes(mapping, hist, 8.0, 14.0, adaptive_info=None, uav_specifications=UAV,
                                                     use_action_costs_input=True)
                got = host(r.planes[row]).astype(np.float64)
                assert got.shape == want.shape
                assert np.max(np.abs(got - want)) < TOL, (i, np.max(np.abs(got - want)))
                stats["planes"] += 1
        ep[e] = None

    for _ in range(16):
        prev0, bud0, dep0 = host(env.prev).copy(), host(env.budget).copy(), host(env.depth).copy()
        for e in range(B):
            if ep[e] is None:  # a new episode: the prior, the device's drawn first waypoint, the start budget (:104-111)
                assert dep0[e] == 0
                ep[e] = dict(state=prior.copy(), prev=prev0[e].copy(), budget=B0, depth=0, rewards=[], examples=[])
            x = ep[e]
            assert x["depth"] < T_max and x["budget"] >= res  # (:112, the loop goes on)
            np.testing.assert_array_equal(x["prev"], prev0[e])
            np.testing.assert_allclose(bud0[e], x["budget"], rtol=0, atol=TOL)
        t = sp.t
        sp.step()
        torch.cuda.synchronize()
        ok, act, rew, done = host(sp.last["ok"]), host(sp.action), host(env.reward), host(env.done)
        for e in range(B):
            x = ep[e]
            if not ok[e]:  # policy is None: break (:130-131)
                stats["no_policy"] += 1
                finish(e)
                continue
            action = act[e].copy()
            x["examples"].append((x["state"], x["prev"].copy(), x["budget"], (t % sp.slots) * B + e))
            reward, _, next_state = simulate_prediction_step(x["state"], x["prev"], action, mapping, UAV, None)  # :137-144
            np.testing.assert_allclose(rew[e], reward, rtol=0, atol=TOL)
            x["budget"] -= action_costs(action, x["prev"], UAV)  # :148
            x["prev"], x["state"] = action, next_state
            x["rewards"].append(reward)
            x["depth"] += 1
            ended = not (x["depth"] < T_max and x["budget"] >= res)
            assert bool(done[e]) == ended, (e, x["depth"], x["budget"])
            if ended:
                stats["normal"] += 1
                finish(e)
    sp.close()
    return stats


def test_reference_loop_on_the_host_with_the_drop_in_classes():
    """The loop of episode_generators.py:112-170 replayed on the host (drop-in classes, the device's actions) gives the device's
    rewards, budgets, episode ends and lengths, values and total episode values within 1e-5, and the drop-in
    generate_input_feature_planes gives the ring's planes.  Two search sizes: 24 simulations end episodes on the budget and the step
    count, 6 simulations leave roots without a policy (every visited action has one visit, mcts.py:128-132)."""
    a = _reference_loop_check(24, 3)
    b = _reference_loop_check(6, 4)
    assert a["normal"] + b["normal"] > 0 and a["no_policy"] + b["no_policy"] > 0 and a["planes"] + b["planes"] > 0, (a, b)
