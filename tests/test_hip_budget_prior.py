"""
GPU tests of budget mode's per-episode priors (ipp_set_budget_prior, ipp_read_prior; VecIPPEnv(budget=B0, shuffle_prior_cov="device"),
SelfPlay / Learner(episode_priors="device")): the reference's shuffle_prior_cov (mapping/mappings.py:238-240, one draw per episode where
planning/mcts_zero/episode_generators.py:53 builds the episode's Mapping), drawn by the reset inside the budget step.
  1. draws and ledger: every env's prior equals the host restatement (vec_env.start_prior) of its running episode bit for bit, through
     resets at many depths; a reset env's variance plane is float32(sigma^2);
  2. rewards, variance planes and candidate scores against the fp64 factor oracle restarted at start_prior of each episode (1e-5);
  3. parts = 2 against parts = 1, 4. two shards against one process: bit identity;
  5. the ABI's refusals, the 12-row window, ipp_set_budget_prior(0) = never called;
  6. the compact replay ring archives the prior of the episode that ENDED: minibatches equal the dense ring's, the archive slots'
     priors are start_prior of their rows' episodes, a drawn row's planes match the fp64 restatement at that prior;
  7. the learn loop resumes into the episodes' own priors.
Shapes: the smallest grid budget mode accepts (40x40 split field), one oracle case on 50x50 GRF; window_rows = -1 everywhere.
"""
import shutil

import numpy as np
import pytest

from oracle import ipp_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = 1e-5  # rewards / diagonals against fp64: the project's parity bar (tests/test_hip_budget.py)
INIT = np.array([2.0, 2.0, 14.0])
ALTS = np.array([8.0, 14.0])
UAV = {"max_v": 2.0, "max_a": 2.0}


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cfg40():
    from ipp_rl_amd import EngineConfig

    return EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")


def flight_cost(a, p, vmax=2.0, amax=2.0):
    """actions.py:32-41 in fp64, vectorised over rows."""
    d = np.sqrt(np.sum((a - p) ** 2, axis=-1))
    d_acc = np.minimum(0.5 * d, vmax * vmax / (2 * amax))
    return (d - 2 * d_acc) / vmax + 2 * np.sqrt(2 * d_acc / amax)


class NumpyLedger:
    """The budget step's bookkeeping on the host (tests/test_hip_budget.py): budget, depth, episode and waypoint of every env."""

    def __init__(self, B, T, B0, shuffle, seed, res, offset=0, depth0=None):
        from ipp_rl_amd.vec_env import start_budget

        self.B, self.T, self.B0, self.shuffle, self.seed, self.res = B, T, B0, shuffle, seed, res
        self.gid = np.arange(B, dtype=np.int64) + offset
        self.ep = np.zeros(B, dtype=np.int64)
        self.bud = start_budget(B0, shuffle, seed, self.gid, self.ep)
        self.dep = np.zeros(B, dtype=np.int64) if depth0 is None else np.asarray(depth0, dtype=np.int64).copy()
        self.prev = np.tile(INIT, (B, 1))

    def near_threshold(self, a, margin):
        return np.abs(self.bud - flight_cost(a, self.prev) - self.res) < margin

    def step(self, a):
        """Returns (done, depth at which the ended episodes ended)."""
        from ipp_rl_amd.vec_env import start_budget

        nb, nd = self.bud - flight_cost(a, self.prev), self.dep + 1
        done = ~((nd < self.T) & (nb >= self.res))
        self.ep = np.where(done, self.ep + 1, self.ep)
        self.bud = np.where(done, start_budget(self.B0, self.shuffle, self.seed, self.gid, self.ep), nb)
        self.dep = np.where(done, 0, nd)
        self.prev = np.where(done[:, None], INIT[None], a)
        return done, nd[done]


def random_actions(rs, led, dim, res):
    """Uniform cell-centre actions, redrawn while a ledger sits within 1e-6 B0 of the threshold (rounding cannot flip a done flag)."""
    B = led.B
    a = np.stack([res * rs.randint(0, dim, B) + 0.5 * res, res * rs.randint(0, dim, B) + 0.5 * res, ALTS[rs.randint(0, 2, B)]], axis=1)
    for _ in range(20):
        near = led.near_threshold(a, 1e-6 * led.B0)
        if not near.any():
            break
        a[near, 0] = res * rs.randint(0, dim, int(near.sum())) + 0.5 * res
    assert not led.near_threshold(a, 1e-6 * led.B0).any()
    return a


# ---------------------------------------------------------------------------------------------------- 1
def test_draws_follow_the_ledger_through_resets():
    import torch
    from ipp_rl_amd.vec_env import VecIPPEnv, start_prior

    cfg = cfg40()
    B, T, B0, seed = 64, 6, 150.0, 5
    env = VecIPPEnv(cfg, B, episode_steps=T, window_rows=-1, seed=seed, budget=B0, shuffle_budget=True, shuffle_prior_cov="device")
    env.reset()
    led = NumpyLedger(B, T, B0, True, seed, cfg.resolution)
    p0 = start_prior(cfg, seed, led.gid, 0)
    assert same_bits(host(env.prior_scale), p0)
    assert len(np.unique(p0[:, 0])) == B and len(np.unique(p0[:, 1])) == B
    for e in (0, 17, 63):
        assert np.all(host(env.diag(e)) == np.float32(p0[e, 0]))
    rs = np.random.RandomState(3)
    resets, depths = 0, set()
    for t in range(12):
        a = random_actions(rs, led, cfg.x_dim, cfg.resolution)
        done, ended_at = led.step(a)
        reward, status = env.step(torch.as_tensor(a, device=env.device))
        torch.cuda.synchronize()
        assert np.array_equal(host(env.done).astype(bool), done), t
        assert np.max(np.abs(host(env.budget) - led.bud)) <= 1e-9 * B0, t
        assert np.array_equal(host(env.depth), led.dep) and np.array_equal(host(env.episode), led.ep), t
        assert np.array_equal(host(env.prev), led.prev), t
        assert int(status.abs().sum()) == 0 and bool(torch.isfinite(reward).all()), t
        want = start_prior(cfg, seed, led.gid, led.ep)
        got = host(env.prior_scale)
        assert same_bits(got, want), (t, np.nonzero((got != want).any(axis=1))[0][:5])
        for e in np.nonzero(done)[0]:
            assert np.all(host(env.diag(int(e))) == np.float32(want[e, 0])), (t, e)
            assert env.engine.rank(int(e)) == 0
        resets += int(done.sum())
        depths.update(int(d) for d in ended_at)
    assert resets >= 20 and len(depths) >= 3, (resets, depths)
    assert int(led.ep.max()) >= 2  # (an env drew the priors of three episodes)
    env.close()


# ---------------------------------------------------------------------------------------------------- 2
def short_hops(rs, led, dim, res):
    """Moves of 6 to 8 cells along x (reflected at the border) and up to 2 along y from every env's waypoint: flight times of 13 to
    19 s, so that a budget of 38 s ends an episode after two or three steps."""
    B = led.B
    cell = np.floor(led.prev[:, :2] / res).astype(np.int64)
    for _ in range(50):
        dx = rs.randint(6, 9, B) * rs.choice([-1, 1], B)
        dy = rs.randint(-2, 3, B)
        x, y = cell[:, 0] + dx, cell[:, 1] + dy
        x = np.where((x < 0) | (x >= dim), cell[:, 0] - dx, x)
        y = np.clip(y, 0, dim - 1)
        a = np.stack([res * x + 0.5 * res, res * y + 0.5 * res, ALTS[rs.randint(0, 2, B)]], axis=1)
        if not led.near_threshold(a, 1e-6 * led.B0).any():
            return a
    raise AssertionError("no actions away from the threshold")


@pytest.mark.parametrize("dim,simulation,B", [(40, "split_random_field", 4), (50, None, 2)])
def test_rewards_diagonals_and_scores_against_the_fp64_oracle(dim, simulation, B):
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv, start_prior

    cfg = EngineConfig(x_dim=dim, y_dim=dim, simulation=simulation) if simulation else EngineConfig(x_dim=dim, y_dim=dim)
    oc = orc.OracleConfig(x_dim=dim, y_dim=dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b,
                          signal_variance=cfg.signal_variance, length_scale=cfg.length_scale)
    T, B0, seed = 6, 38.0, 11
    # (adaptive=False: the reward is the whole trace reduction, a function of the covariance alone -- the mean depends on the noise plane)
    env = VecIPPEnv(cfg, B, episode_steps=T, window_rows=-1, seed=seed, budget=B0, shuffle_prior_cov="device", adaptive=False)
    assert int(env.engine.info.window_rows) == 12
    env.reset()
    led = NumpyLedger(B, T, B0, False, seed, cfg.resolution)
    fs = [orc.factor_reset(oc, tuple(p)) for p in start_prior(cfg, seed, led.gid, 0)]
    rs = np.random.RandomState(2)
    worst = dict(reward=0.0, diag=0.0, score=0.0)
    lengths = []

    def check_scores(t):
        cell = np.floor(led.prev[:, :2] / cfg.resolution).astype(np.int64)
        off = np.array([[0, 0], [2, -1], [-3, 2], [5, 4]])
        cand = np.empty((B, 4, 3))
        for k in range(4):
            c = np.clip(cell + off[k], 0, dim - 1)
            cand[:, k, :2] = cfg.resolution * c + 0.5 * cfg.resolution
            cand[:, k, 2] = ALTS[(k + t) % 2]
        got, status = env.score_actions(cand)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        for e in range(B):
            for k in range(4):
                Wc, _ = orc.factor_step(oc, fs[e], cand[e, k], commit=False)
                want = float(np.sum(Wc ** 2)) / (orc.action_cost(cand[e, k], led.prev[e], UAV) + 1.0)
                worst["score"] = max(worst["score"], abs(float(got[e, k]) - want))

    for t in range(8):
        if t in (2, 5):  # (mid-episode states and fresh ones, every env on its own prior)
            check_scores(t)
        a = short_hops(rs, led, dim, cfg.resolution)
        prev = led.prev.copy()
        done, ended_at = led.step(a)
        lengths += [int(d) for d in ended_at]
        reward, status = env.step(torch.as_tensor(a, device=env.device))
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        assert np.array_equal(host(env.done).astype(bool), done) and np.array_equal(host(env.episode), led.ep), t
        pri = start_prior(cfg, seed, led.gid, led.ep)
        assert same_bits(host(env.prior_scale), pri), t
        for e in range(B):
            Wc, _ = orc.factor_step(oc, fs[e], a[e])
            want = float(np.sum(Wc ** 2)) / (orc.action_cost(a[e], prev[e], UAV) + 1.0)
            worst["reward"] = max(worst["reward"], abs(float(reward[e]) - want))
            if done[e]:
                fs[e] = orc.factor_reset(oc, tuple(pri[e]))
            worst["diag"] = max(worst["diag"], float(np.max(np.abs(host(env.diag(e)).astype(np.float64) - fs[e].diag))))
    print(f"{dim} x {dim}: worst |device - fp64| {worst}, episode lengths {sorted(lengths)}")
    assert lengths and set(lengths) <= {2, 3} and int(led.ep.min()) >= 2, (lengths, led.ep)
    assert max(worst.values()) < TOL, worst
    env.close()


# ---------------------------------------------------------------------------------------------------- 3
def test_parts_are_bit_identical():
    import torch
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions, start_prior

    cfg = cfg40()
    B, T, seed = 64, 6, 21
    envs = [VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=seed, parts=p, budget=150.0, shuffle_budget=True,
                      shuffle_prior_cov="device") for p in (1, 2)]
    assert [e.parts for e in envs] == [1, 2]
    for e in envs:
        e.reset()
    one, two = envs
    sample = [0, 5, 6, 31, 63]
    resets = 0
    for t in range(14):
        a = torch.as_tensor(cell_centre_actions(cfg, t, 0, B, B, [8.0, 14.0]), device=one.device)
        r1, s1 = one.step(a)
        r2, s2 = two.step(a)
        torch.cuda.synchronize()
        assert torch.equal(r1, r2) and torch.equal(s1, s2) and int(s1.abs().sum()) == 0, t
        for name in ("budget", "depth", "episode", "done", "prev"):
            assert torch.equal(getattr(one, name), getattr(two, name)), (t, name)
        p1, p2 = host(one.prior_scale), host(two.prior_scale)
        assert same_bits(p1, p2), t
        assert same_bits(p1, start_prior(cfg, seed, np.arange(B), host(one.episode))), t
        assert torch.equal(one.engine.ranks(), two.engine.ranks()), t
        for e in sample:
            assert torch.equal(one.mean(e), two.mean(e)) and torch.equal(one.diag(e), two.diag(e)), (t, e)
        resets += int(one.done.sum())
    assert resets >= 20
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------- 4
def test_shards_are_bit_identical():
    import torch
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions, start_prior

    cfg = cfg40()
    B, seed = 48, 13
    kw = dict(episode_steps=6, window_rows=-1, seed=seed, budget=150.0, shuffle_budget=True, shuffle_prior_cov="device")
    one = VecIPPEnv(cfg, B, **kw)
    two = [VecIPPEnv(cfg, 24, env_id_offset=o, **kw) for o in (0, 24)]
    for e in [one] + two:
        e.reset()
    resets = 0
    for t in range(10):
        r1, _ = one.step(cell_centre_actions(cfg, t, 0, B, B, [8.0, 14.0]))
        r2 = [s.step(cell_centre_actions(cfg, t, o, o + 24, B, [8.0, 14.0]))[0] for s, o in zip(two, (0, 24))]
        torch.cuda.synchronize()
        assert torch.equal(r1, torch.cat(r2)), t
        for name in ("budget", "depth", "episode", "done"):
            assert torch.equal(getattr(one, name), torch.cat([getattr(s, name) for s in two])), (t, name)
        p1 = host(one.prior_scale)
        assert same_bits(p1, np.concatenate([host(s.prior_scale) for s in two])), t
        assert same_bits(p1, start_prior(cfg, seed, np.arange(B), host(one.episode))), t
        resets += int(one.done.sum())
    assert resets > 0
    for e in [one] + two:
        e.close()


# ---------------------------------------------------------------------------------------------------- 5
def test_abi_refusals_window_and_switching_off():
    import torch
    from ipp_rl_amd import IPPEngine
    from ipp_rl_amd._ffi import IppError
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions

    cfg = cfg40()

    def ledger(dev, n=8):
        return (torch.full((n,), 50.0, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.full((n,), 3, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                torch.full((n,), -1, dtype=torch.int32, device=dev))

    eng = IPPEngine(cfg, capacity=8, state="factor", rank_cap=64, window_rows=-1, fixed_prior=True)
    assert int(eng.info.patch_layout) == 1 and int(eng.info.window_rows) == 10
    with pytest.raises(IppError, match="no ledger"):
        eng.set_budget_prior(True)
    led = ledger(eng.device)
    before = [t.clone() for t in led]
    eng.set_budget(*led, 50.0, 4)
    with pytest.raises(IppError, match="fixed_prior"):
        eng.set_budget_prior(True)
    eng.set_budget_prior(False)  # (switching off is always possible)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(led, before))
    # ipp_read_prior: the config's pair in every slot, a subset by id, NaN for an id outside the engine
    eng.reset()
    p = host(eng.priors())
    assert p.shape == (8, 2) and np.all(p[:, 0] == cfg.signal_variance) and np.all(p[:, 1] == cfg.length_scale)
    q = host(eng.priors([7, 0, 8, -1]))
    assert same_bits(q[:2], p[[7, 0]]) and np.isnan(q[2:]).all()
    eng.close()
    exact = IPPEngine(cfg, capacity=8, state="factor", rank_cap=64, window_rows=0)
    assert int(exact.info.patch_layout) == 0
    with pytest.raises(IppError):
        exact.set_budget_prior(True)
    exact.close()

    # the env's engine has the 1.2 x head-room: 12 rows for the example prior; switched off, it runs as an engine that never got the call
    kw = dict(episode_steps=6, seed=9, budget=150.0, shuffle_budget=True)
    off = VecIPPEnv(cfg, 16, window_rows=-1, shuffle_prior_cov="device", **kw)
    assert int(off.engine.info.window_rows) == 12
    off.engine.set_budget_prior(False)
    off.device_priors = False  # (its resets install the config's prior, like the reset on done now)
    never = VecIPPEnv(cfg, 16, window_rows=12, **kw)
    assert int(never.engine.info.window_rows) == 12
    for e in (off, never):
        e.reset()
    resets = 0
    for t in range(6):
        a = cell_centre_actions(cfg, t, 0, 16, 16, [8.0, 14.0])
        r1, s1 = off.step(a)
        r2, s2 = never.step(a)
        torch.cuda.synchronize()
        assert torch.equal(r1, r2) and torch.equal(s1, s2), t
        for name in ("budget", "depth", "episode", "done", "prev"):
            assert torch.equal(getattr(off, name), getattr(never, name)), (t, name)
        assert same_bits(host(off.prior_scale), host(never.prior_scale))
        for e in range(16):
            assert torch.equal(off.mean(e), never.mean(e)) and torch.equal(off.diag(e), never.diag(e)), (t, e)
        resets += int(off.done.sum())
    assert resets > 0
    assert np.all(host(off.prior_scale) == np.array([cfg.signal_variance, cfg.length_scale]))
    off.close()
    never.close()


# ---------------------------------------------------------------------------------------------------- 6
SP_STEPS, SP_HISTORY, SP_B0 = 5, 2, 24.0


def make_selfplay(planes, B, seed=3):
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=8, temperature_scale=1.0, temperature_threshold=3, input_history_length=SP_HISTORY,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=True,
              shuffle_budget=False)
    md = dict(initial_budget=SP_B0, max_episode_steps=SP_STEPS, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications=UAV, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    # (a sequential search returns to its best action; in waves of 4 the 8 simulations leave single visits and no policy:
    # tests/test_hip_replay_compact.py)
    return SelfPlay(cfg40(), B, hp, md, planes=planes, seed=seed, sims_in_flight=1, episode_priors="device")


def test_compact_ring_archives_the_ended_episodes_prior():
    import torch
    from ipp_rl_amd.feature_planes import entry_records
    from ipp_rl_amd.planning.mcts_zero.selfplay import archive_slot
    from ipp_rl_amd.vec_env import start_prior
    from tests.test_feature_planes_host import ref_planes
    from tests.test_hip_feature_planes import _compare

    B, seed = 8, 3
    dense, compact = make_selfplay(True, B, seed), make_selfplay("compact", B, seed)
    cfg, S = compact.env.cfg, compact.slots
    assert int(compact.env.engine.info.window_rows) == 12 and compact.env.device_priors and dense.env.device_priors
    log = []  # per step: the episode every env was in, and the action it took
    while int(compact.env.episode.min().item()) < 2:
        assert len(log) < 12 * S
        ep = host(compact.env.episode).copy()
        dense.step()
        compact.step()
        log.append((ep, host(compact.action).copy()))
    assert torch.equal(dense.replay.flags, compact.replay.flags)
    assert same_bits(host(dense.env.prior_scale), host(compact.env.prior_scale))
    assert same_bits(host(compact.env.prior_scale), start_prior(cfg, seed, np.arange(B), host(compact.env.episode)))
    x, y = dense.replay.sample(16, num_augmented_samples=1), compact.replay.sample(16, num_augmented_samples=1)
    assert len(x) == len(y) == 7
    for i, (a, b) in enumerate(zip(x, y)):
        assert same_bits(host(a), host(b)), f"output {i} differs"
    assert bool(torch.isfinite(y[0]).all()) and bool((y[5] >= 0).all())

    # the archive slots the drawn rows read hold the prior of the rows' OWN episodes (not the pair of the episode the reset started)
    r = compact.replay
    rows = y[5][:2]
    hr = host(rows)
    rec = entry_records(r.entries[rows])
    tags = host(r.episode_tag)[hr]
    slots = rec["root_env"][:, 0]
    assert slots.tolist() == archive_slot(B, r.archive_episodes, hr % B, tags).tolist()
    want = np.concatenate([start_prior(cfg, seed, [int(e)], int(p)) for e, p in zip(hr % B, tags)])
    got = host(compact.env.engine.priors(slots.astype(np.int32)))
    assert same_bits(got, want), (got, want)
    # (the episodes really had different priors: the pair of the episode behind it differs)
    assert not np.any(want == np.concatenate([start_prior(cfg, seed, [int(e)], int(p) + 1) for e, p in zip(hr % B, tags)]))

    # one drawn row against fp64: the dense Kalman chain of its episode from that episode's prior, through the row's own step
    row, e, p = int(hr[0]), int(hr[0]) % B, int(tags[0])
    t_row = max(t for t in range(len(log)) if t % S == row // B and log[t][0][e] == p)
    acts = [log[t][1][e] for t in range(t_row) if log[t][0][e] == p]
    oc = orc.OracleConfig(x_dim=cfg.x_dim, y_dim=cfg.y_dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b,
                          signal_variance=cfg.signal_variance, length_scale=cfg.length_scale)
    fs = orc.factor_reset(oc, tuple(want[0]))
    states = [orc.factor_to_dense(oc, fs)]
    for a in acts:
        orc.factor_step(oc, fs, a)
        states.append(orc.factor_to_dense(oc, fs))
    valid = rec["valid"][0] == 1
    n_valid = int(valid.sum())
    assert valid[0] and n_valid == min(SP_HISTORY, len(acts) + 1) and list(valid[:n_valid]) == [True] * n_valid
    assert int(rec["rank"][0, 0]) == fs.U.shape[1]
    newest_first = states[::-1][:n_valid]
    positions, budgets = [rec["position"][0, k] for k in range(n_valid)], [float(rec["budget"][0, k]) for k in range(n_valid)]
    mean = host(r.mean[rows[:1]])[0].astype(np.float64)
    planes = host(r.gather_rows(rows[:1])[0])[0]
    ref = ref_planes(newest_first, positions, budgets, SP_HISTORY, cfg.x_dim, cfg.y_dim, fov=False, costs=True, mean=mean, thr=0.4, kf=0.0,
                     uav=UAV)
    worst = _compare(planes, ref, 5, SP_HISTORY, f"row {row} (env {e}, episode {p}, {len(acts)} steps)")
    print(f"row {row}: env {e}, episode {p}, {len(acts)} steps before it, largest state-plane error {worst:.3g}")
    dense.close()
    compact.close()


# ---------------------------------------------------------------------------------------------------- 7
def _learner(tmp):
    import torch
    from ipp_rl_amd.planning.mcts_zero import Learner, PolicyValueNetwork
    from tests import training_cases as tc
    from tests.test_hip_learn import SLOTS
    from tests.test_hip_per import _params

    cfg = cfg40()
    hp, md = _params(shuffle_prior_cov=True)
    net_hp = dict(input_channels=6, num_channels=8, dropout=0.0, use_silu=True, num_encoder_res_blocks=7, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=4, num_policy_head_conv_bn_blocks=1, num_value_head_conv_bn_blocks=1,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    hp = dict(hp, **net_hp, **tc.E2E_TRAIN)
    hp.update(batch_size=4, num_epochs=1, shared_network=True, num_self_play_iterations=2, num_episodes=1, num_workers=4,
              puct_init_decay=0.8, puct_init_min=4.0, dirichlet_alpha_decay=0.8, dirichlet_alpha_min=0.3,
              start_train_examples_history=2, train_examples_history_step=2, max_train_examples_history=10,
              continuous_network_update=True, num_arena_games=4, network_update_threshold=0.52)
    md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(3)
    module = PolicyValueNetwork(net_hp, md).to("cuda:0")
    return Learner(cfg, 4, hp, md, module, str(tmp), seed=6, capacity=4 * SLOTS, sims_in_flight=2, episode_priors="device")


def test_learn_loop_resumes_into_the_episodes_own_priors(tmp_path):
    """Two iterations of 4 envs x 1 episode in all: about 4 s.  The first backward pass of a process adds the convolution library's
    one-time kernel selection (about 30 s) to whichever test trains first (tests/test_hip_learn.py says the same of its own)."""
    from ipp_rl_amd.vec_env import start_prior

    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    a = _learner(a_dir)
    assert a.selfplay.env.device_priors and int(a.selfplay.env.engine.info.window_rows) == 12
    rec = a.learn(iterations=1)
    assert len(rec) == 1 and rec[0]["totals"]["episodes_kept"] == 4 and rec[0]["totals"]["examples"] >= 4
    counters = host(a.selfplay.env.episode).copy()
    assert same_bits(host(a.selfplay.env.prior_scale), start_prior(a.cfg, 6, np.arange(4), counters))
    assert np.all(counters >= 1)
    a.close()
    shutil.copytree(a_dir, b_dir)
    b = _learner(b_dir)
    seen = []
    begin = b.selfplay.begin_iteration

    def spy(*args, **kw):
        begin(*args, **kw)
        seen.append((host(b.selfplay.env.episode).copy(), host(b.selfplay.env.prior_scale).copy()))

    b.selfplay.begin_iteration = spy
    out = b.learn(resume=True)
    assert len(out) == 1 and out[0]["iteration"] == 1 and len(seen) == 1
    episode, prior = seen[0]
    assert np.array_equal(episode, counters + 1)  # (the first reset behind the restored counters)
    assert same_bits(prior, start_prior(b.cfg, 6, np.arange(4), counters + 1))
    assert not np.any(prior == start_prior(b.cfg, 6, np.arange(4), 0))
    b.close()
