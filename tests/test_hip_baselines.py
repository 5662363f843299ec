"""
GPU end-to-end tests of the batched baseline missions (planning/vec_baselines.py), MissionLog and compare() (planning/mission_log.py)
on budget-mode envs.  The grid is 50x50: a budget-mode VecIPPEnv needs the patch layout, which a 10x10 grid cannot have
(tests/test_hip_budget.py pins that rule); the reference's waypoints were recorded on the same 50x50 grid
(tests/golden/gen_golden_baselines.py, keys *_g50_*).
"""
import numpy as np
import pytest

from ipp_rl_amd.planning import vec_baselines as vb
from tests.baseline_kernel_helpers import ALT_HI, ALT_LO, DTB, MAX_A, MAX_V, NUM_WAYPOINTS, RES, SLOPE, SPACING, STEP_SIZE

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DIM = 50
INIT = np.array([2.0, 2.0, 14.0])


def host(t):
    return t.detach().cpu().numpy()


def make_env(n, budget, seed=21, **kw):
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv

    env = VecIPPEnv(EngineConfig(x_dim=DIM, y_dim=DIM), n, window_rows=-1, episode_steps=40, budget=budget, seed=seed, **kw)
    env.reset()
    return env


def make_policy(kind, env, uniforms=None):
    from ipp_rl_amd import planning as pl

    if kind == "lawn":
        return pl.VecLawnmowerPolicy(env, DTB, ALT_LO, ALT_HI, STEP_SIZE, SPACING)
    if kind == "spiral":
        return pl.VecSpiralPolicy(env, DTB, ALT_LO, ALT_HI, NUM_WAYPOINTS, SLOPE)
    if kind.startswith("disc"):
        return pl.VecRandomDiscretePolicy(env, DTB, ALT_LO, ALT_HI, SPACING, adaptive=kind == "disc_ad", uniforms=uniforms)
    return pl.VecRandomContinuousPolicy(env, DTB, ALT_LO, ALT_HI, uniforms=uniforms)


def flown_by_execute(kind, way, budget):
    """How many of the planned waypoints the reference's execute() flies: all of the spiral's, else up to remaining_budget <= cost."""
    if kind == "spiral":
        return len(way)
    left, prev, n = budget, INIT, 0
    for w in way:
        c = float(vb.mission_cost(w, prev, True, MAX_V, MAX_A))
        if left <= c:
            break
        left, prev, n = left - c, w, n + 1
    return n


@pytest.mark.parametrize("kind", ["lawn", "spiral", "disc_na", "disc_ad", "cont"])
def test_waypoints_and_rewards_against_the_reference(golden, kind):
    import torch

    g = golden("baselines")
    B, T = 4, 14
    uniforms = None
    if kind in ("lawn", "spiral"):
        names = [f"{kind}_g{DIM}_time_{c}" for c in ("cut", "all", "cut", "all")]
        ways = [g[n] for n in names]
        budgets = np.array([float(g[n + "_budget"]) for n in names])
    elif kind.startswith("disc"):
        recs = [{k: g[f"disc_g{DIM}_{kind[5:]}_s{s}_{k}"] for k in ("budget", "count", "idx", "way")} for s in (0, 1, 2, 0)]
        ways = [r["way"] for r in recs]
        budgets = np.array([r["budget"][0] for r in recs])
        uniforms = np.full((T, B), 0.5)
        for e, r in enumerate(recs):
            n = min(T, len(r["idx"]))
            uniforms[:n, e] = (r["idx"][:n] + 0.5) / r["count"][:n]
    else:
        recs = [{k: g[f"cont_g{DIM}_s{s}_{k}"] for k in ("budget", "used", "u", "way")} for s in (0, 1, 2, 0)]
        ways = [r["way"] for r in recs]
        budgets = np.array([r["budget"][0] for r in recs])
        uniforms = np.full((T, B, vb.TRIALS, 3), 0.5)
        for e, r in enumerate(recs):
            pos = 0
            for t, used in enumerate(r["used"][:T]):
                uniforms[t, e, :used] = r["u"][pos: pos + used]
                pos += int(used)
    env = make_env(B, float(budgets.max()))
    env.budget.copy_(torch.as_tensor(budgets, device=env.device))
    policy = make_policy(kind, env, uniforms)
    trace = []
    policy.run(T, trace=trace, auto_reset=False)
    torch.cuda.synchronize()
    compared = np.zeros(B, dtype=int)
    for e in range(B):
        n_ref = flown_by_execute(kind, ways[e], budgets[e])
        for t, (before, prev_before, actions, has, reward, done) in enumerate(trace):
            if bool(host(has)[e]):
                assert t < len(ways[e]), (kind, e, t)  # never a waypoint the reference did not plan
                assert np.array_equal(host(actions)[e], ways[e][t]), (kind, e, t, host(actions)[e], ways[e][t])
                compared[e] += 1
            else:
                assert t >= n_ref, (kind, e, t, n_ref)  # no action: the reference's mission is over as well
                assert np.array_equal(host(actions)[e], host(prev_before)[e]) and float(host(env.budget)[e]) == 0.0
            if bool(host(done)[e]):  # the env's own rule (budget < resolution, max_episode_steps) ends the comparison
                break
    # how many waypoints each env must have flown: the reference's waypoints walked on the env's ledger -- charged with the flight time,
    # ended once the budget is below the resolution -- up to what the kind's rule flies (the discrete rule has no execute() test: every
    # recorded draw) and the T steps of this run.  The recordings keep every such comparison 1e-9 away from its threshold.
    expected = np.zeros(B, dtype=int)
    for e in range(B):
        limit = len(ways[e]) if kind.startswith("disc") else flown_by_execute(kind, ways[e], budgets[e])
        left, prev = budgets[e], INIT
        for w in ways[e][:min(limit, T)]:
            left, prev = left - float(vb.mission_cost(w, prev, True, MAX_V, MAX_A)), w
            expected[e] += 1
            if left < RES:
                break
    print(f"{kind}: waypoints compared per env {compared.tolist()}, expected {expected.tolist()}")
    assert np.array_equal(compared, expected) and expected.min() >= 2, (compared, expected)
    # the rewards: the same env stepped with those waypoints by hand
    twin = make_env(B, float(budgets.max()))
    twin.budget.copy_(torch.as_tensor(budgets, device=twin.device))
    for t, (before, prev_before, actions, has, reward, done) in enumerate(trace):
        r, _ = twin.step(actions, auto_reset=False)
        assert torch.equal(r, reward), (kind, t)
    env.close(); twin.close()


@pytest.mark.parametrize("kind", ["lawn", "spiral"])
def test_cursor_starts_again_after_a_reset_on_the_device(kind):
    import torch

    B, T, B0 = 6, 30, 100.0
    env = make_env(B, B0, seed=5, shuffle_budget=True)
    policy = make_policy(kind, env)
    trace = []
    policy.run(T, trace=trace)  # auto-reset: envs end at different steps
    torch.cuda.synchronize()
    table = policy.table_host
    cursor = np.zeros(B, dtype=int)
    resets = np.zeros(B, dtype=int)
    restarts = 0
    name = "lawnmower" if kind == "lawn" else "spiral"
    for t, (before, prev_before, actions, has, reward, done) in enumerate(trace):
        b, p, a, h, d = host(before), host(prev_before), host(actions), host(has).astype(bool), host(done).astype(bool)
        for e in range(B):
            want_has, want = vb.table_next(name, table, int(cursor[e]), p[e], float(b[e]), STEP_SIZE, env.use_flight_time, MAX_V, MAX_A)
            assert want_has == h[e] and np.array_equal(a[e], want), (kind, t, e)
            cursor[e] += want_has
            if resets[e] and cursor[e] == 1 and want_has:
                assert np.array_equal(a[e], table[0]) and np.array_equal(p[e], INIT)
                restarts += 1
            if d[e]:
                cursor[e] = 0
                resets[e] += 1
    ends = [int(np.argmax([bool(host(tr[5])[e]) for tr in trace])) for e in range(B)]
    assert resets.min() >= 1 and len(set(ends)) > 1 and restarts >= B, (resets, ends, restarts)  # envs ended at different steps
    # the device's cursors: those of the replay (an env that ended in the last step resets its cursor at its next decision)
    dev_cursor, ended_last = host(policy.cursor), host(trace[-1][5]).astype(bool)
    assert np.array_equal(dev_cursor[~ended_last], cursor[~ended_last])
    assert np.array_equal(host(policy.decision), np.full(B, T))
    env.close()


def test_philox_draws_do_not_depend_on_the_batch():
    import torch

    traces = []
    for n in (6, 3):
        env = make_env(n, 80.0, seed=9)
        policy = make_policy("disc_ad", env)
        tr = []
        policy.run(6, trace=tr)
        torch.cuda.synchronize()
        traces.append([host(x[2]) for x in tr] + [host(x[0]) for x in tr])
        if n == 6:  # the first decision against the host's copy of the uniform
            actions = vb.discrete_actions(DIM, DIM, RES, policy.levels_host)
            u = vb.baseline_uniform(9, np.arange(n), 0)
            for e in range(n):
                assert np.array_equal(traces[0][0][e], vb.random_discrete_next(actions, INIT, 80.0, u[e], True, MAX_V, MAX_A)[3]), e
        env.close()
    for a6, a3 in zip(*traces):
        assert np.array_equal(a6[:3], a3)
    assert len({tuple(a) for a in traces[0][0]}) > 1


@pytest.mark.parametrize("planner", ["greedy", "disc_na"])
def test_mission_log_behind_a_planner(planner):
    import torch
    from ipp_rl_amd.planning import MissionLog, VecGreedyPolicy
    from ipp_rl_amd.planning.common.actions import _trapezoid_time

    B, T, BUDGET = 4, 10, 24.0  # (a hop costs at least 2.5: every env ends within the run, and some planner acts again behind the end)
    env = make_env(B, BUDGET, seed=3)
    policy = VecGreedyPolicy(env, 8, 14, 6, radius=20.0) if planner == "greedy" else make_policy(planner, env)
    log = MissionLog(env, T + 1)
    log.record(first=True)
    xs = [[0.0] for _ in range(B)]
    ys = [[m.astype(np.float64)] for m in host(env.metrics())]
    ended = np.zeros(B, dtype=bool)
    for t in range(T):
        prev_before = env.prev.clone()
        actions, has = policy.act()
        actions = actions.clone()
        env.step(actions, auto_reset=False)
        log.record(prev_before, actions, has)
        m, h, d = host(env.metrics()).astype(np.float64), host(has).astype(bool), host(actions) - host(prev_before)
        dt = _trapezoid_time(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), MAX_V, MAX_A)
        for e in range(B):
            if h[e] and not ended[e]:
                xs[e].append(xs[e][-1] + dt[e]); ys[e].append(m[e])
        ended |= host(env.done).astype(bool)
    out = log.curves(BUDGET)
    torch.cuda.synchronize()
    assert min(len(x) for x in xs) >= 2 and ended.any()
    max_x, G = vb.curve_axis(max(x[-1] for x in xs), BUDGET)  # experiments.py:227-228
    assert abs(out["max_x_all"] - max(x[-1] for x in xs)) <= 1e-12 * max_x
    axis = np.linspace(0, min(out["max_x_all"], BUDGET), int(np.ceil(min(out["max_x_all"], BUDGET))))
    assert np.array_equal(host(out["axis"]), axis) and len(axis) == G
    got = host(out["per_env"])
    assert got.shape == (B, G, 8) and not host(out["overflow"]).any()
    worst = 0.0
    for e in range(B):
        y = np.array(ys[e])
        want = vb.curve_resample_host(np.array(xs[e]), y, max_x, G)
        assert np.array_equal(np.isfinite(got[e]), np.isfinite(want))
        ok = np.isfinite(want)
        bar = 1e-13 * max(1.0, np.abs(y[np.isfinite(y)]).max())
        err = np.abs(got[e][ok] - want[ok]).max()
        worst = max(worst, err / bar)
        assert err <= bar, (planner, e, err, bar)
    print(f"MissionLog behind {planner}: worst error / bar = {worst:.3f}, G = {G}")
    mean, sd = vb.curve_reduce_host(got)
    assert np.allclose(host(out["mean"]), mean, rtol=1e-12, atol=0, equal_nan=True) and np.allclose(host(out["sd"]), sd, rtol=1e-12, atol=1e-300, equal_nan=True)
    env.close()


def test_compare_two_planners():
    import torch
    from ipp_rl_amd.planning import VecGreedyPolicy, compare

    B, T, BUDGET = 4, 6, 45.0
    envs = [make_env(B, BUDGET, seed=3) for _ in range(2)]
    planners = {"greedy": VecGreedyPolicy(envs[0], 8, 14, 6, radius=20.0), "random": make_policy("disc_na", envs[1])}
    out = compare(planners, T, BUDGET)
    torch.cuda.synchronize()
    assert sorted(out) == ["greedy", "random"]
    for name, c in out.items():
        G = int(c["axis"].numel())
        assert G >= 1 and tuple(c["per_env"].shape) == (B, G, 8) and tuple(c["mean"].shape) == (G, 8) == tuple(c["sd"].shape), name
        assert not host(c["overflow"]).any() and bool(torch.isfinite(c["mean"][:, 5]).all())  # (the trace of the covariance)
        assert float(c["mean"][-1, 5]) < float(c["mean"][0, 5])  # flying reduces the map's uncertainty
    # both maps were the same at step 0: the same seed
    assert torch.equal(out["greedy"]["per_env"][:, 0], out["random"]["per_env"][:, 0])
    # a baseline's run(log=...) steps without the in-launch reset by default and refuses the combination
    from ipp_rl_amd.planning import MissionLog

    rnd = planners["random"]
    rnd.env.reset()
    log = MissionLog(rnd.env, 4)
    rnd.run(2, log=log)
    assert log.started and np.array_equal(host(rnd.env.episode), host(rnd.seen_episode)) and int(log.count.min()) >= 2
    with pytest.raises(ValueError):
        rnd.run(1, log=log, auto_reset=True)
    # every env is reusable: a reset and further steps, then closed
    for planner in planners.values():
        planner.env.reset()
        planner.run(2)
        torch.cuda.synchronize()
        assert int(planner.env.status.abs().sum()) == 0
        planner.env.close()
