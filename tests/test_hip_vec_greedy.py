"""
GPU tests of ipp_score_actions_envs (csrc/k_score_batch.h, include/ipp_engine.h) and the batched greedy planner (planning/vec_greedy.py): the reward of k
candidates per env for many envs in one call, against
  * ipp_step(IPP_COV_ONLY | IPP_PREDICT_ONLY) with the env id repeated, for every (env, candidate),
  * the fp64 oracle's predict step (planning/common/optimization.py:14-30 restated) on a subset of envs,
  * the single-env GreedyPlanner (tests/test_hip_score.py ties it to the reference's greedy goldens on 10x10 / 20x20),
and the policy loop against its host restatement.  The bar is the project's |reward - reference| < 1e-5 (tests/test_hip_score.py).
"""
import numpy as np
import pytest

from oracle import ipp_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = 1e-5
UAV = {"max_v": 2.0, "max_a": 2.0}
ALTS = np.array([5.0, 8.0, 12.0, 14.0])  # the four footprint classes at 4 m cells: 1x1 rf 1, 3x3 rf 1, 3x3 rf 2, 5x5 rf 2
DIM = 50


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ocfg_of(cfg):
    return orc.OracleConfig(x_dim=cfg.x_dim, y_dim=cfg.y_dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b)


def random_candidates(rs, cfg, n, k):
    """[n, k, 3]: random cells and altitudes; the first rows sit on the corners and borders."""
    cells = rs.randint(0, cfg.x_dim, size=(n, k, 2))
    edge = np.array([(0, 0), (0, DIM - 1), (DIM - 1, 0), (DIM - 1, DIM - 1), (0, 25), (25, 0), (DIM - 1, 25), (25, DIM - 1),
                     (1, 1), (1, DIM - 2), (DIM - 2, 1), (DIM - 2, DIM - 2), (0, 1), (1, 0), (DIM - 1, DIM - 2), (DIM - 2, DIM - 1)])
    for j in range(4):  # every border position with every altitude class
        cells[:, 16 * j: 16 * (j + 1)] = edge
    alt = ALTS[rs.randint(0, 4, size=(n, k))]
    for j in range(4):
        alt[:, 16 * j: 16 * (j + 1)] = ALTS[j]
    out = np.empty((n, k, 3))
    out[..., :2] = cfg.resolution * (cells + 0.5)
    out[..., 2] = alt
    return out


def predict_rewards(eng, env_ids, cands, prev, adaptive, flight):
    """The parent route: predict-only covariance-only ipp_step with the env id repeated, in launches of <= max_batch items."""
    import torch

    n, k = cands.shape[:2]
    flat = cands.reshape(-1, 3)
    ids = np.repeat(np.asarray(env_ids, dtype=np.int32), k)
    pv = np.repeat(prev, k, axis=0)
    out, st = [], []
    step = int(eng.max_batch)
    for i in range(0, n * k, step):
        r, s = eng.step(flat[i: i + step], pv[i: i + step], env_ids=ids[i: i + step], cov_only=True, predict_only=True,
                        adaptive=adaptive, use_flight_time=flight)
        out.append(r.clone()); st.append(s.clone())
    return torch.cat(out).reshape(n, k), torch.cat(st).reshape(n, k)


def test_parity_with_predict_step_and_oracle():
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.planning.common.actions import action_costs

    cfg = EngineConfig(x_dim=DIM, y_dim=DIM)
    oc = ocfg_of(cfg)
    B, K, T = 64, 256, 12
    eng = IPPEngine(cfg, capacity=B, state="factor", rank_cap=128, max_batch=4096, window_rows=-1, fixed_prior=True)
    assert int(eng.info.patch_layout) == 1
    rs = np.random.RandomState(11)
    white = rs.normal(size=(B, DIM, DIM))
    eng.reset(white_noise=white)
    nsteps = np.arange(B) % (T + 1)  # 0 .. 12 steps: ranks 0 to ~100
    oracle_envs = [0, 5, 12, 27]
    ost = {b: orc.env_reset(oc, white[b]) for b in oracle_envs}
    prev = np.tile(np.array([2.0, 2.0, 14.0]), (B, 1))
    for t in range(T):
        ids = np.nonzero(nsteps > t)[0].astype(np.int32)
        acts = np.stack([cfg.resolution * (rs.randint(0, DIM, len(ids)) + 0.5), cfg.resolution * (rs.randint(0, DIM, len(ids)) + 0.5),
                         ALTS[rs.randint(0, 4, len(ids))]], axis=1)
        eps = rs.normal(size=(len(ids), 9)) * (ids % 2)[:, None]  # odd envs measure with noise, even ones without
        _, st = eng.step(acts, prev[ids], env_ids=ids, meas_noise=eps)
        assert int(st.abs().sum()) == 0
        for j, b in enumerate(ids):
            if int(b) in ost:
                m = orc.num_measurements(orc.project_fov(oc, acts[j]), orc.resolution_factor(acts[j]))
                orc.env_step(oc, ost[int(b)], acts[j], eps[j, :m])
        prev[ids] = acts
    ranks = host(eng.ranks()).astype(int)
    assert ranks.min() == 0 and ranks.max() >= 60
    cands = random_candidates(rs, cfg, B, K)
    before = (torch.stack([eng.read_mean(b) for b in range(B)]).clone(), torch.stack([eng.read_diag(b) for b in range(B)]).clone(),
              eng.ranks().clone())
    for adaptive, flight in ((True, True), (False, False), (True, False)):
        reward, status, cost = eng.score_actions_envs(cands, prev, adaptive=adaptive, use_flight_time=flight, want_cost=True)
        assert int(status.abs().sum()) == 0
        ref, ref_st = predict_rewards(eng, np.arange(B), cands, prev, adaptive, flight)
        assert int(ref_st.abs().sum()) == 0
        diff = float((reward - ref).abs().max())
        print(f"[adaptive {adaptive}, flight time {flight}] {B} x {K} candidates: max |batched - predict step| = {diff:.3e}, "
              f"max reward {float(ref.max()):.3f}")
        assert diff < TOL
        r, c = host(reward), host(cost)
        worst = 0.0
        for b in oracle_envs:
            info = {"mean": ost[b].mean, "value_threshold": cfg.value_threshold, "interval_factor": cfg.interval_factor} if adaptive else None
            for j in range(K):
                want = orc.predict_step(oc, ost[b].P, prev[b], cands[b, j], UAV if flight else None, info)[0]
                worst = max(worst, abs(r[b, j] - want))
        print(f"    oracle envs {oracle_envs}: max |batched - oracle| = {worst:.3e}")
        assert worst < TOL
        want_cost = np.array([[action_costs(cands[b, j], prev[b], UAV if flight else None) for j in range(K)] for b in range(B)])
        assert np.max(np.abs(c - want_cost)) < 1e-12
    after = (torch.stack([eng.read_mean(b) for b in range(B)]), torch.stack([eng.read_diag(b) for b in range(B)]), eng.ranks())
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    eng.close()


def test_same_answers_as_single_env_planner():
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning import VecGreedyPolicy
    from ipp_rl_amd.planning.greedy import GreedyPlanner
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=DIM, y_dim=DIM)
    oc = ocfg_of(cfg)
    rs = np.random.RandomState(3)
    white = rs.normal(size=(DIM, DIM))
    B = 8
    pl = GreedyPlanner(cfg, 8, 14, 6, UAV, adaptive=True, state="factor")
    pl.reset(white_noise=white)
    env = VecIPPEnv(cfg, 2 * B, window_rows=-1, episode_steps=40)
    assert int(env.engine.info.patch_layout) == 1
    env.reset(white_noise=np.tile(white, (2 * B, 1, 1)))
    st = orc.env_reset(oc, white)
    prev = np.array([2.0, 2.0, 14.0])
    # (the second footprint lies beside the third waypoint: with a length scale below one cell, measurements farther away leave the
    # candidates around the waypoint in exact mirror ties, which no two summation orders break the same way)
    for a in (np.array([30.0, 22.0, 14.0]), np.array([82.0, 62.0, 8.0]), np.array([86.0, 70.0, 14.0])):
        eps = rs.normal(size=9)
        pl.engine.step(a[None], prev[None], env_ids=[0], meas_noise=eps[None])
        env.step(np.tile(a, (2 * B, 1)), meas_noise=np.tile(eps, (2 * B, 1)), auto_reset=False)
        m = orc.num_measurements(orc.project_fov(oc, a), orc.resolution_factor(a))
        orc.env_step(oc, st, a, eps[:m])
        prev = a
    policy = VecGreedyPolicy(env, 8, 14, 6)
    ids = np.arange(B)
    cands = policy.candidates(env.prev[:B])
    assert tuple(cands.shape) == (B, 5000, 3)
    reward, status = env.score_actions(cands, env_ids=ids)
    assert int(status.abs().sum()) == 0
    table = host(cands[0])
    single = pl.score(prev, table)
    r = host(reward)
    diff = float(np.max(np.abs(r - single[None, :])))
    print(f"full table, 8 envs: max |batched - GreedyPlanner.score| = {diff:.3e}")
    assert diff < TOL
    info = {"mean": st.mean, "value_threshold": cfg.value_threshold, "interval_factor": cfg.interval_factor}
    worst = 0.0
    for j in rs.choice(5000, 32, replace=False):
        want = orc.predict_step(oc, st.P, prev, table[j], UAV, info)[0]
        worst = max(worst, float(np.max(np.abs(r[:, j] - want))))
    print(f"32 sampled candidates: max |batched - oracle| = {worst:.3e}")
    assert worst < TOL
    want_wps = np.array(pl.search(prev, 200, 3))
    ways, valid = policy.search(ids, B + ids, np.full(B, 200.0), 3)
    assert bool(valid.all())
    got = host(ways)
    for b in range(B):
        assert np.array_equal(got[b], want_wps), (b, got[b], want_wps)
    env.close()


def test_padding_and_status():
    from ipp_rl_amd import EngineConfig, IPPEngine

    cfg = EngineConfig(x_dim=DIM, y_dim=DIM)
    eng = IPPEngine(cfg, capacity=4, state="factor", rank_cap=64, max_batch=64, window_rows=-1, fixed_prior=True)
    rs = np.random.RandomState(1)
    eng.reset(white_noise=rs.normal(size=(4, DIM, DIM)))
    prev = np.tile(np.array([2.0, 2.0, 14.0]), (4, 1))
    for t in range(3):
        a = np.stack([4.0 * rs.randint(0, DIM, 4) + 2.0, 4.0 * rs.randint(0, DIM, 4) + 2.0, ALTS[rs.randint(0, 4, 4)]], axis=1)
        eng.step(a, prev, meas_noise=rs.normal(size=(4, 9)))
        prev = a
    nan = np.nan
    row = np.array([[102.0, 98.0, 8.0], [nan, 1.0, 8.0], [102.0, 98.0, 60.0], [10.0, 10.0, nan], [2.0, 198.0, 14.0], [50.0, 50.0, 5.0],
                    [150.0, 30.0, 12.0]])  # k = 7: not a multiple of the group size
    ids = np.array([2, 2, 0], dtype=np.int32)  # repeats
    cands = np.tile(row, (3, 1, 1))
    reward, status, cost = eng.score_actions_envs(cands, prev[ids], env_ids=ids, want_cost=True)
    st, r, c = host(status).astype(int), host(reward), host(cost)
    assert np.array_equal(st, np.tile([0, 4, 4, 4, 0, 0, 0], (3, 1)))
    assert np.all(r[:, [1, 2, 3]] == 0) and np.all(r[:, [0, 4, 5, 6]] > 0)
    assert np.all(np.isnan(c[:, [1, 3]])) and np.all(np.isfinite(c[:, [0, 2, 4, 5, 6]]))
    assert np.array_equal(r[0], r[1])  # the same env twice
    good = [0, 4, 5, 6]
    ref, _ = predict_rewards(eng, ids, cands[:, good], prev[ids], True, True)
    assert float(np.max(np.abs(r[:, good] - host(ref)))) < TOL
    # n = 1, k = 1
    r1, s1 = eng.score_actions_envs(cands[:1, :1], prev[ids[:1]], env_ids=ids[:1])
    assert int(s1[0, 0]) == 0 and abs(float(r1[0, 0]) - r[0, 0]) == 0
    eng.close()


def test_policy_loop_matches_host_restatement_and_shards():
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning import VecGreedyPolicy
    from ipp_rl_amd.planning.vec_greedy import budget_filter, first_maximiser, radius_candidates
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=DIM, y_dim=DIM)
    B, RADIUS, BUDGET = 32, 30.0, 60.0

    def make(n, offset):
        env = VecIPPEnv(cfg, n, window_rows=-1, episode_steps=40, budget=BUDGET, seed=21, env_id_offset=offset)
        env.reset()
        return env, VecGreedyPolicy(env, 8, 14, 6, radius=RADIUS)

    env, policy = make(B, 0)
    trace = []
    starved = [3, 17, 30]

    def run(pol, tr):
        pol.run(10, trace=tr)
        pol.env.budget[torch.as_tensor([s for s in starved if s < pol.env.num_envs], device=pol.env.device, dtype=torch.long)] = 2.0
        pol.run(20, trace=tr)

    prevs = []
    orig_act = policy.act

    def act_and_record():
        prevs.append(env.prev.clone())
        return orig_act()

    policy.act = act_and_record
    run(policy, trace)
    torch.cuda.synchronize()
    assert len(trace) == 30
    ended = 0
    for t, (before, reward, cost, idx, has, actions, done) in enumerate(trace):
        bud, r, c, pv = host(before), host(reward), host(cost), host(prevs[t])
        valid = budget_filter(c, bud)
        want_idx, want_has = first_maximiser(r, valid)
        assert np.array_equal(host(has).astype(bool), want_has), t
        assert np.array_equal(host(idx).astype(int)[want_has], want_idx[want_has]), t
        a = host(actions)
        for b in range(B):
            cands = radius_candidates(pv[b], DIM, DIM, cfg.resolution, 8, 14, 6, RADIUS)
            assert np.array_equal(a[b], cands[want_idx[b]] if want_has[b] else pv[b]), (t, b)
        d = host(done).astype(bool)
        assert np.all(d[~want_has])  # no affordable action: the episode ends in this step
        ended += int(d.sum())
        if t == 10:
            assert not want_has[starved].any()
    assert ended > len(starved)  # budget-driven episode ends happened on their own too
    # two shards give the actions of one process
    for lo in (0, B // 2):
        senv, spol = make(B // 2, lo)
        starved_local = [s - lo for s in starved if lo <= s < lo + B // 2]
        tr = []
        spol.run(10, trace=tr)
        senv.budget[torch.as_tensor(starved_local, device=senv.device, dtype=torch.long)] = 2.0
        spol.run(20, trace=tr)
        torch.cuda.synchronize()
        for t in range(30):
            assert torch.equal(tr[t][5], trace[t][5][lo: lo + B // 2]), (lo, t)
        senv.close()
    env.close()


def test_refusals():
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd._ffi import IppError

    cfg = EngineConfig(x_dim=20, y_dim=20)
    cands = np.tile(np.array([[10.0, 10.0, 8.0], [30.0, 30.0, 14.0]]), (2, 1, 1))
    prev = np.tile(np.array([2.0, 2.0, 14.0]), (2, 1))
    for state, window_rows in (("dense", 0), ("factor", 0), ("factor", 12)):
        eng = IPPEngine(cfg, capacity=2, state=state, rank_cap=32, max_batch=8, window_rows=window_rows)
        assert int(eng.info.patch_layout) == 0
        eng.reset()
        with pytest.raises(IppError, match="patch-layout"):
            eng.score_actions_envs(cands, prev)
        eng.close()
