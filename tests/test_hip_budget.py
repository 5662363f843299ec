"""
GPU tests of the budget ledger (IPP_BUDGET / IPP_RESET_ON_DONE, ipp_set_budget, ipp_generate_grf_refill; VecIPPEnv(budget=B0)): the
reference's budget-driven episode loop (planning/mcts_zero/episode_generators.py:109-150) on the device -- remaining_budget -= action
cost, depth += 1, done = !(depth < max_episode_steps and remaining_budget >= resolution), a done env reset inside the step launch and
its next ground truth generated behind it from the device's refill list.
"""
import numpy as np
import pytest

from ipp_rl_amd import _ffi

pytestmark = pytest.mark.gpu
TOL = 1e-5  # rewards / diagonals against the golden episodes (tests/test_hip_window.py)
INIT = np.array([2.0, 2.0, 14.0])


def host(t):
    return t.detach().cpu().numpy()


def flight_cost(a, p, vmax=2.0, amax=2.0):
    """actions.py:32-41 in fp64, vectorised over rows."""
    d = np.sqrt(np.sum((a - p) ** 2, axis=-1))
    d_acc = np.minimum(0.5 * d, vmax * vmax / (2 * amax))
    return (d - 2 * d_acc) / vmax + 2 * np.sqrt(2 * d_acc / amax)


@pytest.mark.parametrize("name", ["episode_rf1_50_s0", "episode_mixed_50_s1"])
@pytest.mark.parametrize("mode", ["distance", "flight_time"])
def test_ledger_matches_reference_loop(golden, name, mode):
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine

    g, bud = golden(name), golden("budget")
    key = f"{name}__{mode}"
    dim = g["gt"].shape[0]
    for j, b0 in enumerate(bud[key + "__budget"]):
        steps = int(bud[key + "__steps"][j])
        rem = bud[key + "__remaining"][j]
        eng = IPPEngine(EngineConfig(x_dim=dim, y_dim=dim), capacity=1, state="factor", rank_cap=400, window_rows=12)
        assert eng.info.patch_layout == 1
        dev = eng.device
        budget = torch.tensor([b0], dtype=torch.float64, device=dev)
        depth = torch.zeros(1, dtype=torch.int32, device=dev)
        episode = torch.zeros(1, dtype=torch.int64, device=dev)
        done = torch.zeros(1, dtype=torch.uint8, device=dev)
        refill = torch.full((1,), -7, dtype=torch.int32, device=dev)
        eng.set_budget(budget, depth, episode, done, refill, float(b0), 40)
        eng.reset(env_ids=[0], white_noise=g["white"][None])
        assert eng.generate_grf_rows(1, 3, 1 << 40, None, row_ids=[0])  # the next episode's field, staged for the reset on done
        prev = torch.tensor(INIT, dtype=torch.float64, device=dev).reshape(1, 3)
        worst = dict(reward=0.0, diag=0.0)
        for t in range(steps):
            reward, status = eng.step(g["actions"][t][None], prev, meas_noise=g["eps"][t][None], update_prev=True, budget=True,
                                      reset_on_done=True, init_action=INIT, use_flight_time=(mode == "flight_time"))
            torch.cuda.synchronize()
            assert int(status[0]) == 0
            last = t == steps - 1
            assert bool(done[0]) == last, (key, b0, t)
            assert int(refill[0]) == (0 if last else -1)
            if not last:
                assert abs(float(budget[0]) - rem[t]) <= 1e-9 * b0, (key, b0, t, float(budget[0]), rem[t])
                assert int(depth[0]) == t + 1
            if mode == "flight_time":  # (the golden episodes' rewards are flight-time rewards)
                worst["reward"] = max(worst["reward"], abs(float(reward[0]) - g["reward"][t]))
                if not last:
                    worst["diag"] = max(worst["diag"], float(np.max(np.abs(host(eng.read_diag(0)).astype(np.float64) - g["diag"][t]))))
        assert max(worst.values()) < TOL, (key, b0, worst)
        # terminated: the env was reset by the same launch
        assert eng.rank(0) == 0
        assert np.array_equal(host(prev)[0], INIT)
        assert float(budget[0]) == float(b0) and int(depth[0]) == 0 and int(episode[0]) == 1
        d = host(eng.read_diag(0))
        assert np.all(np.abs(d - eng.cfg.signal_variance) < 1e-5)
        eng.close()


def _actions(cfg, t, B, lo=0, total=None, altitudes=(8.0, 14.0)):
    from ipp_rl_amd.vec_env import cell_centre_actions

    return cell_centre_actions(cfg, t, lo, lo + B, total or B, list(altitudes))


@pytest.mark.parametrize("stagger", [False, True])
@pytest.mark.parametrize("parts", [1, 2])
def test_huge_budget_equals_fixed_schedule(stagger, parts):
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=50, y_dim=50)
    B, T = 256, 6
    fixed = VecIPPEnv(cfg, B, episode_steps=T, stagger=stagger, window_rows=-1, seed=21, parts=parts)
    bud = VecIPPEnv(cfg, B, episode_steps=T, stagger=stagger, window_rows=-1, seed=21, parts=parts, budget=1e30)
    assert bud.parts == parts
    fixed.reset(); bud.reset()
    sample = [0, 1, 77, 130, 255]
    dev = bud.device
    for t in range(3 * T + 2):
        a = torch.as_tensor(_actions(cfg, t, B), device=dev)
        rf, sf = fixed.step(a)
        rb, sb = bud.step(a)
        if not stagger and (t + 1) % T == 0:
            fixed.reset()  # (lock step: the fixed schedule's episode ends are the caller's resets)
        torch.cuda.synchronize()
        assert torch.equal(rf, rb) and torch.equal(sf, sb), t
        assert int(sb.abs().sum()) == 0
        assert torch.equal(fixed.prev, bud.prev), t
        assert torch.equal(fixed.engine.ranks(), bud.engine.ranks()), t
        ph = host(bud.phase).astype(np.int64)
        expect_done = (t + 1 + ph) % T == 0
        assert np.array_equal(host(bud.done).astype(bool), expect_done), t
        assert np.array_equal(host(bud.depth), (t + 1 + ph) % T), t
        for e in sample:
            assert torch.equal(fixed.mean(e), bud.mean(e)), (t, e)
            assert torch.equal(fixed.diag(e), bud.diag(e)), (t, e)
            assert torch.equal(fixed.ground_truth(e), bud.ground_truth(e)), (t, e)
    fixed.close(); bud.close()


def test_data_dependent_termination_against_numpy_ledger():
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv, start_budget

    cfg = EngineConfig(x_dim=50, y_dim=50)
    B, T, B0, seed = 4096, 40, 400.0, 5
    env = VecIPPEnv(cfg, B, episode_steps=T, window_rows=-1, seed=seed, budget=B0, shuffle_budget=True)
    env.reset()
    dev = env.device
    gid = np.arange(B)
    ep = np.zeros(B, dtype=np.int64)
    bud = start_budget(B0, True, seed, gid, ep)
    assert np.array_equal(host(env.budget), bud)
    dep = np.zeros(B, dtype=np.int64)
    prev = np.tile(INIT, (B, 1))
    rs = np.random.RandomState(3)
    alts = np.array([8.0, 14.0])
    ends = set()
    gt_checked = 0
    margin = 1e-6 * B0
    for t in range(14):
        a = np.stack([4.0 * rs.randint(0, 50, B) + 2.0, 4.0 * rs.randint(0, 50, B) + 2.0, alts[rs.randint(0, 2, B)]], axis=1)
        for _ in range(20):  # no ledger within `margin` of the threshold: rounding cannot flip a done flag
            near = np.abs(bud - flight_cost(a, prev) - cfg.resolution) < margin
            if not near.any():
                break
            a[near, 0] = 4.0 * rs.randint(0, 50, int(near.sum())) + 2.0
        assert not near.any()
        nb, nd = bud - flight_cost(a, prev), dep + 1
        done = ~((nd < T) & (nb >= cfg.resolution))
        ep = np.where(done, ep + 1, ep)
        bud = np.where(done, start_budget(B0, True, seed, gid, ep), nb)
        dep = np.where(done, 0, nd)
        prev = np.where(done[:, None], INIT[None], a)
        reward, status = env.step(torch.as_tensor(a, device=dev))
        torch.cuda.synchronize()
        assert np.array_equal(host(env.done).astype(bool), done), t
        assert np.max(np.abs(host(env.budget) - bud)) <= 1e-9 * B0, t
        assert np.array_equal(host(env.depth), dep) and np.array_equal(host(env.episode), ep), t
        assert np.array_equal(host(env.prev), prev), t
        assert int(status.abs().sum()) == 0 and bool(torch.isfinite(reward).all()), t
        ends.update(int(x) for x in nd[done])
        for e in np.nonzero(done)[0][:3]:  # sampled resets: the new episode's field, bit for bit
            want = torch.empty((1, cfg.n_cells), dtype=torch.float32, device=dev)
            assert env.engine.generate_grf_rows(1, seed, env.GT_STREAM + int(ep[e]), want, row_ids=[int(e)])
            assert torch.equal(env.ground_truth(int(e)).reshape(-1), want[0]), (t, e)
            gt_checked += 1
    assert len(ends) >= 4 and gt_checked >= 10, (ends, gt_checked)  # envs ended at many different depths
    env.close()


def test_one_step_episodes_always_find_a_staged_plane():
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=50, y_dim=50)
    B = 512
    env = VecIPPEnv(cfg, B, episode_steps=40, window_rows=-1, seed=9, budget=5.0)  # below one move: every step ends the episode
    env.reset()
    for t in range(6):
        a = _actions(cfg, t, B, altitudes=(8.0,))  # (z = 8 against the start's 14: every move costs >= 4 s)
        reward, status = env.step(a)
        torch.cuda.synchronize()
        assert bool(env.done.all()), t
        assert int((status == _ffi.STATUS_NOT_PD).sum()) == 0 and int(status.abs().sum()) == 0, t
        assert bool(torch.isfinite(reward).all()), t
        assert bool((env.episode == t + 1).all()) and bool((env.depth == 0).all()) and bool((env.budget == 5.0).all()), t
        assert int(env.engine.ranks().abs().sum()) == 0
        assert bool((env.refill >= 0).all())
    env.close()


def test_sharded_budgets_match_single_shard():
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=50, y_dim=50)
    B = 96
    one = VecIPPEnv(cfg, B, episode_steps=40, window_rows=-1, seed=13, budget=250.0, shuffle_budget=True)
    two = [VecIPPEnv(cfg, 48, episode_steps=40, window_rows=-1, seed=13, budget=250.0, shuffle_budget=True, env_id_offset=o)
           for o in (0, 48)]
    one.reset()
    for s in two:
        s.reset()
    n_done = 0
    for t in range(10):
        r1, _ = one.step(_actions(cfg, t, B))
        r2 = [s.step(_actions(cfg, t, 48, lo=o, total=B))[0] for s, o in zip(two, (0, 48))]
        torch.cuda.synchronize()
        assert torch.equal(r1, torch.cat(r2)), t
        assert torch.equal(one.budget, torch.cat([s.budget for s in two])), t
        assert torch.equal(one.done, torch.cat([s.done for s in two])), t
        assert torch.equal(one.episode, torch.cat([s.episode for s in two])), t
        n_done += int(one.done.sum())
    assert n_done > 0
    one.close()
    for s in two:
        s.close()


def test_rejected_combinations_launch_nothing():
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd._ffi import IppError
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=50, y_dim=50)
    for kw in (dict(shuffle_prior_cov=True), dict(state="dense"), dict(window_rows=0), dict(budget=3.0)):
        args = dict(window_rows=-1, budget=100.0)
        args.update(kw)
        with pytest.raises(ValueError):
            VecIPPEnv(cfg, 8, episode_steps=4, **args)
    with pytest.raises(ValueError):  # a grid without the in-generator noise
        VecIPPEnv(EngineConfig(x_dim=40, y_dim=40), 8, episode_steps=4, window_rows=-1, budget=100.0)
    env = VecIPPEnv(cfg, 8, episode_steps=4, window_rows=-1, budget=100.0)
    env.reset()
    with pytest.raises(ValueError):
        env.reset(env_ids=[0])
    env.close()

    # the ABI: every refused call leaves its outputs untouched
    def fresh(**kw):
        return IPPEngine(cfg, capacity=8, state="factor", rank_cap=64, **kw)

    def ledger(dev, n=8):
        return (torch.full((n,), 50.0, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                torch.full((n,), -1, dtype=torch.int32, device=dev))

    exact = fresh(window_rows=0)
    assert exact.info.patch_layout == 0
    with pytest.raises(IppError):
        exact.set_budget(*ledger(exact.device), 50.0, 4)
    exact.close()
    eng = fresh(window_rows=-1, fixed_prior=True)
    dev = eng.device
    led = ledger(dev)
    prev = torch.tensor(INIT, dtype=torch.float64, device=dev).repeat(8, 1)
    acts = _actions(cfg, 0, 8)
    reward = torch.full((8,), 123.0, dtype=torch.float32, device=dev)
    with pytest.raises(IppError):  # no ledger installed yet
        eng.step(acts, prev, budget=True, reward_out=reward)
    eng.set_budget(*led, 50.0, 4)
    with pytest.raises(IppError):  # not a flag of ipp_step
        eng.step(acts, prev, budget=True, predict_only=True, reward_out=reward)
    with pytest.raises(IppError):  # subsets
        eng.step(acts[:4], prev[:4], env_ids=[0, 1, 2, 3], budget=True, reward_out=reward[:4])
    with pytest.raises(IppError):  # reset on done without budget / without init_action
        eng.step(acts, prev, reset_on_done=True, init_action=INIT, reward_out=reward)
    with pytest.raises(IppError):
        eng.step(acts, prev, budget=True, reset_on_done=True, reward_out=reward)
    torch.cuda.synchronize()
    assert bool((reward == 123.0).all())
    assert bool((led[0] == 50.0).all()) and int(led[1].abs().sum()) == 0
    dense = IPPEngine(cfg, capacity=8, state="dense", rank_cap=64)
    with pytest.raises(IppError):
        dense.set_budget(*ledger(dense.device), 50.0, 4)
    dense.close()
    eng.close()
