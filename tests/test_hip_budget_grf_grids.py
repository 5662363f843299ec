"""
GPU tests of budget-mode envs with Gaussian random fields on grids other than 50x50 / 100x100 (VecIPPEnv(budget=..., grf_rows="all")):
an episode ends inside the step launch and its next field is generated behind that launch from the device's refill list
(ipp_generate_grf_refill) by a generator that draws its own noise -- the GEMM-Hartley kernel at 40x40, the 1024-thread DFT kernel at
132x132.  Every env's ground truth is the field of (seed, global env id, episode): compared bit for bit with the two-call path
(ipp_fill_normal_rows + ipp_generate_grf) after every step.  Sharding, parts, the scheduled mode and the planners on top.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
UAV = {"max_v": 2.0, "max_a": 2.0}


def host(t):
    return t.detach().cpu().numpy()


def cfg_of(n):
    from ipp_rl_amd import EngineConfig

    return EngineConfig(x_dim=n, y_dim=n)  # (simulation: gaussian_random_field, the default)


def actions(cfg, t, B, lo=0, total=None):
    from ipp_rl_amd.vec_env import cell_centre_actions

    return cell_centre_actions(cfg, t, lo, lo + B, total or B, [8.0, 14.0])


def check_ground_truths(env, label):
    """Every env carries the field of its CURRENT episode: white noise of (seed, GT_STREAM + episode, global env id) through the two calls."""
    import torch

    ep = host(env.episode).astype(np.int64)
    N = env.cfg.n_cells
    for e in np.unique(ep):
        sel = np.nonzero(ep == e)[0].astype(np.int32)
        white = torch.empty((len(sel), N), dtype=torch.float32, device=env.device)
        env.engine.normal_rows(white, N, env.seed, env.GT_STREAM + int(e), row_ids=sel, row_offset=env.env_id_offset)
        want = env.engine.generate_grf(white)
        for k, i in enumerate(sel):
            assert torch.equal(env.ground_truth(int(i)).reshape(-1), want[k]), (label, int(i), int(e))


def run_budget_env(n, B, steps, **kw):
    import torch
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = cfg_of(n)
    env = VecIPPEnv(cfg, B, episode_steps=4, window_rows=-1, budget=60.0, shuffle_budget=True, seed=7, grf_rows="all", **kw)
    assert env.field_kind == _ffi.IPP_FIELD_GRF and env.engine.grf_rows == "all"
    env.reset()
    torch.cuda.synchronize()
    check_ground_truths(env, "reset")
    done_steps = set()
    for t in range(steps):
        reward, status = env.step(torch.as_tensor(actions(cfg, t, B), device=env.device))
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and bool(torch.isfinite(reward).all()), t
        if bool(env.done.any()):
            done_steps.add(t)
        check_ground_truths(env, t)
    assert int(env.episode.min()) >= 1 and len(done_steps) >= 2, done_steps  # (envs ended episodes at different steps)
    return env


def test_staggered_resets_40():
    env = run_budget_env(40, 8, 12)
    assert int(env.engine.info.window_rows) == 10
    env.close()


def test_staggered_resets_132_dft_refill():
    from ipp_rl_amd import _ffi

    env = run_budget_env(132, 4, 6)
    assert env.engine.grf_generator()[0] == _ffi.IPP_GRF_GEN_DFT
    env.close()


def test_staggered_resets_40_device_priors():
    from ipp_rl_amd.vec_env import start_prior

    env = run_budget_env(40, 8, 12, shuffle_prior_cov="device")
    assert int(env.engine.info.window_rows) == 12
    want = start_prior(env.cfg, env.seed, np.arange(8), host(env.episode))
    assert np.array_equal(host(env.prior_scale), want)
    env.close()


QUANTITIES = ("budget", "depth", "episode", "done")


def make40(B, **kw):
    from ipp_rl_amd.vec_env import VecIPPEnv

    return VecIPPEnv(cfg_of(40), B, episode_steps=4, window_rows=-1, budget=60.0, shuffle_budget=True, seed=13, grf_rows="all", **kw)


def test_two_shards_equal_one():
    import torch

    cfg = cfg_of(40)
    one, two = make40(8), [make40(4, env_id_offset=o) for o in (0, 4)]
    for s in [one] + two:
        s.reset()
    n_done = 0
    for t in range(8):
        r1, _ = one.step(actions(cfg, t, 8))
        r2 = [s.step(actions(cfg, t, 4, lo=o, total=8))[0] for s, o in zip(two, (0, 4))]
        torch.cuda.synchronize()
        assert torch.equal(r1, torch.cat(r2)), t
        for q in QUANTITIES:
            assert torch.equal(getattr(one, q), torch.cat([getattr(s, q) for s in two])), (t, q)
        for e in range(8):
            s, k = two[e // 4], e % 4
            assert torch.equal(one.mean(e), s.mean(k)) and torch.equal(one.ground_truth(e), s.ground_truth(k)), (t, e)
        n_done += int(one.done.sum())
    assert n_done > 0
    for s in [one] + two:
        s.close()


def test_two_parts_equal_one():
    import torch

    cfg = cfg_of(40)
    one, two = make40(8), make40(8, parts=2)
    assert one.parts == 1 and two.parts == 2
    one.reset(); two.reset()
    n_done = 0
    for t in range(8):
        a = actions(cfg, t, 8)
        r1, _ = one.step(a)
        r2, _ = two.step(a)
        torch.cuda.synchronize()
        assert torch.equal(r1, r2), t
        for q in QUANTITIES:
            assert torch.equal(getattr(one, q), getattr(two, q)), (t, q)
        for e in range(8):
            assert torch.equal(one.mean(e), two.mean(e)) and torch.equal(one.ground_truth(e), two.ground_truth(e)), (t, e)
        n_done += int(one.done.sum())
    assert n_done > 0
    one.close(); two.close()


def test_scheduled_mode_same_fields_by_the_rows_route():
    """The scheduled (non-budget) mode picks the capability up through generate_fields_rows returning True: a faster road to the same
    fields, not other fields."""
    import torch
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg, B = cfg_of(40), 16
    plain = VecIPPEnv(cfg, B, episode_steps=4, stagger=True, window_rows=-1, seed=3)
    rows = VecIPPEnv(cfg, B, episode_steps=4, stagger=True, window_rows=-1, seed=3, grf_rows="all")
    plain.reset(); rows.reset()
    for t in range(10):
        a = torch.as_tensor(actions(cfg, t, B), device=rows.device)
        r1, s1 = plain.step(a)
        r2, s2 = rows.step(a)
        torch.cuda.synchronize()
        assert torch.equal(r1, r2) and torch.equal(s1, s2) and int(s2.abs().sum()) == 0, t
        for e in range(B):
            assert torch.equal(plain.mean(e), rows.mean(e)) and torch.equal(plain.ground_truth(e), rows.ground_truth(e)), (t, e)
    assert plain.alt_blocks == 0 and rows.alt_blocks > 0  # (the rows route was taken, and only where it was switched on)
    plain.close(); rows.close()


def params(sims=8):
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=sims, temperature_scale=1.0, temperature_threshold=3, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=24.0, max_episode_steps=4, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications=UAV, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    return hp, md


def test_selfplay_on_grf_40():
    import torch
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    hp, md = params()
    # (a sequential search returns to its best action; in waves of 4 the 8 simulations leave single visits and no policy, so no sample:
    # tests/test_hip_replay_compact.py)
    sp = SelfPlay(cfg_of(40), 4, hp, md, infer=None, planes="compact", seed=5, sims_in_flight=1, grf_rows="all")
    sp.run(6)
    torch.cuda.synchronize()
    assert int((sp.replay.flags == 2).sum()) > 0  # committed rows
    assert int(sp.env.episode.min()) >= 1
    check_ground_truths(sp.env, "selfplay")
    sp.close()


def test_arena_on_grf_40():
    from ipp_rl_amd.planning.mcts_zero.arena import Arena

    hp, md = params()
    arena = Arena(cfg_of(40), 2, hp, md, None, None, seed=5, sims_in_flight=1, grf_rows="all")
    out = arena.evaluate(num_games=2, threshold=0.5)
    gp, gc = arena.last["prev"]["game_values"], arena.last["curr"]["game_values"]
    assert gp.shape == (2, 1) and np.array_equal(gp, gc) and np.all(np.isfinite(gc))  # (the same players: the same games)
    assert out["ratio"] == 0.5 and np.all(arena.last["curr"]["game_steps"] >= 1)
