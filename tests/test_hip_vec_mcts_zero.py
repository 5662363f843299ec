"""
GPU tests of the batched MCTS-zero deployment planner and the arena (planning/vec_mcts_zero.py, planning/mcts_zero/arena.py) on the engine,
with tests/test_hip_selfplay.py's parameters (24 simulations, episodes of up to 6 steps, budget 40, altitudes 8 / 14, 4 envs of 40x40):
  * every step's decision equals ensemble_pick_host of that step's device policies and the env moved there; root-parallel workers see
    different root noise; without noise they agree and 3 workers act like 1;
  * the deploy read-out equals the host read-out of the same trees; search_device's default is unchanged;
  * the arena: a network against itself draws exactly (paired games), two shards give the games of one process, the temperature-0
    player takes SelfPlay's temperature-0 actions and its game values are SelfPlay's episode values; a root without a policy ends its
    game in that step.
"""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def host(t):
    return t.detach().cpu().numpy()


def _cfg():
    from ipp_rl_amd import EngineConfig

    return EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")


def _policy(B=4, workers=1, mode="deploy", seed=5, env_id_offset=0, games_per_env=1, infer=None, sims_in_flight=4, **over):
    from ipp_rl_amd.planning import VecMctsZeroPolicy
    from ipp_rl_amd.planning.vec_mcts_zero import make_env
    from tests.test_hip_selfplay import _params

    hp, md = _params(**over)
    env = make_env(_cfg(), B, hp, md, workers=workers, sims_in_flight=sims_in_flight, seed=seed, env_id_offset=env_id_offset)
    return VecMctsZeroPolicy(env, hp, md, infer, workers=workers, mode=mode, games_per_env=games_per_env, sims_in_flight=sims_in_flight)


def _check_step(pol, before_prev):
    """The step's decision against the host restatement of its device policies; where the env went."""
    from ipp_rl_amd.planning.mcts_zero.selfplay import ARGMAX_STREAM, step_uniform
    from ipp_rl_amd.planning.vec_mcts_zero import MODES, ensemble_pick_host

    env, B, W = pol.env, pol.num_envs, pol.workers
    p, vi, ok = (host(pol.last[k]) for k in ("policy", "valid_idx", "ok"))
    ens, act_idx, action = host(pol.last["ensemble"]), host(pol.action_idx), host(pol.action)
    forced, done, prev = host(pol.forced), host(env.done), host(env.prev)
    actions, init = host(pol.actions), host(env.init_prev)
    differ = 0
    for e in range(B):
        rows = slice(e * W, (e + 1) * W)
        u = step_uniform(ARGMAX_STREAM, pol.seed, e + env.env_id_offset, pol._ep0[e], pol._d0[e])
        want = ensemble_pick_host(p[rows], vi[rows], ok[rows], MODES[pol.mode], float(u), num_actions=pol.num_actions)
        assert act_idx[e] == want["action_idx"] and forced[e] == want["forced"]
        assert np.array_equal(ens[e], want["ensemble"])
        went = before_prev[e] if want["forced"] else actions[want["action_idx"]]
        assert np.array_equal(action[e], went)
        ended = bool(done[e]) or bool(want["forced"])
        assert np.array_equal(prev[e], init[e] if ended else went)  # (an episode that ended: the env reset to Mission.init_action)
        differ += int(any(not np.array_equal(p[e * W], p[e * W + w]) for w in range(1, W)))
    return differ


def _step_checked(pol):
    import torch

    env = pol.env
    pol._ep0, pol._d0 = host(env.episode).copy(), host(env.depth).copy()
    before = host(env.prev).copy()
    pol.step()
    torch.cuda.synchronize()
    return _check_step(pol, before)


def test_deploy_steps_equal_the_host_restatement():
    """3: six steps, 3 root-parallel workers with 25 % root noise."""
    pol = _policy(workers=3, dirichlet_eps=0.25)
    assert pol._roots.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    differ, moved = 0, 0
    for _ in range(6):
        differ += _step_checked(pol)
        moved += int((host(pol.forced) == 0).sum())
    assert differ >= 1  # (the workers' noise is keyed per root: their policies are not copies of each other)
    assert moved >= 12
    pol.env.close()


def test_run_keeps_a_trace_with_metrics():
    pol = _policy(workers=1, num_mcts_simulations=8)
    trace = []
    pol.run(2, trace=trace, metrics=True)
    assert len(trace) == 2 and pol.t == 2
    for row in trace:
        assert set(row) == {"budget", "action_idx", "actions", "forced", "reward", "done", "metrics"}
        assert row["actions"].shape == (4, 3) and row["action_idx"].shape == (4,)
    assert np.array_equal(host(trace[1]["actions"]), host(pol.action))
    pol.env.close()


def test_without_noise_three_workers_act_like_one():
    """3b"""
    import torch

    three, one = _policy(workers=3), _policy(workers=1)
    for _ in range(6):
        for pol in (three, one):
            pol.step()
        torch.cuda.synchronize()
        p = host(three.last["policy"]).reshape(4, 3, -1)
        assert np.array_equal(p[:, 0], p[:, 1]) and np.array_equal(p[:, 0], p[:, 2])
        assert np.array_equal(p[:, 0], host(one.last["policy"]))
        assert np.array_equal(host(three.action_idx), host(one.action_idx)) and np.array_equal(host(three.action), host(one.action))
        assert np.array_equal(host(three.env.reward), host(one.env.reward))
    three.env.close()
    one.env.close()


def test_deploy_readout_and_unchanged_default():
    """3c"""
    import torch

    pol = _policy(workers=3, dirichlet_eps=0.25)
    pol.step()
    actions, _ = pol.act()
    torch.cuda.synchronize()
    env, m, R = pol.env, pol.mcts, 12
    p, vi, ok = (host(pol.last[k]).copy() for k in ("policy", "valid_idx", "ok"))
    rows = m._policies_rows(R, 1.0, True, None)
    for j in range(R):
        if rows[j] is None:
            assert not ok[j]
            continue
        assert ok[j]
        dense = np.zeros(m.num_actions)
        dense[list(rows[j][0].keys())] = list(rows[j][0].values())
        K = int((vi[j] >= 0).sum())
        np.testing.assert_allclose(p[j, :K], dense[vi[j, :K]], rtol=0, atol=1e-12)
        assert abs(p[j, :K].sum() - 1.0) < 1e-12 and np.all(p[j, K:] == 0)
    # the same roots without the new argument, and with its default spelled out: the same bits (act() has not stepped the env)
    rep = lambda x: x.repeat_interleave(3, dim=0)  # noqa: E731
    args = (pol._roots, rep(env.prev), rep(env.budget), [1.0], rep(pol.tie_u))
    out = m.search_device(*args)
    a = [host(out["policy"][0]).copy(), host(out["valid_idx"]).copy(), host(out["ok"]).copy()]
    out = m.search_device(*args, deploy_time=False)
    b = [host(out["policy"][0]), host(out["valid_idx"]), host(out["ok"])]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[1], vi) and not np.array_equal(a[0], p)  # (the deployment read-out keeps the forced playouts)
    pol.env.close()


def _small_net():
    import torch

    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork
    from tests.test_hip_selfplay import _params

    cfg = _cfg()
    _, md = _params()
    net_hp = dict(input_channels=6, num_channels=8, dropout=0.0, use_silu=True, num_encoder_res_blocks=7, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=4, num_policy_head_conv_bn_blocks=1, num_value_head_conv_bn_blocks=1,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    net_md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(3)
    sd = PolicyValueNetwork(net_hp, net_md).eval().state_dict()
    return DevicePolicyValueNet(net_hp, net_md, sd, side=cfg.n_cells, precision="fp32", max_batch=8, device="cuda:0")


@pytest.mark.parametrize("network", [False, True])
def test_arena_of_a_network_against_itself_draws(network):
    """3d: the same callback twice: paired games, equal bit for bit."""
    from ipp_rl_amd.planning.mcts_zero import Arena
    from tests.test_hip_selfplay import _params

    hp, md = _params()
    net = _small_net() if network else None
    infer = net.infer if network else None
    arena = Arena(_cfg(), 4, hp, md, infer, infer, seed=5, sims_in_flight=2 if network else 4)
    out = arena.evaluate(num_games=4, threshold=0.52)
    gp, gc = arena.last["prev"]["game_values"], arena.last["curr"]["game_values"]
    assert gp.shape == (4, 1) and np.array_equal(gp, gc) and np.array_equal(arena.last["prev"]["game_steps"], arena.last["curr"]["game_steps"])
    seq = 0.0
    for e in range(4):
        seq += gc[e, 0]
    assert out["total_curr"] == seq and out["total_prev"] == seq and seq > 0
    assert out["ratio"] == 0.5 and out["accepted"] is False and out["avg_reward_curr"] == seq / 4
    again = arena.evaluate(num_games=4, threshold=0.5)
    assert again["accepted"] is True and again["ratio"] == 0.5 and again["total_curr"] == seq  # (a fresh env: the same games again)
    if net is not None:
        net.close()


def test_two_shards_play_the_games_of_one_process():
    """3e: arena mode, two workers with root noise: the pick's draws and the search's keys follow the global env id."""
    one = _policy(B=4, workers=2, mode="arena", dirichlet_eps=0.25)
    two = [_policy(B=2, workers=2, mode="arena", env_id_offset=o, dirichlet_eps=0.25) for o in (0, 2)]
    res = [p.play() for p in [one] + two]
    assert res[0]["games"] == 4
    assert np.array_equal(host(res[0]["game_values"]), np.concatenate([host(r["game_values"]) for r in res[1:]]))
    assert np.array_equal(host(res[0]["game_steps"]), np.concatenate([host(r["game_steps"]) for r in res[1:]]))
    assert np.all(host(res[0]["game_steps"]) >= 1)
    for p in [one] + two:
        p.env.close()


def test_arena_player_is_selfplay_at_temperature_zero():
    """3f: the pick draws what ipp_selfplay_record draws: same actions at every step, game values = SelfPlay's episode values."""
    import torch

    from ipp_rl_amd.planning.mcts_zero import SelfPlay
    from tests.test_hip_selfplay import _params

    hp, md = _params(temperature_scale=0.0)
    sp = SelfPlay(_cfg(), 4, hp, md, infer=None, seed=5, random_init_action=False, planes=False)
    pol = _policy(workers=1, mode="arena", seed=5, temperature_scale=0.0)
    first = np.full(4, np.nan)
    for _ in range(7):
        sp.step()
        pol.step()
        torch.cuda.synchronize()
        assert np.array_equal(host(sp.action_idx), host(pol.action_idx)) and np.array_equal(host(sp.action), host(pol.action))
        assert np.array_equal(host(sp.last["policy_1"]), host(pol.last["policy"]))
        ev = host(sp.episode_values)
        first = np.where(np.isnan(first), ev, first)
    assert not np.isnan(first).any() and np.all(host(pol.games) == 1)
    np.testing.assert_allclose(host(pol.game_values)[:, 0], first, rtol=0, atol=1e-12)
    sp.close()
    pol.env.close()


def test_a_root_without_a_policy_ends_its_game():
    """3g: a budget below the cheapest action: no valid action, no policy; the game ends in that step without the step's reward."""
    import torch

    pol = _policy(workers=3, games_per_env=2, max_episode_steps=10, initial_budget=400.0)
    env = pol.env
    pol.step()
    pol.step()
    torch.cuda.synchronize()
    assert np.all(host(pol.games) == 0) and np.all(host(pol.steps) == 2)
    ret0, ep0 = host(pol.ret).copy(), host(env.episode).copy()
    env.budget[1] = 1e-3
    _, has = pol.act()
    assert host(has).tolist() == [True, False, True, True] and np.all(host(pol.last["ok"])[3:6] == 0)
    assert host(env.budget)[1] == 0.0 and host(pol.action_idx)[1] == -1
    env.budget[1] = 1e-3  # (the pick zeroed it; the step below searches again)
    pol.step()
    torch.cuda.synchronize()
    assert host(pol.games).tolist() == [0, 1, 0, 0]
    assert host(pol.game_values)[1, 0] == ret0[1] and host(pol.game_steps)[1, 0] == 2
    assert host(pol.steps).tolist() == [3, 0, 3, 3] and host(pol.ret)[1] == 0.0
    assert host(env.episode)[1] == ep0[1] + 1 and host(env.depth)[1] == 0 and np.all(host(env.episode)[[0, 2, 3]] == ep0[[0, 2, 3]])
    assert pol.totals.tolist() == [ret0[1], 1.0, 2.0, 0.0]
    pol.env.close()
