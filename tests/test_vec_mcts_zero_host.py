"""
CPU tests of the batched MCTS-zero deployment planner and the arena gate (planning/vec_mcts_zero.py, planning/mcts_zero/arena.py): the host
restatements against the reference's literal expressions (mcts_zero_mission.py:516-523 replan, :435-436 the gate, arenas.py:38 the
discounted return), the ipp_play struct against a C sizeof / offsetof listing of include/ipp_engine.h, the symbols, and the constructor's
refusals (no GPU here).
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(**over):
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=24, temperature_scale=1.0, temperature_threshold=3, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=40.0, max_episode_steps=6, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    for k, v in over.items():
        (md if k in md else hp)[k] = v
    return hp, md


def _replan_literal(policies, num_actions):
    """mcts_zero_mission.py:516-523 on the workers' dense [A] policies."""
    policy_total = np.zeros(num_actions)
    for i, policy in enumerate(policies):
        policy = np.array(policy)
        policy_total += policy
    policy_total /= np.sum(policy_total)
    return int(np.argmax(policy_total)), policy_total


def _rows(rs, W, K, A, kmax, dyadic):
    """W workers' sparse rows on one ascending valid set of K of A actions, padded to kmax."""
    idx = np.sort(rs.choice(A, size=K, replace=False))
    vi = np.full((W, kmax), -1, dtype=np.int64)
    vi[:, :K] = idx
    pol = np.zeros((W, kmax))
    if dyadic:  # multiples of 1/64: every sum is exact, so equal totals are exact ties
        pol[:, :K] = rs.randint(0, 4, size=(W, K)) / 64.0
        pol[0, 0] += 1 / 64.0  # (mass somewhere)
    else:
        pol[:, :K] = rs.random_sample((W, K))
        pol[:, :K] /= pol[:, :K].sum(axis=1, keepdims=True)
    return pol, vi, idx


@pytest.mark.parametrize("workers", [1, 3, 8])
@pytest.mark.parametrize("dyadic", [False, True])
def test_ensemble_pick_equals_the_literal_replan(workers, dyadic):
    from ipp_rl_amd.planning.vec_mcts_zero import ensemble_pick_host

    rs = np.random.RandomState(10 * workers + int(dyadic))
    A, kmax = 50, 24
    tied = 0
    for trial in range(40):
        K = int(rs.randint(1, kmax + 1))
        pol, vi, idx = _rows(rs, workers, K, A, kmax, dyadic)
        dense = np.zeros((workers, A))
        dense[:, idx] = pol[:, :K]
        want, total = _replan_literal(dense, A)
        got = ensemble_pick_host(pol, vi, np.ones(workers, dtype=np.int32), tie_rule=0, num_actions=A)
        assert got["forced"] == 0 and got["action_idx"] == want
        # (np.sum adds pairwise, the restatement in ascending order: the same bits where every sum is exact, else within the rounding of
        # a sum of A terms, A 2^-53 < 1e-14 relative)
        if dyadic:
            assert np.array_equal(got["ensemble"][:K], total[idx])
        np.testing.assert_allclose(got["ensemble"][:K], total[idx], rtol=1e-14, atol=0)
        assert np.all(got["ensemble"][K:] == 0)
        n_ties = int((total == total.max()).sum())
        tied += n_ties > 1
        # the arena's rule: number floor(u n) of the maxima in ascending action order (mcts.py:134-138 with a given uniform)
        for u in (0.0, 0.49, 0.999999):
            best = np.argwhere(total == np.max(total)).flatten()
            got1 = ensemble_pick_host(pol, vi, np.ones(workers), tie_rule=1, u=u, num_actions=A)
            assert got1["action_idx"] == best[min(int(u * len(best)), len(best) - 1)]
    assert (tied > 0) == dyadic  # (the dyadic rows do hold exact ties, the random ones do not)


def test_ensemble_pick_skips_workers_without_a_policy_and_refuses_rows_without_mass():
    from ipp_rl_amd.planning.vec_mcts_zero import ensemble_pick_host

    rs = np.random.RandomState(3)
    A, kmax, W, K = 30, 8, 3, 5
    pol, vi, idx = _rows(rs, W, K, A, kmax, False)
    ok = np.array([0, 1, 1])
    vi_bad0 = vi.copy()
    vi_bad0[0] = -1  # (the row of a worker without a policy is not looked at)
    dense = np.zeros((2, A))
    dense[:, idx] = pol[1:, :K]
    want, total = _replan_literal(dense, A)
    got = ensemble_pick_host(pol, vi_bad0, ok, num_actions=A)
    assert got["action_idx"] == want
    np.testing.assert_allclose(got["ensemble"][:K], total[idx], rtol=1e-14, atol=0)
    forced = dict(action_idx=-1, forced=1, slot=-1)
    nan, zero, inf = pol.copy(), np.zeros_like(pol), pol.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = np.inf
    big = vi.copy()
    big[:, :K] += A  # every valid index is no action
    for p, v, o in ((pol, vi, np.zeros(W)), (nan, vi, np.ones(W)), (zero, vi, np.ones(W)), (inf, vi, np.ones(W)), (pol, big, np.ones(W)),
                    (pol, np.full_like(vi, -1), np.ones(W))):
        got = ensemble_pick_host(p, v, o, num_actions=A)
        assert {k: got[k] for k in forced} == forced and np.all(got["ensemble"] == 0)


def test_gate_is_the_reference_comparison():
    from ipp_rl_amd.planning.vec_mcts_zero import gate

    for prev, curr, thr in ((10.0, 10.0, 0.5), (10.0, 10.0, 0.52), (9.0, 11.0, 0.55), (9.0, 11.0, 0.56), (11.0, 9.0, 0.45), (11.0, 9.0, 0.44),
                            (1.0, 3.0, 0.75), (3.0, 1.0, 0.25), (0.1, 0.2, 0.2 / (0.1 + 0.2))):
        relative_total_rewards_curr = curr / (prev + curr)  # :435
        rejected = relative_total_rewards_curr < thr        # :436
        accepted, ratio = gate(prev, curr, thr)
        assert ratio == relative_total_rewards_curr and accepted == (not rejected)
    assert gate(10.0, 10.0, 0.5) == (True, 0.5) and gate(10.0, 10.0, 0.52)[0] is False
    assert gate(1.0, 3.0, 0.75)[0] is True  # exactly at the threshold: kept


@pytest.mark.parametrize("T", [0, 1, 7])
def test_tally_is_the_arena_return(T):
    from ipp_rl_amd.planning.vec_mcts_zero import tally_host

    rs = np.random.RandomState(T)
    gamma = 0.9
    rewards = rs.random_sample(T).astype(np.float32)
    total_reward = 0
    for depth in range(T):
        total_reward += gamma ** depth * float(rewards[depth])  # arenas.py:38
    if T == 0:  # a game without a step: the env had no decision at its first step
        out = tally_host([0.25], [0], [1], gamma, 1)
    else:
        out = tally_host(rewards, [0] * (T - 1) + [1], [0] * T, gamma, 1)
    assert out["games"] == 1 and out["game_value"] == [total_reward] and out["game_steps"] == [T]
    assert out["ret"] == 0.0 and out["steps"] == 0
    # a forced step in the middle ends the game without its reward; later games of a retired env are not counted
    if T == 7:
        f = [0, 0, 1, 0, 0, 0, 0]
        d = [0, 0, 0, 0, 1, 0, 1]
        two = tally_host(rewards, d, f, gamma, 2)
        g0 = gamma ** 0 * float(rewards[0]) + gamma ** 1 * float(rewards[1])
        g1 = gamma ** 0 * float(rewards[3]) + gamma ** 1 * float(rewards[4])
        assert two["game_value"] == [g0, g1] and two["game_steps"] == [2, 2] and two["games"] == 2
        one = tally_host(rewards, d, f, gamma, 1)
        assert one["game_value"] == [g0] and one["games"] == 1
        three = tally_host(rewards, d, f, gamma, 3)
        assert three["games"] == 3 and three["game_steps"] == [2, 2, 2]


def test_totals_host_is_the_ordered_sum():
    from ipp_rl_amd.planning.vec_mcts_zero import totals_host

    rs = np.random.RandomState(0)
    gv, gs = rs.random_sample((5, 3)), rs.randint(1, 7, size=(5, 3))
    games = np.array([3, 1, 0, 3, 2])
    want, steps = 0.0, 0
    for e in range(5):
        for g in range(games[e]):
            want += gv[e, g]
            steps += gs[e, g]
    assert np.array_equal(totals_host(gv, gs, games), [want, 9.0, float(steps), 2.0])


C_LISTING = r"""
#include <stddef.h>
#include <stdio.h>
#include "ipp_engine.h"
#define F(name) printf(#name " %zu\n", offsetof(ipp_play, name));
int main(void) {
    printf("sizeof %zu\n", sizeof(ipp_play));
    FIELDS
    return 0;
}
"""


def test_ipp_play_layout_symbols_and_abi(tmp_path):
    from ipp_rl_amd import _ffi

    names = [f[0] for f in _ffi.IppPlay._fields_]
    src = tmp_path / "layout.c"
    src.write_text(C_LISTING.replace("FIELDS", " ".join(f"F({n})" for n in names)))
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    listing = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(listing.pop("sizeof")) == ctypes.sizeof(_ffi.IppPlay) == 192
    assert {n: int(v) for n, v in listing.items()} == {n: getattr(_ffi.IppPlay, n).offset for n in names}
    # every member of the header's struct is mirrored, in order (as tests/test_selfplay_host.py reads ipp_selfplay)
    import re

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    body = re.search(r"typedef struct ipp_play \{(.*?)\} ipp_play;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [n.strip().lstrip("*").strip() for stmt in body.split(";") if stmt.strip()
               for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]
    assert members == names
    lib = _ffi.load()
    for name, n_args in (("ipp_play_pick", 5), ("ipp_play_tally", 2), ("ipp_play_totals", 3)):
        assert hasattr(lib, name) and len(_ffi.PROTOTYPES[name][1]) == n_args
    assert _ffi.ABI_VERSION == 17 and lib.ipp_abi_version() == 17


def test_play_calls_validate_their_arguments_on_the_host():
    """Bad arguments fail through the library's error message, before any launch (no GPU here)."""
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def play(**over):
        pl = _ffi.IppPlay(num_envs=2, workers=1, kmax=8, num_actions=10, games_per_env=1, tie_rule=0, device=0, gamma=0.9, seed=1, row_offset=0)
        for f, _ in _ffi.IppPlay._fields_[11:-1]:
            setattr(pl, f, p)
        for k, v in over.items():
            setattr(pl, k, v)
        return pl

    for over, word in ((dict(workers=0), "workers"), (dict(kmax=2049), "kmax"), (dict(kmax=0), "kmax"), (dict(games_per_env=0), "games_per_env"),
                       (dict(tie_rule=2), "tie_rule"), (dict(tie_rule=-1), "tie_rule"), (dict(ret=None), "null"), (dict(actions=None), "null")):
        pl = play(**over)
        for rc in (lib.ipp_play_pick(ctypes.byref(pl), p, p, p, None), lib.ipp_play_tally(ctypes.byref(pl), None),
                   lib.ipp_play_totals(ctypes.byref(pl), p, None)):
            assert rc == -1 and word in lib.ipp_last_error().decode(), (over, lib.ipp_last_error())
    pl = play()
    assert lib.ipp_play_pick(ctypes.byref(pl), None, p, p, None) == -1 and lib.ipp_play_totals(ctypes.byref(pl), None, None) == -1
    assert lib.ipp_play_pick(None, p, p, p, None) == -1


def _stub_env(B=4, max_batch=4 * 3 * 4, node_capacity=4 * 3 * 40, budget_mode=True, patch=1, dim=40):
    from ipp_rl_amd import EngineConfig

    eng = types.SimpleNamespace(max_batch=max_batch, _c=types.SimpleNamespace(node_capacity=node_capacity),
                                info=types.SimpleNamespace(patch_layout=patch))
    return types.SimpleNamespace(num_envs=B, budget_mode=budget_mode, engine=eng, prev=None,
                                 cfg=EngineConfig(x_dim=dim, y_dim=dim, simulation="split_random_field"))


def test_constructor_refuses_what_it_cannot_run():
    """Each refusal comes before anything touches a device, and names the number that is needed."""
    from ipp_rl_amd.planning import VecMctsZeroPolicy
    from ipp_rl_amd.planning.vec_mcts_zero import check_args, valid_set_width

    hp, md = _params()
    env = _stub_env()
    assert check_args(env, hp, md, 3, "deploy", 1, 4) == (12, 24, valid_set_width(env.cfg, hp, md))
    assert valid_set_width(env.cfg, hp, md) == (2 * 3 + 1) ** 2 * 2
    with pytest.raises(ValueError, match=r"max_batch >= 48"):
        VecMctsZeroPolicy(_stub_env(max_batch=47), hp, md, workers=3)
    with pytest.raises(ValueError, match=r"node_capacity >= 480"):
        VecMctsZeroPolicy(_stub_env(node_capacity=479), hp, md, workers=3)
    with pytest.raises(ValueError, match=r"node_capacity >= 160"):  # workers from hyper_params['num_workers'], 1 without it
        VecMctsZeroPolicy(_stub_env(node_capacity=159), hp, md)
    with pytest.raises(ValueError, match=r"max_batch >= 128"):
        VecMctsZeroPolicy(_stub_env(), dict(hp, num_workers=8), md)
    h, m = _params(max_valid_action_distance=70.0)
    with pytest.raises(ValueError, match=r"at most 2048"):
        VecMctsZeroPolicy(_stub_env(), h, m, workers=3)
    with pytest.raises(ValueError, match="reset_mcts_each_step"):
        VecMctsZeroPolicy(_stub_env(), dict(hp, reset_mcts_each_step=False), md, workers=3)
    for sims in (0, -1):
        with pytest.raises(ValueError, match=r"network-only.*out of scope"):
            VecMctsZeroPolicy(_stub_env(), dict(hp, num_mcts_simulations=sims), md, workers=3)
    with pytest.raises(ValueError, match="mode"):
        VecMctsZeroPolicy(_stub_env(), hp, md, workers=3, mode="train")
    with pytest.raises(ValueError):
        VecMctsZeroPolicy(_stub_env(), hp, md, workers=0)
    with pytest.raises(ValueError):
        VecMctsZeroPolicy(_stub_env(), hp, md, workers=3, games_per_env=0)
    with pytest.raises(ValueError, match="patch-layout"):
        VecMctsZeroPolicy(_stub_env(patch=0), hp, md, workers=3)
    with pytest.raises(TypeError):
        VecMctsZeroPolicy(_stub_env(budget_mode=False), hp, md, workers=3)


def test_arena_refuses_a_game_count_that_does_not_fill_the_envs():
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import Arena

    hp, md = _params()
    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    arena = Arena(cfg, 4, hp, md, None, None)
    for n in (0, 3, 6):
        with pytest.raises(ValueError, match="multiple of num_envs"):
            arena.play_games(n)
    with pytest.raises(ValueError, match="initial_budget"):
        Arena(cfg, 4, hp, dict(md, initial_budget=None), None, None)
