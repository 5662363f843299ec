"""
CPU-only checks of the batched self-play's host restatements (planning/mcts_zero/selfplay.py) against literal transcriptions of the
reference: the windowed value targets with the absolute-step exponent (episode_generators.py:158-164), the random shift of the replay
buffer (ReplicationPad2d(4) + RandomCrop, replay_buffers.py:58-75), the inverse-CDF action draw and the first-waypoint draw on the host
Philox, and the constructor's refusals.
"""
import numpy as np
import pytest


def _reference_targets(rewards, gamma, episode_horizon):
    """episode_generators.py:158-164, transcribed."""
    total_episode_value = sum([gamma ** j * rewards[j] for j in range(len(rewards))])
    values = []
    for i, reward in enumerate(rewards):
        bootstrapped_idx = min(i + episode_horizon, len(rewards))
        value = sum([gamma ** j * rewards[j] for j in range(i, bootstrapped_idx)])
        values.append(np.sqrt(1 + value) - 1)
    return values, total_episode_value


@pytest.mark.parametrize("gamma,horizon,T", [(0.9, 5, 17), (0.5, 3, 1), (0.97, 40, 40), (1.0, 5, 12)])
def test_value_targets_match_the_reference_transcription(gamma, horizon, T):
    from ipp_rl_amd.planning.mcts_zero.selfplay import value_targets

    rs = np.random.RandomState(T)
    rewards = list(rs.uniform(0, 3, T))
    want, want_tot = _reference_targets(rewards, gamma, horizon)
    got, tot = value_targets(rewards, gamma, horizon)
    assert np.array_equal(got, np.array(want)) and tot == want_tot
    if gamma != 1.0 and T > 1:
        # the exponent is the ABSOLUTE step: a discount relative to i gives other targets beyond the first sample
        rel = [np.sqrt(1 + sum(gamma ** (j - i) * rewards[j] for j in range(i, min(i + horizon, T)))) - 1 for i in range(T)]
        assert got[0] == rel[0] and not np.allclose(got[1:], rel[1:])


def test_shift_equals_replicate_pad_and_crop():
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import replay_draws, shift_planes

    rs = np.random.RandomState(3)
    states = rs.standard_normal((5, 3, 12, 12)).astype(np.float32)
    rows, offs = replay_draws(5, 4, seed=11, draw=2, committed_rows=np.arange(40))
    assert offs.shape == (4, 2) and tuple(offs[0]) == (4, 4) and offs.min() >= 0 and offs.max() <= 8
    assert rows.min() >= 0 and rows.max() < 40
    padded = torch.nn.functional.pad(torch.from_numpy(states), (4, 4, 4, 4), mode="replicate")
    for i in range(9):
        for j in range(9):
            want = padded[..., i:i + 12, j:j + 12].numpy()  # RandomCrop((12, 12)) at (i, j): one offset for the whole 4-D batch
            assert np.array_equal(shift_planes(states, (i, j)), want)
    assert np.array_equal(shift_planes(states, (4, 4)), states)
    # the offsets of the copies are spread over [0, 8]^2
    _, many = replay_draws(1, 400, seed=5, draw=0, committed_rows=np.arange(3))
    assert len(np.unique(many[1:, 0])) == 9 and len(np.unique(many[1:, 1])) == 9


def test_inverse_cdf_and_init_draws_on_the_host_philox():
    from ipp_rl_amd.planning.mcts_zero.selfplay import (ACTION_STREAM, INIT_STREAM, init_action_index, inverse_cdf, step_counter,
                                                        step_uniform)
    from ipp_rl_amd.vec_env import philox_uniform

    rs = np.random.RandomState(0)
    for _ in range(200):
        p = rs.uniform(0, 1, 30) * (rs.uniform(0, 1, 30) < 0.5)
        if p.sum() == 0:
            continue
        p = p / p.sum()
        u = rs.random_sample()
        # np.random.choice(len(p), p=p) with u as its uniform (mtrand.choice: cdf = cumsum(p) / sum, searchsorted right)
        cdf = p.cumsum()
        cdf /= cdf[-1]
        want = int(cdf.searchsorted(u, side="right"))
        assert inverse_cdf(p, u) == want and p[want] > 0
    gid, epi, depth = np.arange(100, 164), 3, 7
    u = step_uniform(ACTION_STREAM, 9, gid, epi, depth)
    assert np.array_equal(u, philox_uniform((gid << 20) + depth, ACTION_STREAM + epi, 9))
    assert np.array_equal(step_counter(gid, depth), (gid << 20) + depth)
    a0 = init_action_index(9, gid, epi, 200)
    assert np.array_equal(a0, np.minimum((philox_uniform(gid, INIT_STREAM + epi, 9) * 200).astype(np.int64), 199))
    big = init_action_index(9, np.arange(20000), 0, 200)
    counts = np.bincount(big, minlength=200)
    assert counts.min() > 50 and counts.max() < 160  # uniform over the action set
    # keyed on the global env id: a shard's envs draw the same numbers
    assert np.array_equal(init_action_index(9, gid[32:], epi, 200), a0[32:])


def test_streams_do_not_collide():
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning.mcts_zero import selfplay as sp
    from ipp_rl_amd.vec_env import VecIPPEnv

    bases = [VecIPPEnv.GT_STREAM, VecIPPEnv.NOISE_STREAM, _ffi.IPP_BUDGET_STREAM, sp.ACTION_STREAM, sp.INIT_STREAM, sp.TIE_STREAM,
             sp.ARGMAX_STREAM, sp.REPLAY_STREAM]
    assert len(set(bases)) == len(bases) and all(b % (1 << 40) == 0 for b in bases)


def test_selfplay_macros_and_prototypes_match_ffi():
    import os
    import re

    from ipp_rl_amd import _ffi

    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ipp_engine.h")).read()
    for macro, val in (("IPP_SP_ACTION_STREAM", _ffi.IPP_SP_ACTION_STREAM), ("IPP_SP_INIT_STREAM", _ffi.IPP_SP_INIT_STREAM),
                       ("IPP_SP_TIE_STREAM", _ffi.IPP_SP_TIE_STREAM), ("IPP_SP_ARGMAX_STREAM", _ffi.IPP_SP_ARGMAX_STREAM),
                       ("IPP_REPLAY_STREAM", _ffi.IPP_REPLAY_STREAM)):
        m = re.search(rf"#define\s+{macro}\s+\((\d+)ull\s*<<\s*(\d+)\)", txt)
        assert m and int(m.group(1)) << int(m.group(2)) == val, macro
    body = re.search(r"typedef struct ipp_selfplay \{(.*?)\} ipp_selfplay;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*").strip() for stmt in body.split(";") if stmt.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]
    assert names == [f[0] for f in _ffi.IppSelfPlay._fields_]
    for name in ("ipp_selfplay_record", "ipp_selfplay_commit", "ipp_replay_gather"):
        assert name in _ffi.PROTOTYPES
    assert _ffi.ABI_VERSION == 17


def _params(**over):
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=11.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=8, temperature_scale=1.0, temperature_threshold=40, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=60.0, max_episode_steps=6, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    for k, v in over.items():
        (md if k in md else hp)[k] = v
    return hp, md


def test_constructor_refuses_what_it_cannot_run():
    """Each refusal comes before anything touches a device (no GPU here)."""
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import SelfPlay
    from ipp_rl_amd.planning.mcts_zero.selfplay import check_args

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    hp, md = _params()
    assert check_args(hp, md, 4, None) == (7, 6)
    assert check_args(hp, md, 4, 40) == (10, 6)
    for bad in (dict(initial_budget=None), dict(reset_mcts_each_step=False), dict(use_per=True), dict(shuffle_prior_cov=True)):
        h, m = _params(**bad)
        with pytest.raises(ValueError):
            SelfPlay(cfg, 4, h, m)
    with pytest.raises(ValueError):
        SelfPlay(cfg, 4, hp, md, capacity=4 * 6)  # 6 step slots < max_episode_steps + 1
    with pytest.raises(ValueError):
        SelfPlay(cfg, 4, hp, md, capacity=4 * 7 + 1)  # not a multiple of num_envs
