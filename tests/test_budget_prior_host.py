"""
CPU tests of the per-episode priors of budget mode (shuffle_prior_cov="device"): the draw's host restatement (vec_env.start_prior,
prior_from_uniform) against NumPy's own uniform(low, high) -- the reference's draw, mapping/mappings.py:238-240, sigma^2 before l --,
the refusals that come before any device call, and the two new entry points and IPP_PRIOR_STREAM of include/ipp_engine.h against the
ctypes binding.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_formula_is_numpys_uniform_bit_for_bit():
    """NumPy's legacy uniform(low, high) is low + (high - low) u exactly: the host formula applied to the generator's own u gives the
    generator's own value, for both nominals and in the order sigma^2, l."""
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import prior_from_uniform

    cfg = EngineConfig(x_dim=40, y_dim=40)
    for nominals in ((cfg.signal_variance, cfg.length_scale), (0.37, 11.3)):
        for s in range(5):
            a, b = np.random.RandomState(s), np.random.RandomState(s)
            for nominal in nominals:  # sigma^2 first
                u = a.random_sample()
                want = b.uniform(0.8 * nominal, 1.2 * nominal)
                got = prior_from_uniform(nominal, u)
                assert np.float64(got).tobytes() == np.float64(want).tobytes(), (s, nominal, float(got), want)


def test_start_prior_ranges_keys_and_streams():
    from ipp_rl_amd import EngineConfig, _ffi
    from ipp_rl_amd.vec_env import philox_uniform, prior_from_uniform, start_prior

    cfg = EngineConfig(x_dim=40, y_dim=40)
    ids = np.arange(4096)
    p = start_prior(cfg, 7, ids, 3)
    assert p.shape == (4096, 2) and p.dtype == np.float64
    for d, nominal in enumerate((cfg.signal_variance, cfg.length_scale)):
        assert p[:, d].min() >= 0.8 * nominal and p[:, d].max() <= 1.2 * nominal
        assert p[:, d].max() - p[:, d].min() > 0.39 * nominal      # spread over U(0.8, 1.2)
        assert len(np.unique(p[:, d])) > 4000                      # differ between envs
    assert np.all(p[:, 0] / cfg.signal_variance != p[:, 1] / cfg.length_scale)  # two draws, not one
    # the definition: counters 2 g and 2 g + 1 of subsequence IPP_PRIOR_STREAM + episode
    for d, nominal in enumerate((cfg.signal_variance, cfg.length_scale)):
        u = philox_uniform(2 * ids + d, _ffi.IPP_PRIOR_STREAM + 3, 7)
        assert np.array_equal(p[:, d], prior_from_uniform(nominal, u))
    # ... differ between episodes and seeds
    assert not np.any(start_prior(cfg, 7, ids, 4) == p)
    assert not np.any(start_prior(cfg, 8, ids, 3) == p)
    # a per-env episode array
    epi = ids % 5
    q = start_prior(cfg, 7, ids, epi)
    for e in range(5):
        assert np.array_equal(q[epi == e], start_prior(cfg, 7, ids[epi == e], e))
    # keyed on the GLOBAL env id (env id + offset): shards agree
    assert np.array_equal(start_prior(cfg, 7, np.arange(1000) + 3096, 3), p[3096:])
    # not the start budget's uniforms for the same (env, episode)
    ub = philox_uniform(ids, _ffi.IPP_BUDGET_STREAM + 3, 7)
    for d in range(2):
        assert not np.any(philox_uniform(2 * ids + d, _ffi.IPP_PRIOR_STREAM + 3, 7) == ub)
    bases = [1 << 40, 2 << 40, _ffi.IPP_BUDGET_STREAM, _ffi.IPP_SP_ACTION_STREAM, _ffi.IPP_SP_INIT_STREAM, _ffi.IPP_SP_TIE_STREAM,
             _ffi.IPP_SP_ARGMAX_STREAM, _ffi.IPP_REPLAY_STREAM, _ffi.IPP_CMA_STREAM, _ffi.IPP_BASELINE_STREAM]
    assert _ffi.IPP_PRIOR_STREAM == 11 << 40 and _ffi.IPP_PRIOR_STREAM not in bases


def test_refusals_come_before_any_device_call():
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import SelfPlay
    from ipp_rl_amd.planning.mcts_zero.selfplay import check_args
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    with pytest.raises(ValueError, match="budget"):  # "device" is budget mode's
        VecIPPEnv(cfg, 8, episode_steps=4, device="cpu", shuffle_prior_cov="device")
    with pytest.raises(ValueError):  # no other string
        VecIPPEnv(cfg, 8, episode_steps=4, device="cpu", budget=100.0, shuffle_prior_cov="host")
    with pytest.raises(ValueError, match="'device'"):  # True keeps raising in budget mode, and names the opt-in
        VecIPPEnv(cfg, 8, episode_steps=4, device="cpu", budget=100.0, shuffle_prior_cov=True)
    hp, md = _params()
    hs, ms = _params(shuffle_prior_cov=True)
    with pytest.raises(ValueError):
        SelfPlay(cfg, 4, hs, ms, episode_priors="host")
    with pytest.raises(ValueError):
        SelfPlay(cfg, 4, hp, md, episode_priors=True)
    with pytest.raises(ValueError, match="episode_priors"):  # without the opt-in the refusal stays, and names it
        check_args(hs, ms, 4, None)
    assert check_args(hs, ms, 4, None, episode_priors="device") == check_args(hp, md, 4, None) == (7, 6)
    assert check_args(hp, md, 4, 40, episode_priors="device") == (10, 6)


def test_header_and_binding_agree():
    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    m = re.search(r"#define\s+IPP_PRIOR_STREAM\s+\((\d+)ull\s*<<\s*(\d+)\)", txt)
    assert m and int(m.group(1)) << int(m.group(2)) == _ffi.IPP_PRIOR_STREAM
    assert re.search(r"int\s+ipp_set_budget_prior\(void\*\s*engine,\s*int32_t\s+shuffle_prior\);", txt)
    assert re.search(r"int\s+ipp_read_prior\(void\*\s*engine,\s*const int32_t\*\s*env_ids,\s*int32_t\s+n,\s*double\*\s*out[^,]*,\s*void\*\s*stream\);", txt)
    import ctypes as C

    assert _ffi.PROTOTYPES["ipp_set_budget_prior"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert _ffi.PROTOTYPES["ipp_read_prior"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
    assert int(re.search(r"#define\s+IPP_ABI_VERSION\s+(\d+)", txt).group(1)) == _ffi.ABI_VERSION == 17
