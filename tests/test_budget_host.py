"""
CPU tests of the budget ledger's host side: the budget.npz fixture's semantics (the reference's episode loop,
planning/mcts_zero/episode_generators.py:109-150, restated as a NumPy ledger), the host copy of the start-budget draw, and the new
flag macros of include/ipp_engine.h against the ctypes binding.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT = np.array([2.0, 2.0, 14.0])
RES, MAX_STEPS = 4.0, 40


def costs(actions, flight_time, vmax=2.0, amax=2.0):
    """action_costs (planning/common/actions.py:8-41) of a sequence that starts from INIT_ACTION."""
    prev = np.vstack([INIT[None], actions[:-1]])
    d = np.sqrt(np.sum((actions - prev) ** 2, axis=1))
    if not flight_time:
        return d
    d_acc = np.minimum(0.5 * d, vmax * vmax / (2 * amax))
    return (d - 2 * d_acc) / vmax + 2 * np.sqrt(2 * d_acc / amax)


def ledger(actions, b0, flight_time):
    """NumPy ledger: remaining budget after every step, and the step after which done is first set."""
    rem = b0 - np.cumsum(costs(actions, flight_time))
    depth = np.arange(1, len(actions) + 1)
    done = ~((depth < MAX_STEPS) & (rem >= RES))
    return rem, int(np.argmax(done)) + 1


def test_fixture_matches_numpy_ledger(golden):
    bud = golden("budget")
    seen = set()
    for name in ("episode_rf1_50_s0", "episode_mixed_50_s1"):
        acts = golden(name)["actions"]
        for mode in ("distance", "flight_time"):
            key = f"{name}__{mode}"
            for j, b0 in enumerate(bud[key + "__budget"]):
                rem, steps = ledger(acts, b0, mode == "flight_time")
                assert np.max(np.abs(rem - bud[key + "__remaining"][j])) <= 1e-9 * b0
                assert steps == int(bud[key + "__steps"][j])
                # away from the threshold: a rounding of the last bit cannot move the end
                assert np.min(np.abs(rem - RES)) > 1e-6 * b0
                seen.add("early" if steps < 15 else "mid" if steps < MAX_STEPS else "never")
    assert seen == {"early", "mid", "never"}


def test_host_philox_known_answers_and_start_budgets():
    from ipp_rl_amd.vec_env import philox_uniform, start_budget

    # Philox4x32-10 known-answer vectors (Salmon et al., SC'11, Random123): first output word
    assert philox_uniform(0, 0, 0) == (0x6627E8D5 + 0.5) / 2 ** 32
    assert philox_uniform(-1, -1, 2 ** 64 - 1) == (0x408F276D + 0.5) / 2 ** 32
    ids = np.arange(10000)
    b = start_budget(200.0, True, 7, ids, 3)
    assert b.min() >= 10 and b.max() < 200 and np.all(b == np.floor(b))
    assert len(np.unique(b)) > 150  # spread over U(10, 200)
    # keyed on (global env id, episode): a shard sees the same numbers
    assert np.array_equal(start_budget(200.0, True, 7, ids[5000:], 3), b[5000:])
    assert not np.array_equal(start_budget(200.0, True, 7, ids, 4), b)
    assert np.all(start_budget(200.0, False, 7, ids, 3) == 200.0)


def test_budget_macros_match_ffi():
    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    for macro, val in (("IPP_BUDGET", _ffi.IPP_BUDGET), ("IPP_RESET_ON_DONE", _ffi.IPP_RESET_ON_DONE),
                       ("IPP_ABI_VERSION", _ffi.ABI_VERSION)):
        m = re.search(rf"#define\s+{macro}\s+(\d+)", txt)
        assert m and int(m.group(1)) == val, macro
    m = re.search(r"#define\s+IPP_BUDGET_STREAM\s+\((\d+)ull\s*<<\s*(\d+)\)", txt)
    assert m and int(m.group(1)) << int(m.group(2)) == _ffi.IPP_BUDGET_STREAM
    flags = [_ffi.IPP_COV_ONLY, _ffi.IPP_PREDICT_ONLY, _ffi.IPP_ADAPTIVE, _ffi.IPP_USE_FLIGHT_TIME, _ffi.IPP_GIVEN_OBSERVATION,
             _ffi.IPP_UPDATE_PREV, _ffi.IPP_BUDGET, _ffi.IPP_RESET_ON_DONE]
    assert sum(flags) == 255 and len(set(flags)) == 8  # distinct bits
    for name in ("ipp_set_budget", "ipp_generate_grf_refill"):
        assert name in _ffi.PROTOTYPES


def test_budget_mode_arguments_are_checked_before_any_engine():
    """The constructor refuses what budget mode cannot run before it builds an engine (no GPU needed to see that)."""
    import pytest
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=50, y_dim=50)
    for kw in (dict(shuffle_prior_cov=True), dict(state="dense"), dict(budget=3.0), dict(budget=None, shuffle_budget=True),
               dict(budget=8.0, shuffle_budget=True)):
        args = dict(budget=100.0)
        args.update(kw)
        with pytest.raises(ValueError):
            VecIPPEnv(cfg, 8, episode_steps=4, device="cpu", **args)
    with pytest.raises(ValueError):
        VecIPPEnv(EngineConfig(x_dim=40, y_dim=40), 8, episode_steps=4, device="cpu", budget=100.0)
