"""
CPU-only checks of the prioritised replay's host restatements (planning/mcts_zero/selfplay.py: per_mass, per_probabilities, per_rows,
per_weights, per_beta_step, per_update) against tests/golden/per.npz, recorded from the reference's PrioritizedExperienceReplayBuffer
(replay_buffers.py:104-141; tests/golden/gen_per_golden.py) over six iterations of sample -> update -> step per case: the indices from
the recorded uniforms exactly, the float32 weights to 1e-7, beta to 1e-15, the priorities after each update exactly (minibatches that
repeat an index included).  And the C ABI: the header and the ctypes binding both declare the prioritised-replay entry points.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ipp_replay_priority_reset", "ipp_replay_mass", "ipp_replay_draw_per", "ipp_replay_gather_rows",
                "ipp_replay_priority_update")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "per.npz"))


def _cases(g):
    return sorted(int(k[1:-5]) for k in g.files if k.endswith("_meta"))


def test_fixture_covers_the_cases(golden):
    metas = {tuple(golden[f"c{c}_meta"][:5]) for c in _cases(golden)}
    assert metas == {(L, b, 0.75, beta0, 3.0) for (L, b) in ((7, 4), (64, 32), (300, 32)) for beta0 in (0.4, 0.5)}
    repeats = sum(len(row) - len(np.unique(row)) for c in _cases(golden) for row in golden[f"c{c}_indices"])
    assert repeats > 0  # (the last-occurrence-wins update is exercised)
    for c in _cases(golden):
        assert golden[f"c{c}_u"].shape[0] == 6 and golden[f"c{c}_weights"].dtype == np.float32


def test_host_restatements_reproduce_the_reference(golden):
    from ipp_rl_amd.planning.mcts_zero.selfplay import per_beta_step, per_mass, per_rows, per_update, per_weights

    for c in _cases(golden):
        L, batch, alpha, beta0, epochs, total_steps = golden[f"c{c}_meta"]
        L, batch, total_steps = int(L), int(batch), int(total_steps)
        assert total_steps == (L // max(1, batch)) * int(epochs)
        pri = np.ones(L) / L
        beta = beta0
        committed = np.ones(L, dtype=bool)
        for t in range(6):
            mass = per_mass(pri, committed, alpha)
            rows = per_rows(mass, golden[f"c{c}_u"][t])
            assert np.array_equal(rows, golden[f"c{c}_indices"][t]), (c, t)
            w = per_weights(mass, rows, L, beta)
            assert w.dtype == np.float32 and w.max() == 1.0 and np.all(w > 0)
            np.testing.assert_allclose(w, golden[f"c{c}_weights"][t], rtol=0, atol=1e-7)
            assert abs(beta - golden[f"c{c}_beta"][t]) <= 1e-15
            pri = per_update(pri, rows, golden[f"c{c}_values"][t])
            assert np.array_equal(pri, golden[f"c{c}_priorities"][t]), (c, t)
            beta = per_beta_step(beta, beta0, total_steps)
            assert abs(beta - golden[f"c{c}_beta_next"][t]) <= 1e-15 and beta <= 1.0


def test_mass_and_rows_edge_cases():
    from ipp_rl_amd.planning.mcts_zero.selfplay import per_mass, per_probabilities, per_rows, per_update, per_weights

    pri = np.array([0.5, 0.0, -1.0, np.nan, np.inf, 2.0, 3.0])
    committed = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)
    mass = per_mass(pri, committed, 0.75)
    assert np.array_equal(mass, [0.5 ** 0.75, 0, 0, 0, 0, 0, 3.0 ** 0.75])  # (0, negative, NaN, inf and uncommitted rows: no mass)
    p = per_probabilities(mass)
    assert abs(p.sum() - 1) < 1e-15
    u = np.array([0.0, p[0] - 1e-12, p[0] + 1e-12, 1 - 2.0 ** -33])
    assert np.array_equal(per_rows(mass, u), [0, 0, 6, 6])
    assert np.array_equal(per_rows(np.zeros(5), [0.3, 0.9]), [-1, -1])
    assert np.all(np.isnan(per_weights(mass, [-1, -1], 2, 0.5)))
    assert np.array_equal(per_weights(mass, [0, 6, 0], 2, 0.0), np.ones(3, np.float32))  # (beta = 0: all ones)
    out = per_update(np.zeros(4), [2, -1, 2, 0, 2], [1.0, 9.0, 2.0, 5.0, 3.0])
    assert np.array_equal(out, [5.0, 0.0, 3.0, 0.0])  # (the last of the repeated index 2 wins, -1 is skipped)


def test_uniforms_are_the_uniform_samplers():
    from ipp_rl_amd.planning.mcts_zero.selfplay import per_uniforms, replay_draws

    u = per_uniforms(16, seed=11, draw=3)
    rows, _ = replay_draws(16, 1, seed=11, draw=3, committed_rows=np.arange(1000))
    assert np.array_equal(rows, np.minimum((u * 1000).astype(np.int64), 999))


def test_entry_points_declared_in_header_and_binding():
    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(rf"\bint {name}\s*\(\s*const ipp_selfplay\*\s*sp\b([^;]*)\);", code)
        assert m, f"{name} is not declared in include/ipp_engine.h"
        assert name in _ffi.PROTOTYPES
        res, args = _ffi.PROTOTYPES[name]
        assert len(args) == m.group(0).count(",") + 1, name  # (one ctypes argument per declared parameter)
    m = re.search(r"#define\s+IPP_REPLAY_SCAN_TILE\s+(\d+)", txt)
    assert m and int(m.group(1)) == _ffi.IPP_REPLAY_SCAN_TILE
    assert int(re.search(r"#define\s+IPP_ABI_VERSION\s+(\d+)", txt).group(1)) == _ffi.ABI_VERSION == 17


def test_prioritized_is_public_and_the_loop_points_to_it():
    from ipp_rl_amd.planning.mcts_zero import PrioritizedReplay, ReplayBuffer
    from ipp_rl_amd.planning.mcts_zero.selfplay import check_args

    assert callable(ReplayBuffer.prioritized) and PrioritizedReplay.sample and PrioritizedReplay.update and PrioritizedReplay.step
    hp = dict(reset_mcts_each_step=True, use_per=True, shuffle_prior_cov=False)
    with pytest.raises(ValueError, match="ReplayBuffer.prioritized"):
        check_args(hp, dict(initial_budget=40.0, max_episode_steps=6), 4, None)
