"""
Host side of the batched greedy planner (planning/vec_greedy.py, ipp_score_actions_envs): the binding and the header agree, and the
host restatements of the candidate order, the radius table, the budget filter and the first-maximiser rule.  No GPU.
"""
import os
import re

import numpy as np
import pytest

from ipp_rl_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipp_score_actions_envs", "ipp_score_actions_envs_scratch_bytes")


def test_prototypes_match_header():
    assert _ffi.ABI_VERSION == 17
    text = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert name in _ffi.PROTOTYPES
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_args == len(_ffi.PROTOTYPES[name][1]), (name, n_args)
    assert "#define IPP_ABI_VERSION 17" in open(os.path.join(ROOT, "include", "ipp_engine.h")).read()


class _Grid:
    def __init__(self, x_dim, y_dim, resolution):
        self.x_dim, self.y_dim, self.resolution = x_dim, y_dim, resolution
        self.num_grid_cells = x_dim * y_dim


def test_candidate_table_is_get_actions_order():
    from ipp_rl_amd.planning.common.actions import get_actions
    from ipp_rl_amd.planning.vec_greedy import candidate_table

    table = candidate_table(10, 10, 4.0, 8.0, 14.0, 6.0)
    assert table.shape == (200, 3)
    prev = np.array([2.0, 2.0, 14.0])
    want = np.array(get_actions(prev, 1e9, _Grid(10, 10, 4.0), 8.0, 14.0, 6.0, None))
    # get_actions drops the waypoint itself (cost 0): the table with that row removed is the list, in order
    keep = np.linalg.norm(table - prev, axis=1) > 0
    assert keep.sum() == 199
    assert np.array_equal(table[keep], want)
    # row, column, level
    assert np.array_equal(table[0], [2.0, 2.0, 8.0]) and np.array_equal(table[1], [2.0, 2.0, 14.0])
    assert np.array_equal(table[2], [6.0, 2.0, 8.0]) and np.array_equal(table[20], [2.0, 6.0, 8.0])


@pytest.mark.parametrize("position", [(2.0, 2.0, 14.0), (22.0, 18.0, 8.0), (38.0, 38.0, 14.0), (21.0, 17.5, 11.0)])
def test_radius_table_is_brute_force_filter(position):
    from ipp_rl_amd.planning.vec_greedy import candidate_table, radius_candidates

    radius = 13.0
    position = np.array(position)
    table = candidate_table(10, 10, 4.0, 8.0, 14.0, 6.0)
    want = table[np.linalg.norm(table - position, axis=1) < radius]  # mcts_mission.py:169-173
    got = radius_candidates(position, 10, 10, 4.0, 8.0, 14.0, 6.0, radius)
    assert got.shape == ((2 * 4 + 1) ** 2 * 2, 3)
    rows = got[~np.isnan(got).any(axis=1)]
    assert len(want) > 0 and np.array_equal(rows, want)


def test_budget_filter_and_first_maximiser():
    from ipp_rl_amd.planning.vec_greedy import budget_filter, first_maximiser

    cost = np.array([[0.0, 1.0, 2.0, 3.0, np.nan, 5.0],
                     [4.0, 4.0, 4.0, 4.0, 4.0, 4.0],
                     [1.0, 2.0, 3.0, 1.0, 2.0, 3.0]])
    budget = np.array([3.0, 3.5, 10.0])
    valid = budget_filter(cost, budget)
    assert np.array_equal(valid, [[False, True, True, True, False, False], [False] * 6, [True] * 6])
    reward = np.array([[9.0, 0.5, 0.7, 0.7, 8.0, 7.0],     # the cost-0, the NaN-cost and the too-expensive candidates never win
                       [1.0, 2.0, 3.0, 4.0, 5.0, 6.0],     # nothing reachable
                       [0.25, np.nan, 0.5, 0.5, 0.5, 0.1]])  # ties: the first one; a NaN reward never wins
    idx, has = first_maximiser(reward, valid)
    assert np.array_equal(has, [True, False, True])
    assert np.array_equal(idx, [2, 0, 2])
    # all rewards equal: the first valid candidate
    idx, has = first_maximiser(np.zeros((1, 4)), np.array([[False, False, True, True]]))
    assert idx[0] == 2 and has[0]


def test_policy_argument_checks():
    from ipp_rl_amd.planning import VecGreedyPolicy

    class FakeEnv:
        prev = None
        cfg = None

        def score_actions(self, *a, **k):
            raise AssertionError("not called")

    with pytest.raises(ValueError):
        VecGreedyPolicy(FakeEnv(), 8.0, 14.0, 0.0)
    with pytest.raises(ValueError):
        VecGreedyPolicy(FakeEnv(), 14.0, 8.0, 6.0)
    with pytest.raises(ValueError):
        VecGreedyPolicy(FakeEnv(), 8.0, 14.0, 6.0, radius=-1.0)
    with pytest.raises(TypeError):
        VecGreedyPolicy(object(), 8.0, 14.0, 6.0)
