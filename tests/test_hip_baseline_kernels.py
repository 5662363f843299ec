"""
GPU tests of ipp_baseline_act on bare arrays (csrc/k_baselines.h, include/ipp_engine.h): every kind at the smallest shapes at which its
kernel can go wrong, against the host restatements of planning/vec_baselines.py, bit for bit.
"""
import numpy as np
import pytest

from ipp_rl_amd.planning import vec_baselines as vb
from tests.baseline_kernel_helpers import (ALT_HI, ALT_LO, DTB, MAX_A, MAX_V, NUM_WAYPOINTS, RES, SLOPE, SPACING, STEP_SIZE,
                                           baseline_launch)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
DISCRETE, CONTINUOUS, LAWN, SPIRAL = 2, 3, 0, 1
LEVELS = vb.altitude_linspace(ALT_LO, ALT_HI, SPACING)


def check_bookkeeping(out, budget, has, decision0=0):
    assert np.array_equal(out["has"], has.astype(np.uint8))
    assert np.array_equal(out["budget"], np.where(has, budget, 0.0))  # no action: the budget is zeroed, else untouched
    assert np.array_equal(out["decision"], np.full(len(budget), decision0 + 1))


@pytest.mark.parametrize("adaptive", [False, True])
def test_discrete_ranks_in_index_order(adaptive):
    """A = 300 actions (10x10 x 3 levels): neither a multiple of 64 nor of 256.  Envs: count 0, count 1, rank 0, rank count - 1,
    u = 0.999999, u = 1.0 (outside the contract [0, 1): floor(u count) = count is clamped; for u < 1 the fp64 product never reaches count,
    count (1 - 2^-53) rounds down), and a budget cut that bites."""
    actions = vb.discrete_actions(10, 10, RES, LEVELS)
    assert len(actions) == 300
    centre, corner = np.array([18.0, 18.0, 11.0]), np.array([2.0, 2.0, 14.0])
    one = 1.0
    if adaptive:  # flight time of a 3 m climb: 1 m of cruise at 2 m/s + 2 s of ramps = 2.5, exactly
        cases = [(centre, 1.0, 0.3), (np.array([18.0, 18.0, 8.0]), 2.5, 0.7), (corner, 100.0, 0.0), (corner, 100.0, None),
                 (centre, 100.0, 0.999999), (centre, 4.0, one), (corner, 6.5, 0.5)]
    else:
        cases = [(centre, 1.0, 0.3), (np.array([18.0, 18.0, 8.0]), 3.0, 0.7), (centre, 100.0, 0.0), (centre, 100.0, None),
                 (centre, 100.0, 0.999999), (centre, 4.0, one), (corner, 7.0, 0.5)]
    prev = np.stack([c[0] for c in cases])
    budget = np.array([c[1] for c in cases])
    counts = [int(vb.discrete_mask(actions, p, b, adaptive, MAX_V, MAX_A).sum()) for p, b in zip(prev, budget)]
    u = np.array([(counts[i] - 0.5) / counts[i] if c[2] is None else c[2] for i, c in enumerate(cases)])
    assert counts[0] == 0 and counts[1] == 1 and counts[5] > 1 and np.floor(u[5] * counts[5]) == counts[5], counts
    assert np.floor(0.999999 * counts[4]) == counts[4] - 1 and np.floor(np.nextafter(1.0, 0.0) * counts[4]) == counts[4] - 1
    if adaptive:
        assert counts[2] == 299 and counts[6] < counts[2]  # every action but the own one: valid on both sides of every wave and stride boundary
    else:
        assert counts[2] == int(vb.discrete_mask(actions, centre, 11.5, False, MAX_V, MAX_A).sum()) < 299  # the d < 11.5 cut bites at budget 100
        assert counts[6] < int(vb.discrete_mask(actions, corner, 11.5, False, MAX_V, MAX_A).sum())  # ... and the budget cut at 7
    want = [vb.random_discrete_next(actions, prev[i], budget[i], u[i], adaptive, MAX_V, MAX_A) for i in range(len(cases))]
    assert want[2][1] == 0 and want[3][1] == counts[3] - 1 and want[4][1] == counts[4] - 1 and want[5][1] == counts[5] - 1
    out = baseline_launch(DISCRETE, prev, budget, levels=LEVELS, uniforms=u, adaptive=adaptive, decision=np.full(len(cases), 4))
    has = np.array([w[4] for w in want])
    check_bookkeeping(out, budget, has, decision0=4)
    for i, w in enumerate(want):
        assert np.array_equal(out["action"][i], w[3]), (i, out["action"][i], w[3])
    # the picks sit on both sides of a wave (64) and of a stride (256) boundary
    idx = np.array([w[2] for w in want])
    assert idx[has].min() < 64 and idx[has].max() >= 256, idx


@pytest.mark.parametrize("flight", [False, True])
def test_continuous_first_feasible_trial(flight):
    """First feasible trial 0, 63, 64, 100, none, and a negative budget; waypoints bit-identical to low + (high - low) u."""
    low, high = vb.continuous_box(10, 10, RES, DTB, ALT_LO, ALT_HI)
    first = [0, 63, 64, 100, None, 0]
    n = len(first)
    rs = np.random.RandomState(3)
    u = np.empty((n, vb.TRIALS, 3))
    u[..., :2] = 0.8 + 0.19 * rs.random_sample((n, vb.TRIALS, 2))  # far from the corner: not affordable
    u[..., 2] = rs.random_sample((n, vb.TRIALS))
    for e, f in enumerate(first):
        if f is not None:
            u[e, f:, :2] = 0.02 * rs.random_sample((vb.TRIALS - f, 2))  # the first affordable trial and affordable ones behind it
    prev = np.tile(np.array([4.0, 4.0, 11.0]), (n, 1))
    budget = np.array([6.0, 6.0, 6.0, 6.0, 6.0, -1.0])
    want = [vb.random_continuous_next(prev[e], budget[e], u[e], low, high, flight, MAX_V, MAX_A) for e in range(n)]
    assert [w[0] for w in want] == [0, 63, 64, 100, 100, 100] and [w[2] for w in want] == [True, True, True, True, False, False]
    out = baseline_launch(CONTINUOUS, prev, budget, uniforms=u, flight=flight, low=low, high=high)
    check_bookkeeping(out, budget, np.array([w[2] for w in want]))
    for e, w in enumerate(want):
        assert np.array_equal(out["action"][e], w[1]), e
        if w[2]:
            assert np.array_equal(out["action"][e], low + (high - low) * u[e, w[0]])


@pytest.mark.parametrize("flight", [False, True])
def test_table_kinds_rules_and_cursor(flight):
    lawn = vb.lawnmower_table(10, 10, RES, DTB, ALT_LO, ALT_HI, STEP_SIZE, SPACING)
    spiral = vb.spiral_table(10, 10, RES, DTB, ALT_LO, ALT_HI, NUM_WAYPOINTS, SLOPE)
    init = np.array([2.0, 2.0, 14.0])

    def cost(a, b):
        return float(vb.mission_cost(a, b, flight, MAX_V, MAX_A))

    for kind, name, table in ((LAWN, "lawnmower", lawn), (SPIRAL, "spiral", spiral)):
        K = len(table)
        # (cursor, prev, budget, episode, seen): the last row, past the last row, budget == cost, just above it, the first row with a
        # budget below its cost, a small budget, a changed episode entry, an unchanged one
        rows = [(K - 1, table[K - 2], 50.0, 0, 0), (K, table[K - 1], 50.0, 0, 0),
                (5, table[4], cost(table[5], table[4]), 0, 0), (5, table[4], np.nextafter(cost(table[5], table[4]), np.inf), 0, 0),
                (0, init, 0.5 * cost(table[0], init), 0, 0), (3, table[2], 0.75 * STEP_SIZE, 2, 2),
                (7, init, 60.0, 4, 3), (7, table[6], 60.0, 4, 4)]
        cursor = np.array([r[0] for r in rows]); prev = np.stack([r[1] for r in rows]); budget = np.array([r[2] for r in rows])
        episode = np.array([r[3] for r in rows]); seen = np.array([r[4] for r in rows])
        eff = np.where(episode != seen, 0, cursor)
        want = [vb.table_next(name, table, int(eff[i]), prev[i], budget[i], STEP_SIZE, flight, MAX_V, MAX_A) for i in range(len(rows))]
        has = np.array([w[0] for w in want])
        if kind == LAWN:  # budget == cost: no action; a budget below step_size: none although the hop is affordable
            assert list(has) == [True, False, False, budget[3] >= STEP_SIZE, False, False, True, True]
            assert budget[5] > cost(table[3], table[2]) or not flight  # (as a distance every hop of this table is >= step_size)
        else:  # budget - cost == 0: an action; the first waypoint whatever it costs
            assert list(has) == [True, False, True, True, True, True, True, True]
        out = baseline_launch(kind, prev, budget, episode=episode, cursor=cursor, seen=seen, table=table, flight=flight)
        check_bookkeeping(out, budget, has)
        for i, w in enumerate(want):
            assert np.array_equal(out["action"][i], w[1]), (name, i)
        assert np.array_equal(out["cursor"], eff + has), name
        assert np.array_equal(out["seen"], episode)
        assert np.array_equal(out["start"], np.where(episode != seen, budget, -1.0))  # latched on a new episode only
        assert np.array_equal(out["action"][6], table[0]) and out["cursor"][6] == 1  # the changed episode: back to row 0


def test_philox_uniforms_follow_the_convention():
    """uniforms == NULL: u = philox_uniform(512 (env + row_offset), IPP_BASELINE_STREAM + decision, seed); one valid action per rank
    interval tells the uniform apart."""
    actions = vb.discrete_actions(10, 10, RES, LEVELS)
    n, seed, offset = 5, 77, 9
    prev = np.tile(np.array([18.0, 18.0, 11.0]), (n, 1))
    budget = np.full(n, 100.0)
    decision = np.array([0, 1, 2, 3, 40])
    out = baseline_launch(DISCRETE, prev, budget, levels=LEVELS, adaptive=True, decision=decision, seed=seed, row_offset=offset)
    u = vb.baseline_uniform(seed, np.arange(n) + offset, decision)
    for e in range(n):
        w = vb.random_discrete_next(actions, prev[e], budget[e], u[e], True, MAX_V, MAX_A)
        assert np.array_equal(out["action"][e], w[3]), e
    assert len({tuple(a) for a in out["action"]}) > 1
