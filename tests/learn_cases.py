"""
Shared cases of tests/test_learn_host.py (CPU) and tests/test_hip_learn_kernels.py (GPU): the iteration state in front of an
ipp_selfplay_commit_iter on the bare rings of tests/selfplay_cases.py (build_commit), and inputs of the totals and the windowed reset.

The module imports neither torch nor the package at import time.
"""
import numpy as np

from tests import selfplay_cases as sc

CAP = 3                  # episode_cap of the commit cases
ITERATION = 5
HORIZON = 3
# (T, step): episodes of 0 .. T samples on a ring of T + 1 slots; T in {0, 1, horizon, horizon + 1}.  build_commit has envs of T, T // 2,
# T - 1, 1 and 0 samples, ended by done, forced, or running on; T = 0 is its env 10 in every case and every env of the (1, ..)
# case's "half" / "T-1" kinds has at least one row
COMMIT_CASES = ((1, 1), (1, 5), (HORIZON, HORIZON), (HORIZON, 2 * (HORIZON + 1) + 1), (HORIZON + 1, HORIZON + 1),
                (HORIZON + 1, 2 * (HORIZON + 2) + 2))
ITER_EPISODES = (0, CAP - 1, CAP)   # per env in turn, shifted per case so that every kind of env meets every count


def iter_state(state, shift=0, rng=0):
    """The iteration arrays in front of a commit: counters per env in turn (0, cap - 1, cap), recognisable tags, sums of mixed magnitude."""
    B, cap = state["B"], state["B"] * state["S"]
    rs = np.random.RandomState(100 + rng)
    return dict(iteration=ITERATION, episode_cap=CAP,
                iter_episodes=np.array([ITER_EPISODES[(e + shift) % 3] for e in range(B)], np.int32),
                r_iter=rs.randint(-1, ITERATION, cap).astype(np.int32),
                examples=rs.randint(0, 1000, B).astype(np.int64),
                value_sum=rs.uniform(0, 3, B) * 10.0 ** rs.randint(-8, 8, B))


def build(T, step, shift=0):
    """(state, episodes, it) of a commit_iter case."""
    state, episodes = sc.build_commit(T, HORIZON, 0.97, step, random_init=(T + step) % 2, rng=7)
    return state, episodes, iter_state(state, shift=shift, rng=T + step)


TOTALS_B = (1, 63, 64, 65, 300)


def totals_inputs(B):
    """(iter_episodes, examples, value_sum, cap): value sums from 1e-9 to 1e9 with both signs, so that the order of the additions shows."""
    rs = np.random.RandomState(40 + B)
    return (rs.randint(0, 2 * CAP + 1, B).astype(np.int32), rs.randint(0, 1 << 40, B).astype(np.int64),
            rs.uniform(-1, 1, B) * 10.0 ** rs.randint(-9, 10, B), CAP)


WINDOW_CAPS = (1, 255, 256, 257)
WINDOWS = {"empty": (7, 9), "partial": (1, 2), "full": (0, 3), "one": (2, 2)}   # tags are -1 .. 3


def window_inputs(cap):
    """(flags, r_iter): every flag with every tag; committed rows inside each window (but the empty one) whenever cap > 1."""
    rs = np.random.RandomState(60 + cap)
    flags = rs.randint(0, 3, cap).astype(np.uint8)
    tags = rs.randint(-1, 4, cap).astype(np.int32)
    if cap == 1:
        flags[0], tags[0] = sc.COMMITTED, 2
    else:
        flags[:5], tags[:5] = sc.COMMITTED, (0, 1, 2, 3, -1)
        flags[5:8], tags[5:8] = sc.PENDING, (1, 2, 2)   # rows re-opened inside the window
        flags[cap - 1], tags[cap - 1] = sc.COMMITTED, 2
    return flags, tags
