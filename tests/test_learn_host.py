"""
CPU tests of the learn loop's host side (planning/mcts_zero/learn.py, the iteration restatements of planning/mcts_zero/selfplay.py):
  * exploration_schedule / off_policy_window_size against the reference's formulas (mcts_zero_mission.py:231-252) on config/example.yaml's
    values;
  * commit_iter_host, iter_totals_host and window_rows_host -- the oracles of tests/test_hip_learn_kernels.py -- on hand-made rings:
    cap reached, over-cap dropped, T = 0, forced end; against tests/selfplay_cases.commit_ref wherever the iteration rule changes nothing;
  * header and _ffi agree on ipp_selfplay_iter and the three new prototypes;
  * what the Learner refuses before it touches a device.
"""
import os
import re

import numpy as np
import pytest

from tests import learn_cases as lc
from tests import selfplay_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = dict(puct_init=15, puct_init_decay=0.8, puct_init_min=4, dirichlet_alpha=1.0, dirichlet_alpha_decay=0.8, dirichlet_alpha_min=0.3,
               start_train_examples_history=1, train_examples_history_step=2, max_train_examples_history=10)


def test_exploration_schedule_of_example_yaml():
    from ipp_rl_amd.planning.mcts_zero.learn import exploration_schedule

    hp = dict(EXAMPLE)
    puct, alpha = [], []
    for i in range(8):  # (applied once per iteration, written back as the reference does)
        hp["puct_init"], hp["dirichlet_alpha"] = exploration_schedule(hp, i)
        puct.append(hp["puct_init"])
        alpha.append(hp["dirichlet_alpha"])
    np.testing.assert_allclose(puct, [15, 12, 9.6, 7.68, 6.144, 4.9152, 4, 4], rtol=1e-14, atol=0)
    np.testing.assert_allclose(alpha, [1, 0.8, 0.64, 0.512, 0.4096, 0.32768, 0.3, 0.3], rtol=1e-14, atol=0)
    assert puct[6:] == [4, 4] and alpha[6:] == [0.3, 0.3]  # (the minima themselves, then constant)
    assert exploration_schedule(hp, 8) == (4, 0.3)
    assert exploration_schedule(EXAMPLE, 0) == (15, 1.0) and EXAMPLE["puct_init"] == 15  # (iteration 0 keeps them; nothing is written)


def test_off_policy_window_size_of_example_yaml():
    from ipp_rl_amd.planning.mcts_zero.learn import off_policy_window_size

    got = [off_policy_window_size(EXAMPLE, i) for i in range(21)]
    assert got == [min(int(1 + i / 2), 10) for i in range(21)]
    assert got[:5] == [1, 1, 2, 2, 3] and got[18:] == [10, 10, 10]


# ---------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("T,step", lc.COMMIT_CASES)
def test_commit_iter_host_on_hand_made_rings(T, step, shift):
    from ipp_rl_amd.planning.mcts_zero.selfplay import commit_iter_host, value_targets

    state, episodes, it = lc.build(T, step, shift)
    B, S = state["B"], state["S"]
    ref = sc.commit_ref(state, step)
    got = commit_iter_host(state, step, it)
    # what the iteration rule leaves alone is the plain commit's
    for k in ("r_reward", "ep_len", "prev", "episode_value", "forced", "tie_u"):
        assert np.array_equal(sc.bits(got[k]), sc.bits(ref[k])), k
    want = {k: np.array(it[k]) for k in ("iter_episodes", "r_iter", "examples", "value_sum")}
    want["r_value"], want["r_flags"] = state["r_value"].copy(), state["r_flags"].copy()
    kinds = set()
    for e, (Te, kind) in enumerate(episodes):
        if kind == "on":
            continue
        rows = sc.episode_rows(step, Te, kind == "forced", S, B, e)
        before = int(it["iter_episodes"][e])
        want["iter_episodes"][e] = before + 1      # counted whether kept or not, with T = 0 too
        kinds.add((Te == 0, kind, before))
        if before < lc.CAP:
            vals, tot = value_targets(ref["r_reward"][rows], state["gamma"], state["horizon"])
            want["r_value"][rows], want["r_flags"][rows], want["r_iter"][rows] = vals, sc.COMMITTED, lc.ITERATION
            want["examples"][e] += Te
            want["value_sum"][e] += tot
            assert np.array_equal(sc.bits(got["r_value"][rows]), sc.bits(ref["r_value"][rows]))  # (a kept episode: the plain commit's targets)
        else:
            want["r_flags"][rows] = 0              # dropped: no sample, targets and tags untouched
    for k, v in want.items():
        assert np.array_equal(sc.bits(got[k]), sc.bits(v)), k
    assert any(b == lc.CAP - 1 for _, _, b in kinds) and any(b == lc.CAP for _, _, b in kinds)  # cap reached, past the cap
    assert any(k == "forced" for _, k, _ in kinds) and any(z for z, _, _ in kinds)               # forced end, T = 0


def test_scan_order_sum_and_totals_host():
    from ipp_rl_amd.planning.mcts_zero.selfplay import iter_totals_host, scan_order_sum

    assert scan_order_sum([]) == 0.0 and scan_order_sum([2.5]) == 2.5
    # one wave: the shuffle scan's last lane is the balanced tree over ... + (x[62] + x[63]); here visible in the last place
    x = np.array([1.0] + [2.0 ** -53] * 63)
    tree = x.copy()
    o = 1
    while o < 64:
        tree = np.concatenate([tree[:o], tree[o:] + tree[:-o]])
        o *= 2
    assert scan_order_sum(x) == tree[63] and scan_order_sum(x) != float(np.cumsum(x)[-1])
    # four waves in wave order, chunks in chunk order
    y = np.arange(1, 601, dtype=np.float64)
    assert scan_order_sum(y) == y.sum()   # (small integers: exact in every order)
    for B in lc.TOTALS_B:
        n, ex, vs, cap = lc.totals_inputs(B)
        t = iter_totals_host(n, ex, vs, cap)
        assert t["episodes_kept"] == sum(min(int(v), cap) for v in n) and t["envs_at_cap"] == sum(int(v) >= cap for v in n)
        assert t["examples"] == int(ex.sum()) and abs(t["value_sum"] - float(np.sum(vs))) <= 1e-12 * float(np.abs(vs).sum())


def test_window_rows_host():
    from ipp_rl_amd.planning.mcts_zero.selfplay import window_rows_host

    flags = np.array([2, 2, 1, 2, 0, 2, 2], np.uint8)
    tags = np.array([0, 1, 1, -1, 1, 2, 3], np.int32)
    assert window_rows_host(flags, tags, 1, 2).tolist() == [1, 5]      # (pending and free rows inside the window: not in it)
    assert window_rows_host(flags, tags, 0, 3).tolist() == [0, 1, 5, 6]  # (tag -1: never in a window of iterations >= 0)
    assert window_rows_host(flags, tags, 4, 9).tolist() == []
    assert window_rows_host(flags, np.full(7, -1), 0, 100).tolist() == []  # (a ring that never saw an iteration)
    for cap in lc.WINDOW_CAPS:
        f, t = lc.window_inputs(cap)
        assert len(window_rows_host(f, t, *lc.WINDOWS["empty"])) == 0
        assert len(window_rows_host(f, t, *lc.WINDOWS["full"])) >= len(window_rows_host(f, t, *lc.WINDOWS["partial"])) >= (cap > 1)


# ---------------------------------------------------------------------------------------------------- ABI
def test_iteration_struct_and_prototypes_match_ffi():
    import ctypes as C

    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    body = re.search(r"typedef struct ipp_selfplay_iter \{(.*?)\} ipp_selfplay_iter;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*").strip() for stmt in body.split(";") if stmt.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]
    assert names == [f[0] for f in _ffi.IppSelfPlayIter._fields_]
    assert C.sizeof(_ffi.IppSelfPlayIter) == 8 + 4 * C.sizeof(C.c_void_p) and C.sizeof(_ffi.IppIterTotals) == 32
    nargs = {"ipp_selfplay_commit_iter": 4, "ipp_selfplay_iter_totals": 4, "ipp_replay_priority_reset_window": 7}
    for name, n in nargs.items():
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\);", txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == n == len(_ffi.PROTOTYPES[name][1]), name
    assert int(re.search(r"#define\s+IPP_ABI_VERSION\s+(\d+)", txt).group(1)) == _ffi.ABI_VERSION


def test_library_exports_the_iteration_calls():
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    for name in ("ipp_selfplay_commit_iter", "ipp_selfplay_iter_totals", "ipp_replay_priority_reset_window"):
        assert getattr(lib, name).argtypes == _ffi.PROTOTYPES[name][1]
    # refusals that need no device: NULL arguments come back as the neighbouring calls' -1
    assert lib.ipp_selfplay_commit_iter(None, 0, None, None) == -1
    assert lib.ipp_selfplay_iter_totals(None, None, None, None) == -1
    assert lib.ipp_replay_priority_reset_window(None, None, 0, 1, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- the Learner's refusals
def test_learner_refuses_what_it_cannot_run():
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import Learner
    from ipp_rl_amd.planning.mcts_zero.learn import check_args

    cfg = EngineConfig(x_dim=40, y_dim=40)
    hp = dict(EXAMPLE, shared_network=False, num_episodes=13, num_workers=22, num_arena_games=40, continuous_network_update=True)
    with pytest.raises(ValueError, match="shared_network"):
        Learner(cfg, 4, hp, {}, module=None, checkpoint_dir="unused")
    hp["shared_network"] = True
    assert check_args(hp, 64, None, None) == (5, None)       # ceil(13 x 22 / 64)
    assert check_args(hp, 286, None, None) == (1, None) and check_args(hp, 4, 2, None) == (2, None)
    hp["continuous_network_update"] = False
    assert check_args(hp, 64, None, None) == (5, 8)          # gcd(40, 64) envs play the 40 arena games
    with pytest.raises(ValueError, match="num_arena_games"):
        check_args(hp, 64, None, 7)
    with pytest.raises(ValueError, match="episodes_per_env"):
        check_args(hp, 64, 0, None)
