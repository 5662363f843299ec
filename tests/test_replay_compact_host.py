"""
CPU tests of the compact replay ring's host side (planning/mcts_zero/selfplay.py: archive_slot, eviction_host, check_replay_mode;
include/ipp_engine.h: ipp_replay_compact and its three calls):
  * the archive slot rule and the eviction rule -- the oracles of tests/test_hip_replay_compact.py -- on a hand-made trace of one env with
    one-step episodes, a step without a sample and E in {1, 2, S}, against rows and counts worked out by hand; E >= S never evicts;
  * header and _ffi agree on the struct and the prototypes, the ABI number is the binding's, the library exports the calls and refuses
    NULL arguments without a device;
  * what SelfPlay refuses before it touches a device: archive_episodes < 1, an unknown planes mode, 'compact' on a grid without patch layout.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = {"ipp_replay_record_compact": 6, "ipp_selfplay_archive": 4, "ipp_replay_compact_planes": 12}

# one env, S = 4 step slots: (episode tag, the step left a sample, the episode ended in the step)
TRACE = [(0, True, True),    # t0 row 0: a one-step episode
         (1, True, False),   # t1 row 1
         (1, True, True),    # t2 row 2: episode 1 ends with rows 1, 2
         (2, True, True),    # t3 row 3: one step again
         (3, True, False),   # t4 row 0 re-opened
         (3, True, True),    # t5 row 1 re-opened: episode 3 ends with rows 0, 1
         (4, False, True)]   # t6 row 2: a root without a policy at the episode's first step (no sample, T = 0)
# by hand: (flags after t5, evicted after t5, flags after t6, evicted after t6)
EXPECT = {1: ([2, 2, 0, 0], 4, [0, 0, 0, 0], 6),   # E = 1: every end evicts the episode before it
          2: ([2, 2, 0, 2], 2, [2, 2, 0, 0], 3),   # E = 2: episode 2's end takes row 0 (tag 0), episode 3's row 2 (tag 1), episode 4's row 3 (tag 2)
          4: ([2, 2, 2, 2], 0, [2, 2, 0, 2], 0)}   # E = S: only the ring's own wrap-around (row 2 re-opened at t6)


def test_archive_slot_rule():
    from ipp_rl_amd.planning.mcts_zero.selfplay import archive_slot

    B, E = 3, 2
    got = [[int(archive_slot(B, E, e, p)) for p in range(5)] for e in range(B)]
    assert got == [[3, 4, 3, 4, 3], [5, 6, 5, 6, 5], [7, 8, 7, 8, 7]]
    # the spare slots [B, B + B E) are used, each by one (env, episode mod E), and never an env slot
    slots = archive_slot(5, 3, np.repeat(np.arange(5), 3), np.tile(np.arange(3), 5))
    assert sorted(slots.tolist()) == list(range(5, 20))
    assert int(archive_slot(4, 1, 2, 10 ** 12)) == 6  # (E = 1: one slot per env; int64 episode counters)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_eviction_rule_on_a_hand_made_trace(E):
    from ipp_rl_amd.planning.mcts_zero.selfplay import eviction_host

    f5, n5, f6, n6 = EXPECT[E]
    flags, tags, evicted = eviction_host(TRACE[:6], 4, E)
    assert flags.tolist() == f5 and evicted == n5 and tags.tolist() == [3, 3, 1, 2]
    flags, tags, evicted = eviction_host(TRACE, 4, E)
    assert flags.tolist() == f6 and evicted == n6 and tags.tolist() == [3, 3, 4, 2]


def test_no_eviction_with_as_many_archive_slots_as_step_slots():
    """An episode takes at least one step, so when episode p ends the row of every step of episode p - S has been re-opened."""
    from ipp_rl_amd.planning.mcts_zero.selfplay import eviction_host

    rs = np.random.RandomState(0)
    for S in (2, 3, 7):
        trace, p = [], 0
        for _ in range(200):
            ended = rs.rand() < 0.45
            trace.append((p, bool(rs.rand() < 0.8 or not ended), ended))  # (a step without a sample always ends the episode)
            p += int(ended)
        for E in (S, S + 3):
            assert eviction_host(trace, S, E)[2] == 0
        assert eviction_host(trace, S, 1)[2] > 0


def test_struct_and_prototypes_match_ffi():
    import ctypes as C

    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    body = re.search(r"typedef struct ipp_replay_compact \{(.*?)\} ipp_replay_compact;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"^\s*(const\s+)?\w+\s*\*?\s*", "", stmt.strip()) for stmt in body.split(";") if stmt.strip()]
    assert names == [f[0] for f in _ffi.IppReplayCompact._fields_]
    assert C.sizeof(_ffi.IppReplayCompact) == 8 + 6 * C.sizeof(C.c_void_p)
    for name, n in NEW_CALLS.items():
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\);", txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == n == len(_ffi.PROTOTYPES[name][1]), name
    assert int(re.search(r"#define\s+IPP_ABI_VERSION\s+(\d+)", txt).group(1)) == _ffi.ABI_VERSION == 17
    # the reference's lines the declarations cite
    assert "replay_buffers.py:48-101" in txt and "episode_generators.py:157-192" in txt
    # existing structs keep their layout: the new calls take a struct of their own
    assert C.sizeof(_ffi.IppSelfPlay) == 10 * 4 + 3 * 8 + 18 * C.sizeof(C.c_void_p) and C.sizeof(_ffi.IppPlaneSpec) == 6 * 4 + 2 * 8


def test_library_exports_the_compact_calls():
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    for name in NEW_CALLS:
        assert getattr(lib, name).argtypes == _ffi.PROTOTYPES[name][1]
    assert lib.ipp_replay_record_compact(None, None, None, 0, None, None) == -1
    assert lib.ipp_selfplay_archive(None, None, None, None) == -1
    assert lib.ipp_replay_compact_planes(None, None, None, None, 1, 1, None, None, None, None, None, None) == -1


def _dicts():
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=8, temperature_scale=1.0, temperature_threshold=3, input_history_length=2,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=24.0, max_episode_steps=5, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    return hp, md


def test_selfplay_refuses_before_it_touches_a_device():
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.engine import patch_layout_possible
    from ipp_rl_amd.planning.mcts_zero import SelfPlay
    from ipp_rl_amd.planning.mcts_zero.selfplay import check_replay_mode

    hp, md = _dicts()
    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="archive_episodes"):
            SelfPlay(cfg, 3, hp, md, planes="compact", archive_episodes=bad)
    with pytest.raises(ValueError, match="archive_episodes"):
        SelfPlay(cfg, 3, hp, md, planes=True, archive_episodes=0)
    for bad in ("dense", "Compact", 1, None, 2):
        with pytest.raises(ValueError, match="planes"):
            SelfPlay(cfg, 3, hp, md, planes=bad)
    # 20x20 cannot hold the two-dimensional windows of the patch layout (x_dim > 2 R + 13 with the 10-row window of the example prior)
    small = EngineConfig(x_dim=20, y_dim=20, simulation="split_random_field")
    assert patch_layout_possible(cfg) and not patch_layout_possible(small)
    assert not patch_layout_possible(cfg, state="dense") and not patch_layout_possible(cfg, window_rows=0)
    assert not patch_layout_possible(cfg, rank_cap=513) and not patch_layout_possible(EngineConfig(x_dim=41, y_dim=41))
    with pytest.raises(ValueError, match="patch"):
        SelfPlay(small, 3, hp, md, planes="compact")
    with pytest.raises(ValueError, match="patch"):
        SelfPlay(cfg, 3, hp, md, planes="compact", window_rows=0)
    # E: None = the ring's step slots, 0 in the other modes
    assert check_replay_mode("compact", None, 6) == 6 and check_replay_mode("compact", 2, 6) == 2
    assert check_replay_mode(True, None, 6) == 0 and check_replay_mode(False, 4, 6) == 0
