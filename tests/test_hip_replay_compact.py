"""
GPU tests of the compact replay ring (planning/mcts_zero/selfplay.py planes="compact"; csrc/k_replay_compact.h: ipp_replay_record_compact,
ipp_selfplay_archive, ipp_replay_compact_planes) against the dense ring of the same seed:
  1. bit identity: minibatches (uniform with augmented copies, prioritised, the window of an iteration) equal the dense ring's in all
     seven outputs while the ring wraps and archive slots are reused; nothing evicted with the default E = S; no planes tensor, rows of
     a few KB;
  2. forced ends (a root without a policy): the earlier rows of those episodes draw the dense ring's planes;
  3. interval_factor = 2: the planes of drawn rows are ipp_feature_planes of the rows' stored entries and mean on the archive slots
     (pinned to the fp64 oracle by tests/test_hip_feature_planes.py); everything but the planes equals the dense ring's;
  4. eviction with E = 2 and one- and two-step episodes: the counter and the committed rows equal the host restatement (eviction_host) fed
     with the recorded trace, every surviving row's planes equal the dense ring's row;
  5. two shards give the rows of one process.
Shapes: the smallest square split-field grid with patch layout (20x20 if the engine reports it there, else 40x40), B in {3, 5}, history 2,
5-step episodes that end by budget at different steps, 8 simulations, no network.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

UAV = {"max_v": 2.0, "max_a": 2.0}
STEPS, HISTORY = 5, 2


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    """Same shape, dtype and bits (NaNs included)."""
    import torch

    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype in (torch.float32, torch.float64):
        w = torch.int32 if a.dtype == torch.float32 else torch.int64
        return torch.equal(a.contiguous().view(w), b.contiguous().view(w))
    return torch.equal(a, b)


def same_batch(x, y):
    assert len(x) == len(y) == 7
    for i, (a, b) in enumerate(zip(x, y)):
        assert bits_equal(a, b), f"output {i} differs"


_GRID = []


def grid_dim():
    """20 if a 20x20 engine has the patch layout, else the 40 of tests/test_hip_selfplay.py."""
    if not _GRID:
        from ipp_rl_amd import EngineConfig, IPPEngine

        eng = IPPEngine(EngineConfig(x_dim=20, y_dim=20, simulation="split_random_field"), capacity=1, state="factor", rank_cap=90,
                        window_rows=-1, fixed_prior=True)
        _GRID.append(20 if int(eng.info.patch_layout) == 1 else 40)
        eng.close()
    return _GRID[0]


def make(planes, B, seed=3, interval_factor=0.0, **over):
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=8, temperature_scale=1.0, temperature_threshold=3, input_history_length=HISTORY,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=24.0, max_episode_steps=STEPS, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications=UAV, scenario_info={"value_threshold": 0.4, "interval_factor": interval_factor})
    # (8 simulations one after the other: in waves of 4 they visit 8 different actions of the ~100 valid ones once each, and the
    # read-out drops single visits (mcts.py: no policy, every step a forced end); a sequential search returns to its best action)
    kw = dict(sims_in_flight=1)
    for k, v in over.items():
        if k in md:
            md[k] = v
        elif k in hp:
            hp[k] = v
        else:
            kw[k] = v
    d = grid_dim()
    cfg = EngineConfig(x_dim=d, y_dim=d, simulation="split_random_field", interval_factor=float(interval_factor))
    return SelfPlay(cfg, B, hp, md, planes=planes, seed=seed, **kw)


def entry_bytes():
    from ipp_rl_amd.feature_planes import ENTRY_DTYPE

    return ENTRY_DTYPE.itemsize


def check_compact_size(sp):
    r = sp.replay
    rows, N = r.capacity, sp.env.cfg.n_cells
    assert r.planes is None and r.compact is not None
    small = sum(t.numel() * t.element_size() for t in (r.policy, r.idx, r.value, r.reward, r.flags))
    assert r.nbytes() <= rows * (HISTORY * entry_bytes() + 4 * N + 16) + small


def assert_same_rows(dense, compact, rows):
    """gather_rows of the given ring rows: all five outputs bit for bit."""
    for a, b in zip(dense.replay.gather_rows(rows), compact.replay.gather_rows(rows)):
        assert bits_equal(a, b)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("B", [3, 5])
def test_minibatches_equal_the_dense_rings(B):
    import torch

    dense, compact = make(True, B), make("compact", B)
    S, N = dense.slots, dense.env.cfg.n_cells
    assert S == STEPS + 1 == compact.slots and compact.replay.archive_episodes == S
    assert compact.env.engine.capacity == B * (1 + S) and dense.env.engine.capacity == B
    check_compact_size(compact)
    assert dense.replay.nbytes() > 100 * compact.replay.nbytes()

    def check(t):
        assert bits_equal(dense.replay.flags, compact.replay.flags)
        x, y = dense.replay.sample(9, num_augmented_samples=2), compact.replay.sample(9, num_augmented_samples=2)
        same_batch(x, y)
        assert tuple(y[0].shape) == (9, 5 * HISTORY + 1, N, N) and torch.isfinite(y[0]).all() and (y[5] >= 0).all()  # (planes, not NaN = NaN)
        assert float(y[0][:3, 0].max()) == 1.0 and float(y[0][:3, 0].min()) == 0.0  # (a min-max normalised covariance plane)
        assert bits_equal(dense.replay.last_offsets, compact.replay.last_offsets)
        per = [r.replay.prioritized(batch_size=4) for r in (dense, compact)]
        for _ in range(2):
            x, y = per[0].sample(), per[1].sample()
            same_batch(x, y)
            for p, b in zip(per, (x, y)):
                p.update(b[5], torch.rand(4, generator=torch.Generator().manual_seed(t)).double() + 1e-8)
                p.step()
        assert_same_rows(dense, compact, dense.replay.committed_rows())

    t = 0
    while t < 3 * S + 1 or (int(compact.replay.episodes.min().item()) <= S and t < 8 * S):
        dense.step()
        compact.step()
        if t in (S, 2 * S - 1, 3 * S):  # (before the ring wraps, in the wrap, behind it)
            check(t)
        t += 1
    assert int(compact.replay.episodes.min().item()) > S  # (every env has reused an archive slot: more than E = S episodes ended)
    check(t)
    # an iteration of the learn loop on top: reset, tagged rows, the window's draws
    for r in (dense, compact):
        r.run_iteration(0, 1)
    assert bits_equal(dense.replay.flags, compact.replay.flags) and bits_equal(dense.replay.iter, compact.replay.iter)
    same_batch(dense.replay.window(0, 0).sample(6, num_augmented_samples=1), compact.replay.window(0, 0).sample(6, num_augmented_samples=1))
    same_batch(dense.replay.window(0, 0).prioritized(batch_size=3).sample(), compact.replay.window(0, 0).prioritized(batch_size=3).sample())
    assert compact.replay.evicted == 0 and dense.replay.evicted == 0
    check_compact_size(compact)
    dense.close()
    compact.close()


# ---------------------------------------------------------------------------------------------------- 2
def manual_step(sp, no_policy):
    """SelfPlay.step with the ok flags of the envs `no_policy` zeroed (tests/test_hip_selfplay.py, test_no_policy_ends_the_episode_at_kernel_level)."""
    from ipp_rl_amd import _ffi

    env, r, B, t = sp.env, sp.replay, sp.num_envs, sp.t
    slot = t % sp.slots
    ent = env.history_entries()
    if r.compact is not None:
        _ffi.check(sp._lib.ipp_replay_record_compact(env.engine._h, C.byref(sp._sp), C.byref(r.compact), t, ent.data_ptr(), env.engine.stream))
    else:
        env.engine.feature_planes(ent, sp.spec, mask_env=ent[:, 0, 0], out=r.planes[slot * B:(slot + 1) * B])
    out = sp.mcts.search_device(sp._roots, env.prev, env.budget, sp._temps, sp.tie_u, depth=0)
    ok = out["ok"].clone()
    ok[no_policy] = 0
    pol_t, pol_1 = out["policy"][sp._t_index[0]], out["policy"][sp._t_index[1]]
    _ffi.check(sp._lib.ipp_selfplay_record(C.byref(sp._sp), t, pol_t.data_ptr(), pol_1.data_ptr(), out["valid_idx"].data_ptr(), ok.data_ptr(),
                                           env.engine.stream))
    env.step(sp.action)
    if r.compact is not None:
        _ffi.check(sp._lib.ipp_selfplay_archive(env.engine._h, C.byref(sp._sp), C.byref(r.compact), env.engine.stream))
    _ffi.check(sp._lib.ipp_selfplay_commit(C.byref(sp._sp), t, env.engine.stream))
    sp.t += 1


def test_forced_ends_keep_the_earlier_rows():
    B = 5
    dense, compact = make(True, B, seed=9, initial_budget=400.0), make("compact", B, seed=9, initial_budget=400.0)
    for r in (dense, compact):
        r.step()
        r.step()
    assert len(dense.replay) == 0  # (a budget of 400: nothing has ended)
    ep0 = host(compact.replay.episodes).copy()
    for r in (dense, compact):
        manual_step(r, [1, 4])
    flags = host(compact.replay.flags).reshape(compact.slots, B)
    assert bits_equal(dense.replay.flags, compact.replay.flags)
    for e in (1, 4):  # two samples each, committed by the forced end; the forced step's own row is no sample
        assert flags[:, e].tolist() == [2, 2, 0, 0, 0, 0]
    for e in (0, 2, 3):
        assert flags[:, e].tolist() == [1, 1, 1, 0, 0, 0]
    assert (host(compact.replay.episodes) - ep0).tolist() == [0, 1, 0, 0, 1]  # (read on the device: only the ended envs were archived)
    rows = compact.replay.committed_rows()
    assert rows.numel() == 4
    assert_same_rows(dense, compact, rows)
    for r in (dense, compact):  # the envs go on; a forced end at the first step of an episode (T = 0) archives an empty prefix
        manual_step(r, [1])
        r.step()
    assert bits_equal(dense.replay.flags, compact.replay.flags)
    assert_same_rows(dense, compact, compact.replay.committed_rows())
    same_batch(dense.replay.sample(4, num_augmented_samples=1), compact.replay.sample(4, num_augmented_samples=1))
    assert compact.replay.evicted == 0
    dense.close()
    compact.close()


# ---------------------------------------------------------------------------------------------------- 3
def test_adaptive_interval_planes_are_feature_planes_of_the_archive():
    import torch

    B = 3
    dense, compact = make(True, B, seed=11, interval_factor=2.0), make("compact", B, seed=11, interval_factor=2.0)
    for _ in range(2 * compact.slots):
        dense.step()
        compact.step()
    assert bits_equal(dense.replay.flags, compact.replay.flags)
    x, y = dense.replay.sample(8, num_augmented_samples=1), compact.replay.sample(8, num_augmented_samples=1)
    for i in (1, 2, 3, 4, 5, 6):  # policies, values, rewards, masks, indices, weights
        assert bits_equal(x[i], y[i]), i
    n, rows = 4, y[5][:4]
    r = compact.replay
    ent = r.entries[rows]
    slots = host(ent[:, :, 0])
    valid = host(ent[:, :, 8]) == 1
    assert valid[:, 0].all() and (slots[valid] >= B).all() and (slots[valid] < B * (1 + r.archive_episodes)).all()
    assert (host(ent[:, 0, 1]) >= 0).all()  # (entry 0's rank is explicit)
    direct = compact.env.engine.feature_planes(ent, compact.spec, mask_mean=r.mean[rows])
    assert bits_equal(y[0][:n], direct)
    assert bits_equal(r.gather_rows(rows)[0], direct)
    assert torch.isfinite(direct).all()
    dense.close()
    compact.close()


# ---------------------------------------------------------------------------------------------------- 4
def test_eviction_matches_the_host_restatement():
    from ipp_rl_amd.planning.mcts_zero.selfplay import archive_slot, eviction_host

    B, E = 5, 2
    dense, compact = make(True, B, seed=6, initial_budget=7.0), make("compact", B, seed=6, initial_budget=7.0, archive_episodes=E)
    S, r = compact.slots, compact.replay
    assert compact.env.engine.capacity == B * (1 + E)
    trace = [[] for _ in range(B)]
    for _ in range(2 * S + 3):
        tag = host(r.episodes).copy()
        dense.step()
        compact.step()
        rec, end = host(compact.action_idx) >= 0, ~np.isnan(host(compact.episode_values))
        for e in range(B):
            trace[e].append((int(tag[e]), bool(rec[e]), bool(end[e])))
    flags, tags = host(r.flags).reshape(S, B), host(r.episode_tag).reshape(S, B)
    total = 0
    for e in range(B):
        f, tg, n = eviction_host(trace[e], S, E)
        assert flags[:, e].tolist() == f.tolist() and tags[:, e].tolist() == tg.tolist(), e
        total += n
    assert r.evicted == total > 0
    # a surviving row names the archive slot of its own episode, and its planes are the dense ring's row
    rows = r.committed_rows()
    hr = host(rows)
    assert 0 < len(hr) <= len(dense.replay)
    ent0 = host(r.entries[rows][:, 0, 0])
    assert ent0.tolist() == archive_slot(B, E, hr % B, host(r.episode_tag)[hr]).tolist()
    assert (host(dense.replay.flags)[hr] == 2).all()
    assert_same_rows(dense, compact, rows)
    dense.close()
    compact.close()


# ---------------------------------------------------------------------------------------------------- 5
def test_two_shards_give_the_rows_of_one_process():
    import torch

    B, cut = 5, 2
    one = make("compact", B, seed=4)
    two = [make("compact", n, seed=4, env_id_offset=o) for o, n in ((0, cut), (cut, B - cut))]
    S = one.slots
    for _ in range(S + 3):
        one.step()
        for s in two:
            s.step()
        assert np.array_equal(host(one.action_idx), np.concatenate([host(s.action_idx) for s in two]))
    for name in ("flags", "episode_tag", "value", "reward"):
        whole = host(getattr(one.replay, name)).reshape(S, B)
        parts = np.concatenate([host(getattr(s.replay, name)).reshape(S, -1) for s in two], axis=1)
        assert np.array_equal(whole, parts, equal_nan=whole.dtype.kind == "f"), name
    assert np.array_equal(host(one.replay.mean).reshape(S, B, -1), np.concatenate([host(s.replay.mean).reshape(S, s.num_envs, -1) for s in two], axis=1))
    fl = host(one.replay.flags).reshape(S, B)
    for o, s in zip((0, cut), two):
        st, ev = np.nonzero(fl[:, o:o + s.num_envs] == 2)
        assert len(st)
        a = one.replay.gather_rows(torch.as_tensor(st * B + ev + o))
        b = s.replay.gather_rows(torch.as_tensor(st * s.num_envs + ev))
        for u, v in zip(a, b):
            assert bits_equal(u, v)
    for s in [one] + two:
        s.close()
