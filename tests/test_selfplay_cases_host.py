"""
CPU-only: the frozen constants of tests/selfplay_cases.py reach the edges of csrc/k_selfplay.h that tests/test_hip_selfplay_kernels.py
names them for, and the restatements agree with the pinned host functions where the two can be compared directly.  A case that stops
reaching its edge (another seed, another size) fails here, not silently on the GPU.
"""
import sys

import numpy as np

from tests import selfplay_cases as sc


def test_helper_imports_without_torch():
    import subprocess

    code = "import sys; import tests.selfplay_cases; sys.exit(int('torch' in sys.modules or 'ipp_rl_amd' in sys.modules))"
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


def test_tie_cases_reach_every_ballot_and_rank():
    stats = [s for name in sc.TIE_CASES for s in sc.tie_stats(name)]
    ballots = {b for b, _, _, _ in stats}
    assert {0, 1, 2} <= ballots
    assert any(rank >= 1 for _, rank, _, _ in stats)
    for b in (0, 1, 2):  # a pick of rank >= 1 in each of the first three ballots
        assert any(rank >= 1 for bb, rank, _, _ in stats if bb == b), b
    assert any(n == 1 and K > 1 for _, _, n, K in stats) and any(n == K and K > 64 for _, _, n, K in stats)
    # a pick beyond ballot 0 whose ballot is not the first with ties (`seen` is not 0 there), and one at kmax = 2048 in a late ballot
    for name in ("ties-130", "ties-257", "ties-2048", "temp-zero-depth-0", "high-counter", "high-seed"):
        assert any(b >= 1 for b, _, _, _ in sc.tie_stats(name)), name
    assert max(b for b, _, _, _ in sc.tie_stats("ties-2048")) >= 20
    # every tie case has temperature-0 envs; the cdf cases have both kinds
    for name, c in sc.RECORD_CASES.items():
        st = sc.build_record(name)[0]
        t0 = (st["depth"] >= st["temp_threshold"]) | bool(st["temp_zero"])
        assert t0.any() and (c["temp_zero"] or (~t0).any()), name


def test_record_cases_hold_the_named_sizes_and_sources():
    for k in (1, 63, 64, 65, 130, 257, 2048):
        for layout in ("cdf", "ties"):
            st, step, pol_t, pol_1, vidx, ok = sc.build_record(f"{layout}-{k}")
            K = (vidx >= 0).sum(axis=1)
            assert st["kmax"] == k and {1, k} <= set(K.tolist()) and ok.all()
            if k >= 65:
                assert {64, 65} <= set(K.tolist())
            # the two sources have different maxima: taking the wrong one is visible
            for e in range(st["B"]):
                if K[e] > 1:
                    assert np.argmax(pol_t[e, :K[e]]) != np.argmax(pol_1[e, :K[e]])
            want = sc.record_ref(st, step, pol_t, pol_1, vidx, ok)
            assert (want["flag"] == sc.PENDING).all() and (want["action_idx"] >= 0).all()
            assert want["action_idx"].min() == 0 and (k == 1 or want["action_idx"].max() > 0)
    # the inverse-CDF layouts, on the pol_t path
    st, step, pol_t, pol_1, vidx, ok = sc.build_record("cdf-130")
    rows = [pol_t[e, :(vidx[e] >= 0).sum()] for e in range(st["B"]) if st["depth"][e] < st["temp_threshold"]]
    assert any(p[0] == 0 and p[-1] == 0 and len(p) > 2 for p in rows) and any((p > 0).sum() == 1 for p in rows)
    assert any((p == 1e-300).sum() >= 60 and p.max() == 1.0 for p in rows)
    sums = np.array([p.sum() for p in rows])
    assert (np.abs(sums - 1) < 1e-9).any() and (sums > 3).any() and (sums < 0.02).any()


def test_refusal_case_holds_every_kind_on_both_temperature_paths():
    st, step, pol_t, pol_1, vidx, ok = sc.build_record("refusals")
    want = sc.record_ref(st, step, pol_t, pol_1, vidx, ok)
    seen = set()
    for e in range(st["B"]):
        kind, t0 = sc.refusal_kind(e), bool(st["depth"][e] >= st["temp_threshold"])
        seen.add((kind, t0))
        assert (want["forced"][e] == 1) == (kind != "fine"), (e, kind)
        K = int((vidx[e] >= 0).sum())
        if kind == "index>=A":
            assert ok[e] == 1 and vidx[e].max() >= st["A"]
        if kind == "K=0":
            assert ok[e] == 1 and K == 0
        if kind == "zeros":
            assert ok[e] == 1 and K > 0 and not pol_t[e, :K].any() and not pol_1[e, :K].any()
        if kind == "nan":
            assert ok[e] == 1 and np.isnan(pol_t[e, :K]).sum() == 1 and np.isnan(pol_1[e, :K]).sum() == 1
    assert seen == {(k, t) for k in sc.REFUSAL_KINDS for t in (False, True)}


def test_uniform_cases_reach_the_high_words():
    from ipp_rl_amd.planning.mcts_zero import selfplay as sp
    from ipp_rl_amd.vec_env import philox_uniform

    def uniforms(st, stream, seed=None, low_counter=False):
        gid = np.arange(st["B"], dtype=np.int64) + st["row_offset"]
        q = sp.step_counter(gid, st["depth"])
        return philox_uniform(q & 0xFFFFFFFF if low_counter else q, stream + st["episode"], st["seed"] if seed is None else seed)

    for name in ("high-counter", "huge-counter", "max-depth"):
        st, step, pol_t, pol_1, vidx, ok = sc.build_record(name)
        assert st["row_offset"] >= 4096
        q = sp.step_counter(np.arange(st["B"], dtype=np.int64) + st["row_offset"], st["depth"])
        assert (q >= 2 ** 32).all()
        for stream in (sp.ACTION_STREAM, sp.ARGMAX_STREAM, sp.TIE_STREAM):
            assert (uniforms(st, stream) != uniforms(st, stream, low_counter=True)).all()
        # ... and the recorded actions differ where the counter's high word is dropped
        low = sc.copy_state(st)
        low["row_offset"] = st["row_offset"] & 0xFFF  # (gid << 20 without its bits from 32 up)
        a, b = sc.record_ref(st, step, pol_t, pol_1, vidx, ok), sc.record_ref(low, step, pol_t, pol_1, vidx, ok)
        assert (a["action_idx"] != b["action_idx"]).sum() >= 8, name
    st, step, pol_t, pol_1, vidx, ok = sc.build_record("max-depth")
    assert set(st["depth"].tolist()) == {2 ** 20 - 2, 2 ** 20 - 1}
    st, step, pol_t, pol_1, vidx, ok = sc.build_record("high-seed")
    assert st["seed"] >= 2 ** 32
    for stream in (sp.ACTION_STREAM, sp.ARGMAX_STREAM, sp.TIE_STREAM):
        assert (uniforms(st, stream) != uniforms(st, stream, seed=st["seed"] & 0xFFFFFFFF)).all()
    low = sc.copy_state(st)
    low["seed"] = st["seed"] & 0xFFFFFFFF
    a, b = sc.record_ref(st, step, pol_t, pol_1, vidx, ok), sc.record_ref(low, step, pol_t, pol_1, vidx, ok)
    assert (a["action_idx"] != b["action_idx"]).sum() >= 8


def test_gather_configurations_hold_the_named_offsets():
    offs = sc.offsets_of(sc.ALL_OFFSETS)
    assert tuple(offs[0]) == (4, 4)
    assert {(i, j) for i, j in offs[1:].tolist()} == {(i, j) for i in range(9) for j in range(9)}
    few = sc.offsets_of(sc.FEW_OFFSETS)[1:]
    dy, dx = few[:, 0] - 4, few[:, 1] - 4
    assert ((dx == 0) & (dy != 0)).any() and (dx == -4).any() and (dx == 4).any() and (dy == -4).any() and (dy == 4).any()
    assert len(few) <= 64
    for side in sc.GATHER_SIDES:
        assert (side % 4 == 0) == (side in (4, 8, 36))
    assert 18 * 18 > 256 and 36 * 36 > 4 * 256 and 8 * 8 <= 4 * 256


def test_draw_cases_draw_the_first_and_the_last_committed_row():
    from ipp_rl_amd.planning.mcts_zero.selfplay import replay_draws

    seen = set()
    for c in sc.DRAW_CASES:
        flags = sc.committed_pattern(c["cap"], c["pattern"])
        committed = np.nonzero(flags == sc.COMMITTED)[0]
        seen.add((c["cap"], c["pattern"]))
        if c["pattern"] == "none":
            assert len(committed) == 0
            continue
        rows, _ = replay_draws(c["n"], 1, sc.DRAW_SEED, c["draw"], committed)
        if c["ends"]:
            assert committed[0] in rows and committed[-1] in rows, c
    for cap, want in ((1, 1), (2, 2), (320, 320)):
        assert len(sc.committed_pattern(cap, "all")) == want
    assert {(320, p) for p in ("first", "last", "every-other", "all", "none")} <= seen and {c["n"] for c in sc.DRAW_CASES} == {1, 255, 256, 257}
    # an even count of committed rows above 2 with both ends drawn: what tells floor(u total) clamped from floor(u total) wrapped
    every = sc.committed_pattern(320, "every-other")
    assert (every == sc.COMMITTED).sum() == 160 and every[0] != sc.COMMITTED and every[319] == sc.COMMITTED


def test_dense_cases_hold_both_end_actions_and_an_exact_zero():
    for kmax, K, A in sc.DENSE_CASES:
        st, _ = sc.build_ring(8, kmax, K, A)
        idx, pol = st["r_idx"], st["r_policy"]
        assert ((idx[0] >= 0).sum(), (idx[1] >= 0).sum()) == (K, K) and idx[0, 0] == 0 and idx[1, K - 1] == A - 1
        for r in range(8):
            k = int((idx[r] >= 0).sum())
            assert k >= 1 and np.all(np.diff(idx[r, :k]) > 0) and np.all(idx[r, k:] == -1) and idx[r, k - 1] < A
            assert (pol[r, :k] == 0).sum() == 1 and np.all(pol[r, k:] > 0)  # (garbage behind the valid set)


def test_commit_ref_is_value_targets_on_a_straight_episode():
    from ipp_rl_amd.planning.mcts_zero.selfplay import value_targets

    for T in sc.COMMIT_LENGTHS:
        for horizon, gamma in zip(sc.commit_horizons(T), (0.9, 0.97, 1.0, 0.9, 0.97)):
            step = T  # rows 1 .. T of env 0, ended by done
            st, episodes = sc.build_commit(T, horizon, gamma, step)
            assert episodes[0] == (T, "done")
            rows = np.arange(1, T + 1) * st["B"]
            assert np.array_equal(sc.episode_rows(step, T, False, st["S"], st["B"], 0), rows)
            rewards = np.append(st["r_reward"][rows[:-1]], float(st["reward"][0]))
            vals, tot = value_targets(rewards, gamma, horizon)
            out = sc.commit_ref(st, step)
            assert np.array_equal(out["r_value"][rows], vals) and out["episode_value"][0] == tot
            assert np.all(out["r_flags"][rows] == sc.COMMITTED) and out["ep_len"][0] == 0
            assert st["r_reward"].max() <= 0.05 and st["reward"].max() <= 0.05 and st["S"] == T + 1


def test_commit_cases_straddle_the_wrap():
    for T in sc.COMMIT_LENGTHS:
        kinds, steps = set(), set()
        launches = sc.commit_launches(T)
        assert {(h, g) for h, g, _, _ in launches} == {(h, g) for h in (0, 1, 3, T, T + 5) for g in (0.9, 0.97, 1.0)}
        for horizon, gamma, step, random_init in launches:
            st, episodes = sc.build_commit(T, horizon, gamma, step, random_init)
            S, B = st["S"], st["B"]
            steps.add((step, gamma != 1.0, random_init))
            for e, (Te, kind) in enumerate(episodes):
                slots = sc.episode_rows(step, Te, kind == "forced", S, B, e) // B
                if Te > 1 and np.any(np.diff(slots) < 0):
                    assert slots[0] > slots[-1] and S - 1 in slots and 0 in slots
                    kinds.add(kind)
            assert (0, "forced") in episodes and (T, "done") in episodes and (T, "forced") in episodes and (T, "on") in episodes
        if T >= 2:
            assert {"done", "forced", "on"} <= kinds, (T, kinds)
        assert len({s for s, _, _ in steps}) == (3 if T > 1 else 2) and {r for _, _, r in steps} == {0, 1}


def test_gather_ref_of_copy_zero_is_the_identity():
    st, planes = sc.build_ring(6, 5, 5, 7, side=6)
    out = sc.gather_ref(st, planes, 4, 3, 9, 2)
    rows = out["index"][:4]
    assert np.array_equal(out["index"], np.tile(rows, 3)) and tuple(out["offsets"][0]) == (4, 4)
    assert np.array_equal(sc.bits(out["states"][:4]), sc.bits(planes[rows]))
    same = sc.gather_rows_ref(st, planes, rows)
    for k in ("policy", "mask", "value", "reward"):
        assert np.array_equal(out[k][:4], same[k])
    assert np.isnan(planes).any() and np.isinf(planes).any() and (sc.bits(planes) == 0x80000000).any()
    # the empty row
    empty = sc.gather_rows_ref(st, planes, [-1, 6, 13])
    assert np.isnan(empty["states"]).all() and np.isnan(empty["value"]).all() and not empty["policy"].any() and not empty["mask"].any()
