"""
GPU tests of csrc/k_selfplay.h at kernel level: ipp_selfplay_record, ipp_selfplay_commit, ipp_replay_gather and ipp_replay_gather_rows
on bare rings (tests/selfplay_cases.py: SyntheticRing, no engine, no search) against the fp64 NumPy restatements of the same file,
which are composed from the host functions that tests/test_selfplay_host.py pins to the reference.  tests/test_selfplay_cases_host.py
proves on the CPU that the frozen cases reach the edges they are named for ("Self-play kernels on bare rings", has the
table).

Everything a kernel stores or moves is compared bit for bit (policies, indices, flags, actions, masks, planes as uint32, rows, offsets,
uniforms).  The value targets and the episode value are the only inexact outputs: atol 1e-12, the bound tests/test_hip_selfplay.py
asserts for them.  Measured on an MI355X: at most 2.3e-16 over all 90 commit launches (rewards in [0, 0.05], sums of up to 135 terms).
"""
import numpy as np
import pytest

from tests import selfplay_cases as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

VALUE_ATOL = 1e-12
UNTOUCHED_BY_RECORD = ("actions", "depth", "episode", "done", "prev", "reward", "tie_u", "episode_value", "r_value", "r_reward")
UNTOUCHED_BY_COMMIT = ("actions", "budget", "depth", "episode", "done", "reward", "action", "action_idx", "r_policy", "r_idx")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(sc.bits(a), sc.bits(b))


# ---------------------------------------------------------------------------------------------------- record
def _check_record(name):
    st, step, pol_t, pol_1, vidx, ok = sc.build_record(name)
    want = sc.record_ref(st, step, pol_t, pol_1, vidx, ok)
    got = sc.SyntheticRing(st).record(step, pol_t, pol_1, vidx, ok)
    rows, bad = want["rows"], []
    for e in range(st["B"]):
        same = (got["action_idx"][e] == want["action_idx"][e], got["r_flags"][rows[e]] == want["flag"][e], got["forced"][e] == want["forced"][e],
                same_bits(got["r_policy"][rows[e]], want["policy"][e]), np.array_equal(got["r_idx"][rows[e]], want["idx"][e]))
        if not all(same):  # (env, depth, K, action index got and wanted, which of the five comparisons hold)
            bad.append((e, int(st["depth"][e]), int((vidx[e] >= 0).sum()), int(got["action_idx"][e]), int(want["action_idx"][e]), same))
    assert not bad, (name, len(bad), bad[:12])
    for k in ("action", "ep_len", "budget"):
        assert same_bits(got[k], want[k]), (name, k)
    # nothing else moved: the other rows of the ring, the env's own fields
    others = np.setdiff1d(np.arange(st["B"] * st["S"]), rows)
    for k in ("r_policy", "r_idx", "r_flags"):
        assert same_bits(got[k][others], st[k][others]), (name, k)
    for k in UNTOUCHED_BY_RECORD:
        assert same_bits(got[k], st[k]), (name, k)
    return st, want, got


@pytest.mark.parametrize("name", [n for n in sc.RECORD_CASES if n != "refusals"])
def test_record(name):
    st, want, got = _check_record(name)
    assert (want["flag"] == sc.PENDING).all() and (got["action_idx"] >= 0).all()
    t0 = (st["depth"] >= st["temp_threshold"]) | bool(st["temp_zero"])
    rows = want["rows"]
    onehot = (got["r_policy"][rows] == 1.0).sum(axis=1) == 1
    assert np.all(onehot[t0]) and np.all((got["r_policy"][rows][t0] != 0).sum(axis=1) == 1)
    assert np.array_equal(got["action"], st["actions"][got["action_idx"]])


def test_record_ends_an_env_without_a_recordable_policy():
    """ok == 0; ok == 1 with the mass on an index that is no action, with an empty valid set, with a policy of zeros and with a NaN in
    it: forced, budget 0, the action is the current waypoint, no sample, and the row's earlier policy and valid set stay."""
    st, want, got = _check_record("refusals")
    rows = want["rows"]
    for e in range(st["B"]):
        kind = sc.refusal_kind(e)
        if kind == "fine":
            assert got["forced"][e] == 0 and got["r_flags"][rows[e]] == sc.PENDING and got["budget"][e] == st["budget"][e]
            assert got["ep_len"][e] == st["ep_len"][e] + 1
            continue
        assert got["forced"][e] == 1 and got["budget"][e] == 0.0 and got["action_idx"][e] == -1 and got["r_flags"][rows[e]] == 0, (e, kind)
        assert np.array_equal(got["action"][e], st["prev"][e]) and got["ep_len"][e] == st["ep_len"][e], (e, kind)
        assert same_bits(got["r_policy"][rows[e]], st["r_policy"][rows[e]]) and np.array_equal(got["r_idx"][rows[e]], st["r_idx"][rows[e]])


# ---------------------------------------------------------------------------------------------------- commit
def _check_commit(st, step, label):
    want = sc.commit_ref(st, step)
    got = sc.SyntheticRing(st).commit(step)
    for k in ("r_reward", "r_flags", "ep_len", "prev", "tie_u", "forced"):
        assert same_bits(got[k], want[k]), (label, k)
    assert np.array_equal(np.isnan(got["episode_value"]), np.isnan(want["episode_value"])), label
    ended = ~np.isnan(want["episode_value"])
    moved = want["r_flags"] != st["r_flags"]   # the rows this step committed
    assert same_bits(got["r_value"][~moved], st["r_value"][~moved]), label
    err = max(np.abs(got["r_value"][moved] - want["r_value"][moved]).max(initial=0.0),
              np.abs(got["episode_value"][ended] - want["episode_value"][ended]).max(initial=0.0))
    assert err <= VALUE_ATOL, (label, err)
    for k in UNTOUCHED_BY_COMMIT:
        assert same_bits(got[k], st[k]), (label, k)
    return want, got, err


@pytest.mark.parametrize("T", sc.COMMIT_LENGTHS)
def test_commit(T):
    worst = 0.0
    for horizon, gamma, step, random_init in sc.commit_launches(T):
        st, episodes = sc.build_commit(T, horizon, gamma, step, random_init)
        label = (T, horizon, gamma, step, random_init)
        want, got, err = _check_commit(st, step, label)
        worst = max(worst, err)
        B, S = st["B"], st["S"]
        for e, (Te, kind) in enumerate(episodes):
            own = (step % S) * B + e
            if kind == "on":  # the episode goes on: the reward is stored, the rows stay pending, ep_len stays
                assert np.isnan(got["episode_value"][e]) and got["r_reward"][own] == float(st["reward"][e])
                assert got["ep_len"][e] == Te and np.all(got["r_flags"][sc.episode_rows(step, Te, False, S, B, e)] == sc.PENDING)
                assert np.array_equal(got["prev"][e], st["prev"][e])
                continue
            rows = sc.episode_rows(step, Te, kind == "forced", S, B, e)
            assert np.all(got["r_flags"][rows] == sc.COMMITTED) and got["ep_len"][e] == 0 and not np.isnan(got["episode_value"][e])
            if kind == "forced":  # the forced step's own slot is no part of the episode
                assert own not in rows and got["r_flags"][own] == 0 and got["r_reward"][own] == st["r_reward"][own]
                if Te:
                    assert rows[-1] == ((step - 1) % S) * B + e
            if Te == 0:
                assert got["episode_value"][e] == 0.0
            if not random_init:
                assert np.array_equal(got["prev"][e], st["prev"][e])
        if random_init:
            assert (got["prev"] != st["prev"]).any()
    print(f"T {T}: max |value - restatement| over {len(sc.commit_launches(T))} launches {worst:.3e} (bound {VALUE_ATOL:.0e})")


def test_commit_forced_at_step_zero_commits_nothing():
    st, _ = sc.build_commit(3, 3, 0.9, 3)
    st["forced"][:], st["ep_len"][:], st["done"][:] = 1, 0, 0
    st["r_flags"][st["r_flags"] == sc.PENDING] = 0
    want, got, _ = _check_commit(st, 0, "step 0")
    assert np.all(got["episode_value"] == 0.0) and np.all(got["ep_len"] == 0)
    for k in ("r_flags", "r_value", "r_reward"):
        assert same_bits(got[k], st[k]), k


@pytest.mark.parametrize("key", ["high-counter", "huge-counter", "high-seed", "max-depth"])
def test_commit_draws_with_the_high_words(key):
    """tie_u and the next episode's first waypoint at a global env id of 4096 and more, a seed of 2^32 and more, depth 2^20 - 1."""
    c = sc.RECORD_CASES[key]
    for random_init in (0, 1):
        st, _ = sc.build_commit(5, 3, 0.97, 13, random_init, seed=c["seed"], row_offset=c["row_offset"],
                                depth=c["depths"][-1] if key == "max-depth" else None)
        _check_commit(st, 13, (key, random_init))


# ---------------------------------------------------------------------------------------------------- gather
def _check_gather(got, want, label):
    for k in ("policy", "mask", "value", "reward", "index", "offsets", "states"):
        if k not in want:
            continue
        if want[k] is None:
            assert got[k] is None, (label, k)
        else:
            assert same_bits(got[k], want[k]), (label, k)


@pytest.mark.parametrize("side", sc.GATHER_SIDES)
def test_gather_planes(side):
    cfg = sc.GATHER_CONFIG[side]
    st, planes = sc.build_ring(6, 5, 5, 7, side=side)
    st["r_flags"][4] = sc.PENDING  # (one row that no draw may return)
    ring = sc.SyntheticRing(st, planes)
    want = sc.gather_ref(st, planes, cfg["n"], cfg["copies"], cfg["seed"], cfg["draw"])
    got = ring.gather(cfg["n"], cfg["copies"], cfg["seed"], cfg["draw"])
    _check_gather(got, want, side)
    assert 4 not in got["index"] and len(np.unique(got["index"])) > 1
    if side >= 3:  # the special values went through, and the copies are shifted
        assert np.isnan(got["states"]).any() and np.isinf(got["states"]).any() and (sc.bits(got["states"]) == 0x80000000).any()
        assert len(np.unique(sc.bits(got["states"]).reshape(len(got["index"]), -1), axis=0)) >= 9


@pytest.mark.parametrize("kmax,K,A", sc.DENSE_CASES)
def test_gather_dense_policy_and_mask_without_planes(kmax, K, A):
    st, _ = sc.build_ring(8, kmax, K, A)
    ring = sc.SyntheticRing(st)  # channels = 0: null planes and states
    want = sc.gather_ref(st, None, 9, 2, 5, 1)
    got = ring.gather(9, 2, 5, 1)
    _check_gather(got, want, (kmax, K, A))
    rows = np.array([0, 1, 7, 0, 3, 1])
    got = ring.gather_rows(rows)
    _check_gather(got, sc.gather_rows_ref(st, None, rows), (kmax, K, A, "rows"))
    assert got["mask"][0, 0] == 1 and got["mask"][1, A - 1] == 1 and got["mask"][0].sum() == K
    assert ((got["mask"] == 1) & (got["policy"] == 0)).sum() == len(rows)  # the exact 0 of every row: mask 1, policy 0


@pytest.mark.parametrize("case", sc.DRAW_CASES, ids=lambda c: f"{c['cap']}-{c['pattern']}-{c['n']}")
def test_gather_draws(case):
    st, planes = sc.build_ring(case["cap"], 5, 5, 7, side=3, pattern=case["pattern"])
    ring = sc.SyntheticRing(st, planes)
    copies = 1 + case["draw"] % 3
    want = sc.gather_ref(st, planes, case["n"], copies, sc.DRAW_SEED, case["draw"])
    got = ring.gather(case["n"], copies, sc.DRAW_SEED, case["draw"])
    _check_gather(got, want, case)
    committed = np.nonzero(st["r_flags"] == sc.COMMITTED)[0]
    if case["pattern"] == "none":
        assert np.all(got["index"] == -1) and np.isnan(got["value"]).all() and np.isnan(got["reward"]).all()
        assert np.isnan(got["states"]).all() and not got["policy"].any() and not got["mask"].any()
    else:
        assert np.all(np.isin(got["index"], committed))
        if case["ends"]:
            assert committed[0] in got["index"] and committed[-1] in got["index"]


@pytest.mark.parametrize("side", [6, 8])
def test_gather_rows(side):
    st, planes = sc.build_ring(16, 65, 64, 300, side=side, pattern="every-other")
    ring = sc.SyntheticRing(st, planes)
    cap = 16
    rows = np.array([3, -1, cap, 3, cap + 7, 0, 15, 15, 3, -5])  # (pending and free rows are served too: the caller drew them)
    got = ring.gather_rows(rows)
    _check_gather(got, sc.gather_rows_ref(st, planes, rows), side)
    for o in (1, 2, 4, 9):
        assert np.all(sc.bits(got["states"][o]) == 0x7fc00000) and np.isnan(got["value"][o]) and not got["mask"][o].any()


def test_refusals_launch_nothing():
    import ctypes as C

    st, planes = sc.build_ring(6, 5, 5, 7, side=4)
    ring = sc.SyntheticRing(st, planes)
    before = ring.download()
    sentinel = lambda out: all(np.all(v == 7) or np.all(v == -7) for v in out.values() if v is not None)  # noqa: E731
    for n, copies, kw in ((0, 1, {}), (1, 0, {}), (2, 2, dict(channels=2, side=4, planes=None))):
        rc, out = ring.gather_rc(n, copies, 5, 0, **kw)
        assert rc == -1 and sentinel(out), (n, copies, kw)
    pol = np.full((st["B"], st["kmax"]), 0.2)
    vidx = np.tile(np.arange(5, dtype=np.int32), (st["B"], 1))
    assert ring.record_rc(-1, pol, pol, vidx, np.ones(st["B"], np.int32)) == -1 and ring.commit_rc(-1) == -1
    for kmax in (0, sc.MAX_KMAX + 1):
        ring.sp.kmax = kmax
        assert ring.gather_rc(1, 1, 5, 0)[0] == -1 and ring.commit_rc(0) == -1
        assert ring.record_rc(0, pol, pol, vidx, np.ones(st["B"], np.int32)) == -1
    ring.sp.kmax = st["kmax"]
    after = ring.download()
    for k in sc.STATE_ARRAYS:
        assert same_bits(before[k], after[k]), k
    rc, out = ring.gather_rc(2, 2, 5, 0)  # ... and the same ring serves a proper call
    assert rc == 0 and not sentinel(out)
