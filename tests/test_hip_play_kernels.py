"""
GPU tests of ipp_play_pick / ipp_play_tally / ipp_play_totals (csrc/k_play.h) on bare buffers, no engine, against the host restatements
of planning/vec_mcts_zero.py (which tests/test_vec_mcts_zero_host.py holds to the reference's literal expressions):
  * the pick at the wave64 tile edges of kmax, for 1 and 3 workers and both tie rules: distinct maxima, exact ties, a worker without a
    policy, and every way a row has no decision (no worker ok, a NaN, zero mass, a valid index that is no action); action_idx, forced,
    budget and action exactly, the ensemble bit for bit, two runs bit for bit;
  * the tally over seven scripted steps: game values within 1e-12 (the tolerance of the self-play value targets), steps, game counts and
    the retire rule exactly, the next tie uniform; the totals in their fixed order bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SEED, OFFSET, A = 11, 7, 300


def host(t):
    return t.detach().cpu().numpy()


class Bare:
    """An ipp_play on freshly made device buffers."""

    def __init__(self, B, workers, kmax, games_per_env, tie_rule, gamma=0.9, with_ensemble=True):
        import torch

        from ipp_rl_amd import _ffi

        self.torch, self.lib = torch, _ffi.load()
        dev = torch.device("cuda:0")
        rs = np.random.RandomState(1)
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
        self.actions = t(rs.random_sample((A, 3)) * 100.0, torch.float64)
        self.budget = t(np.full(B, 40.0), torch.float64)
        self.depth = t(np.arange(B) % 4, torch.int32)
        self.episode = t(np.arange(B) // 2, torch.int64)
        self.done = t(np.zeros(B), torch.uint8)
        self.prev = t(rs.random_sample((B, 3)) * 100.0, torch.float64)
        self.reward = t(np.zeros(B), torch.float32)
        self.ret, self.steps, self.games = t(np.zeros(B), torch.float64), t(np.zeros(B), torch.int32), t(np.zeros(B), torch.int32)
        self.forced = t(np.full(B, 7), torch.uint8)
        self.tie_u = t(np.zeros(B), torch.float64)
        self.action = t(np.full((B, 3), -1.0), torch.float64)
        self.action_idx = t(np.full(B, -9), torch.int32)
        self.game_value = t(np.zeros((B, games_per_env)), torch.float64)
        self.game_steps = t(np.zeros((B, games_per_env)), torch.int32)
        self.ensemble = t(np.full((B, kmax), -3.0), torch.float64) if with_ensemble else None
        self.pl = _ffi.IppPlay(num_envs=B, workers=workers, kmax=kmax, num_actions=A, games_per_env=games_per_env, tie_rule=tie_rule, device=0,
                               reserved=0, gamma=gamma, seed=SEED, row_offset=OFFSET)
        for name, _ in _ffi.IppPlay._fields_[11:]:
            buf = getattr(self, name)
            setattr(self.pl, name, buf.data_ptr() if buf is not None else None)
        self.B, self.check = B, _ffi.check

    def pick(self, pol, vi, ok):
        self.check(self.lib.ipp_play_pick(C.byref(self.pl), pol.data_ptr(), vi.data_ptr(), ok.data_ptr(), None))
        self.torch.cuda.synchronize()

    def tally(self):
        self.check(self.lib.ipp_play_tally(C.byref(self.pl), None))

    def totals(self):
        out = self.torch.zeros(4, dtype=self.torch.float64, device="cuda:0")
        self.check(self.lib.ipp_play_totals(C.byref(self.pl), out.data_ptr(), None))
        self.torch.cuda.synchronize()
        return host(out)


def _pick_case(workers, kmax, bad):
    """policy [5 W][kmax], valid_idx, ok for the five envs (see the module docstring); dyadic values: every sum is exact."""
    rs = np.random.RandomState(100 * workers + kmax)
    B, W = 5, workers
    pol = np.zeros((B, W, kmax))
    vi = np.full((B, W, kmax), -1, dtype=np.int32)
    ok = np.ones((B, W), dtype=np.int32)
    for e in range(B):
        K = kmax if e < 4 else max(1, (2 * kmax) // 3)  # env 4: the -1 padding starts in the middle of a tile
        idx = np.sort(rs.choice(A, size=K, replace=False))
        vi[e, :, :K] = idx
        pol[e, :, :K] = rs.randint(0, 8, size=(W, K)) / 64.0
        pol[e, 0, rs.randint(K)] += 1 / 64.0  # (mass somewhere)
    if kmax >= 2:  # env 0: one maximum, in the last slot (the last tile's last lane in use)
        pol[0, :, kmax - 1] = 1.0
    # env 1: exact ties of the summed values in every tile (the workers' shares differ, their sums do not)
    tie_slots = sorted({0, kmax // 2, kmax - 1})
    pol[1] = 0.0
    for s in tie_slots:
        share = rs.multinomial(12, np.ones(W) / W)
        pol[1, :, s] = share / 16.0
    # env 2: worker 0 has no policy; its row is garbage that must not be read as one
    ok[2, 0] = 0
    pol[2, 0] = np.nan
    vi[2, 0] = -1
    # env 3: no decision
    if bad == "none_ok":
        ok[3] = 0
    elif bad == "nan":
        pol[3, W - 1, kmax // 2] = np.nan
    elif bad == "zero":
        pol[3] = 0.0
    elif bad == "index":
        vi[3, :, :] = np.where(vi[3] >= 0, vi[3] + A, -1)
    # env 4: a hole of -1 inside the valid slots too
    if kmax >= 3:
        vi[4, :, 1] = -1
        pol[4, :, 1] = 5.0  # (not on the valid set: ignored)
        pol[4, 0, 0] += 1 / 64.0
    return pol.reshape(B * W, kmax), vi.reshape(B * W, kmax), ok.reshape(B * W)


@pytest.mark.parametrize("kmax", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("workers", [1, 3])
@pytest.mark.parametrize("tie_rule", [0, 1])
def test_pick_equals_the_host_restatement(workers, kmax, tie_rule):
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import ARGMAX_STREAM, step_uniform
    from ipp_rl_amd.planning.vec_mcts_zero import ensemble_pick_host

    B, W = 5, workers
    tied = 0
    for bad in ("none_ok", "nan", "zero", "index"):
        pol, vi, ok = _pick_case(W, kmax, bad)
        runs = []
        for _ in range(2):
            b = Bare(B, W, kmax, 1, tie_rule)
            b.pick(torch.as_tensor(pol, device="cuda:0"), torch.as_tensor(vi, device="cuda:0"), torch.as_tensor(ok, device="cuda:0"))
            runs.append({k: host(getattr(b, k)) for k in ("action_idx", "forced", "budget", "action", "ensemble")})
        got = runs[0]
        assert all(np.array_equal(runs[0][k], runs[1][k], equal_nan=True) for k in got)
        u = step_uniform(ARGMAX_STREAM, SEED, np.arange(B) + OFFSET, host(b.episode), host(b.depth))
        actions, prev = host(b.actions), host(b.prev)
        for e in range(B):
            rows = slice(e * W, (e + 1) * W)
            want = ensemble_pick_host(pol[rows], vi[rows], ok[rows], tie_rule, u[e], num_actions=A)
            assert got["action_idx"][e] == want["action_idx"] and got["forced"][e] == want["forced"], (bad, e)
            assert np.array_equal(got["ensemble"][e], want["ensemble"]), (bad, e)  # bit for bit
            if want["forced"]:
                assert got["budget"][e] == 0.0 and np.array_equal(got["action"][e], prev[e])
            else:
                assert got["budget"][e] == 40.0 and np.array_equal(got["action"][e], actions[want["action_idx"]])
                tied += int((want["ensemble"] == want["ensemble"].max()).sum() > 1)
        forced_want = [0, 0, 1 if W == 1 else 0, 1, 0]
        assert got["forced"].tolist() == forced_want, bad
        if kmax >= 2:
            assert got["action_idx"][0] == vi[0, kmax - 1]
    assert tied > 0 or kmax == 1  # (env 1's ties were ties)


def test_pick_without_an_ensemble_buffer():
    import torch

    pol, vi, ok = _pick_case(3, 65, "zero")
    a, b = Bare(5, 3, 65, 1, 0), Bare(5, 3, 65, 1, 0, with_ensemble=False)
    for x in (a, b):
        x.pick(torch.as_tensor(pol, device="cuda:0"), torch.as_tensor(vi, device="cuda:0"), torch.as_tensor(ok, device="cuda:0"))
    assert np.array_equal(host(a.action_idx), host(b.action_idx)) and np.array_equal(host(a.forced), host(b.forced))


@pytest.mark.parametrize("games_per_env", [1, 2])
def test_tally_and_totals_over_scripted_steps(games_per_env):
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import TIE_STREAM, step_uniform
    from ipp_rl_amd.planning.vec_mcts_zero import tally_host, totals_host

    B, G, gamma = 4, games_per_env, 0.9
    rs = np.random.RandomState(5)
    reward = rs.random_sample((7, B)).astype(np.float32)
    #                 env 0          env 1 (forced end)  env 2 (three episodes)  env 3 (never ends)
    done = np.array([[0, 0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 0, 1, 0], [0, 1, 0, 1, 0, 1, 0], [0] * 7], dtype=np.uint8).T
    forced = np.array([[0] * 7, [0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0], [0] * 7], dtype=np.uint8).T
    b = Bare(B, 1, 4, G, 1, gamma=gamma)
    gid = np.arange(B) + OFFSET
    for t in range(7):
        b.reward.copy_(torch.as_tensor(reward[t]))
        b.done.copy_(torch.as_tensor(done[t]))
        b.forced.copy_(torch.as_tensor(forced[t]))
        b.depth.copy_(torch.as_tensor(((np.arange(B) + t) % 5).astype(np.int32)))
        b.episode.copy_(torch.as_tensor((np.arange(B) + t // 2).astype(np.int64)))
        b.tally()
        tot = b.totals()
        gv, gs, games = host(b.game_value), host(b.game_steps), host(b.games)
        for e in range(B):
            want = tally_host(reward[:t + 1, e], done[:t + 1, e], forced[:t + 1, e], gamma, G)
            n = want["games"]
            assert games[e] == n and gs[e, :n].tolist() == want["game_steps"] and np.all(gs[e, n:] == 0)
            np.testing.assert_allclose(gv[e, :n], want["game_value"], rtol=0, atol=1e-12)
            assert np.all(gv[e, n:] == 0.0)
            np.testing.assert_allclose(host(b.ret)[e], want["ret"], rtol=0, atol=1e-12)
            assert host(b.steps)[e] == want["steps"]
        assert np.array_equal(tot, totals_host(gv, gs, games))  # bit for bit: (env, game) order
        seq = 0.0
        for e in range(B):
            for g in range(games[e]):
                seq += gv[e, g]
        assert tot[0] == seq and tot[1] == games.sum() and tot[3] == (games == G).sum()
        assert np.array_equal(host(b.tie_u), step_uniform(TIE_STREAM, SEED, gid, host(b.episode), host(b.depth)))
    games = host(b.games)
    assert games.tolist() == [min(2, G), min(3, G), min(4, G), 0]  # (retired envs play on, uncounted; env 3 has no game)


def test_totals_past_one_wave_of_items():
    """80 items: partial sums of two items each, added in lane order -- the restatement's order, bit for bit."""
    import torch

    from ipp_rl_amd.planning.vec_mcts_zero import totals_host

    B, G = 40, 2
    rs = np.random.RandomState(9)
    b = Bare(B, 1, 4, G, 0)
    gv, gs = rs.random_sample((B, G)) * 10.0 ** rs.randint(-3, 4, size=(B, G)), rs.randint(1, 7, size=(B, G)).astype(np.int32)
    games = rs.randint(0, G + 1, size=B).astype(np.int32)
    b.game_value.copy_(torch.as_tensor(gv))
    b.game_steps.copy_(torch.as_tensor(gs))
    b.games.copy_(torch.as_tensor(games))
    got = [b.totals() for _ in range(2)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], totals_host(gv, gs, games))
    assert got[0][1] == games.sum() and got[0][3] == (games == G).sum()
