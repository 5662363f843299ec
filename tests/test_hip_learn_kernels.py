"""
GPU tests of the learn loop's kernels on bare rings (tests/selfplay_cases.py, tests/learn_cases.py), against the host restatements of
planning/mcts_zero/selfplay.py that tests/test_learn_host.py pins:
  * ipp_selfplay_commit_iter (k_sp_commit_iter, csrc/k_selfplay.h) against commit_iter_host: episodes of 0, 1, horizon and horizon + 1
    rows, ended by done and forced and running on, with 0, cap - 1 and cap episodes counted before -- every array bit for bit, and what
    commit_ref defines wherever the iteration rule changes nothing; ipp_selfplay_commit on the same inputs still equals commit_ref;
  * ipp_selfplay_iter_totals (csrc/k_learn.h) for 1, 63, 64, 65 and 300 envs with value sums of mixed magnitude: the record bit for bit;
  * ipp_replay_priority_reset_window for rings of 1, 255, 256 and 257 rows and windows that are empty, partial and full; rows re-opened
    (pending) inside the window get 0;
  * every refused call leaves its outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

from tests import learn_cases as lc
from tests import selfplay_cases as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ITER_ARRAYS = ("iter_episodes", "r_iter", "examples", "value_sum")
COMMIT_FIELDS = ("r_reward", "r_value", "r_flags", "ep_len", "prev", "episode_value", "forced", "tie_u")


class IterRing(sc.SyntheticRing):
    """A SyntheticRing with the arrays of an ipp_selfplay_iter."""

    def __init__(self, state, it):
        super().__init__(state)
        self.it_t = {k: self.up(it[k]) for k in ITER_ARRAYS}
        self.it = self.ffi.IppSelfPlayIter(iteration=int(it["iteration"]), episode_cap=int(it["episode_cap"]),
                                           **{k: v.data_ptr() for k, v in self.it_t.items()})

    def commit_iter_rc(self, step, it="own"):
        return self.lib.ipp_selfplay_commit_iter(C.byref(self.sp), int(step), C.byref(self.it) if it == "own" else it, self.stream)

    def download_all(self):
        out = self.download()
        out.update({k: v.cpu().numpy() for k, v in self.it_t.items()})
        return out

    def totals_rc(self, out, it="own"):
        return self.lib.ipp_selfplay_iter_totals(C.byref(self.sp), C.byref(self.it) if it == "own" else it,
                                                 None if out is None else out.data_ptr(), self.stream)


def _same(got, want, keys):
    for k in keys:
        assert got[k].dtype == np.asarray(want[k]).dtype or got[k].dtype.itemsize == np.asarray(want[k]).dtype.itemsize, k
        assert np.array_equal(sc.bits(got[k]), sc.bits(np.asarray(want[k]))), k


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("T,step", lc.COMMIT_CASES)
def test_commit_iter_equals_its_restatement(T, step, shift):
    from ipp_rl_amd.planning.mcts_zero.selfplay import commit_iter_host

    state, episodes, it = lc.build(T, step, shift)
    want = commit_iter_host(state, step, it)
    ring = IterRing(state, it)
    ring.ffi.check(ring.commit_iter_rc(step))
    got = ring.download_all()
    _same(got, want, COMMIT_FIELDS + ITER_ARRAYS)
    ref = sc.commit_ref(state, step)  # (everything the plain commit defines and the iteration rule does not change)
    _same(got, ref, ("r_reward", "ep_len", "prev", "episode_value", "forced", "tie_u"))
    kept = [e for e, (Te, kind) in enumerate(episodes) if kind != "on" and it["iter_episodes"][e] < lc.CAP]
    dropped = [e for e, (Te, kind) in enumerate(episodes) if kind != "on" and it["iter_episodes"][e] >= lc.CAP]
    assert kept and dropped
    for e in kept:
        rows = sc.episode_rows(step, episodes[e][0], episodes[e][1] == "forced", state["S"], state["B"], e)
        assert np.array_equal(sc.bits(got["r_value"][rows]), sc.bits(ref["r_value"][rows])) and np.all(got["r_flags"][rows] == sc.COMMITTED)
        assert np.all(got["r_iter"][rows] == lc.ITERATION)
    for e in dropped:
        rows = sc.episode_rows(step, episodes[e][0], episodes[e][1] == "forced", state["S"], state["B"], e)
        assert np.all(got["r_flags"][rows] == 0) and np.array_equal(got["r_iter"][rows], it["r_iter"][rows])
        assert np.array_equal(sc.bits(got["r_value"][rows]), sc.bits(state["r_value"][rows]))
    # the plain commit on the same inputs is what it was
    plain = sc.SyntheticRing(sc.copy_state(state))
    _same(plain.commit(step), ref, COMMIT_FIELDS)


@pytest.mark.parametrize("B", lc.TOTALS_B)
def test_iteration_totals_bit_for_bit(B):
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import iter_totals_host

    n, ex, vs, cap = lc.totals_inputs(B)
    state = sc.make_state(B, 1, 1, 4)
    ring = IterRing(state, dict(iteration=0, episode_cap=cap, iter_episodes=n, r_iter=np.full(B, -1, np.int32), examples=ex, value_sum=vs))
    out = torch.full((4,), -7, dtype=torch.int64, device=ring.dev)
    ring.ffi.check(ring.totals_rc(out))
    again = torch.full((4,), -7, dtype=torch.int64, device=ring.dev)
    ring.ffi.check(ring.totals_rc(again))
    rec = out.cpu().numpy()
    want = iter_totals_host(n, ex, vs, cap)
    assert rec[:3].tolist() == [want["episodes_kept"], want["envs_at_cap"], want["examples"]]
    assert rec[3:4].view(np.uint64)[0] == np.array([want["value_sum"]]).view(np.uint64)[0], (rec[3:4].view(np.float64)[0], want["value_sum"])
    assert np.array_equal(rec, again.cpu().numpy())
    _same(ring.download_all(), dict(iter_episodes=n, examples=ex, value_sum=vs), ("iter_episodes", "examples", "value_sum"))  # (read only)


class WindowRing:
    """An ipp_selfplay with nothing but flags, and the tags: what the windowed reset reads."""

    def __init__(self, flags, tags):
        import torch

        from ipp_rl_amd import _ffi

        self.torch, self.ffi, self.lib = torch, _ffi, _ffi.load()
        self.dev = torch.device("cuda:0")
        self.rows = len(flags)
        self.flags = torch.as_tensor(np.asarray(flags, np.uint8), device=self.dev)
        self.tags = torch.as_tensor(np.asarray(tags, np.int32), device=self.dev)
        self.sp = _ffi.IppSelfPlay(num_envs=self.rows, slots=1, device=0, r_flags=self.flags.data_ptr())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.priority = torch.full((self.rows,), -3.0, dtype=torch.float64, device=self.dev)
        self.count = torch.full((1,), 99, dtype=torch.int64, device=self.dev)

    def reset_rc(self, lo, hi, tags="own", priority="own", count="own"):
        ptr = lambda x, own: own.data_ptr() if isinstance(x, str) else x  # noqa: E731
        return self.lib.ipp_replay_priority_reset_window(C.byref(self.sp), ptr(tags, self.tags), int(lo), int(hi), ptr(priority, self.priority),
                                                         ptr(count, self.count), self.stream)


@pytest.mark.parametrize("window", sorted(lc.WINDOWS))
@pytest.mark.parametrize("cap", lc.WINDOW_CAPS)
def test_windowed_priority_reset(cap, window):
    from ipp_rl_amd.planning.mcts_zero.selfplay import window_rows_host

    flags, tags = lc.window_inputs(cap)
    lo, hi = lc.WINDOWS[window]
    ring = WindowRing(flags, tags)
    ring.ffi.check(ring.reset_rc(lo, hi))
    rows = window_rows_host(flags, tags, lo, hi)
    L = len(rows)
    assert (L == 0) == (window == "empty")
    want = np.zeros(cap)
    if L:
        want[rows] = 1.0 / L
    pri = ring.priority.cpu().numpy()
    assert int(ring.count.cpu().numpy()[0]) == L and np.array_equal(sc.bits(pri), sc.bits(want))
    if cap > 1:
        assert np.all(pri[5:8] == 0.0) and pri[4] == 0.0  # (pending rows inside the window; a committed row that never saw an iteration)
    # against the whole-ring reset: the window of every tag, -1 included, is the committed rows
    ring.ffi.check(ring.reset_rc(-1, 3))
    whole = ring.torch.full((cap,), -3.0, dtype=ring.torch.float64, device=ring.dev)
    cnt = ring.torch.zeros((1,), dtype=ring.torch.int64, device=ring.dev)
    ring.ffi.check(ring.lib.ipp_replay_priority_reset(C.byref(ring.sp), whole.data_ptr(), cnt.data_ptr(), ring.stream))
    assert np.array_equal(sc.bits(ring.priority.cpu().numpy()), sc.bits(whole.cpu().numpy())) and int(cnt.cpu()[0]) == int(ring.count.cpu()[0])


def test_refused_calls_leave_their_outputs_untouched():
    import torch

    state, episodes, it = lc.build(lc.HORIZON, lc.HORIZON, 0)
    ring = IterRing(sc.copy_state(state), it)
    before = ring.download_all()
    ffi = ring.ffi

    def variant(**over):
        v = ffi.IppSelfPlayIter(iteration=ring.it.iteration, episode_cap=ring.it.episode_cap, iter_episodes=ring.it.iter_episodes,
                                r_iter=ring.it.r_iter, examples=ring.it.examples, value_sum=ring.it.value_sum)
        for k, x in over.items():
            setattr(v, k, x)
        return C.byref(v)

    bad = [variant(episode_cap=0), variant(episode_cap=-2)] + [variant(**{k: None}) for k in ITER_ARRAYS]
    out = torch.full((4,), -7, dtype=torch.int64, device=ring.dev)
    for b in bad + [None]:
        assert ring.commit_iter_rc(lc.HORIZON, it=b) == -1
        assert ring.totals_rc(out, it=b) == -1
    assert ring.commit_iter_rc(-1) == -1 and ring.totals_rc(None) == -1
    assert ring.lib.ipp_selfplay_commit_iter(None, 3, C.byref(ring.it), ring.stream) == -1
    no_ring = ffi.IppSelfPlay(num_envs=0, slots=1, device=0)
    assert ring.lib.ipp_selfplay_iter_totals(C.byref(no_ring), C.byref(ring.it), out.data_ptr(), ring.stream) == -1
    after = ring.download_all()
    _same(after, before, sc.STATE_ARRAYS + ITER_ARRAYS)
    assert out.cpu().numpy().tolist() == [-7] * 4

    flags, tags = lc.window_inputs(257)
    w = WindowRing(flags, tags)
    assert w.reset_rc(3, 2) == -1 and b"lo > hi" in w.lib.ipp_last_error()
    assert w.reset_rc(0, 3, tags=None) == -1 and w.reset_rc(0, 3, priority=None) == -1 and w.reset_rc(0, 3, count=None) == -1
    assert w.lib.ipp_replay_priority_reset_window(None, w.tags.data_ptr(), 0, 3, w.priority.data_ptr(), w.count.data_ptr(), w.stream) == -1
    torch.cuda.synchronize()
    assert np.all(w.priority.cpu().numpy() == -3.0) and int(w.count.cpu()[0]) == 99
