"""
The cases of tests/test_hip_selfplay_kernels.py (GPU) and tests/test_selfplay_cases_host.py (CPU): csrc/k_selfplay.h's record, commit
and gather kernels on bare rings, with no engine and no search behind them.

  * case tables (RECORD_CASES, COMMIT_*, GATHER_*, DENSE_CASES, DRAW_CASES): every input is drawn from the seeds frozen here;
  * SyntheticRing: an _ffi.IppSelfPlay whose pointers are plain torch tensors uploaded from a state of NumPy arrays (make_state); the
    env fields (budget, depth, episode, done, prev, reward) are set the way an env step would leave them;
  * record_ref / commit_ref / gather_ref / gather_rows_ref: fp64 NumPy restatements of the three calls, composed from the functions of
    planning/mcts_zero/selfplay.py that tests/test_selfplay_host.py pins to the reference (step_uniform, init_action_index,
    inverse_cdf, value_targets, replay_draws, shift_planes).  They work on whole arrays per env: no ballots, no binary search, no lanes.

The module imports neither torch nor the package at import time (SyntheticRing and the restatements import them when called).
"""
import ctypes as C

import numpy as np

PENDING, COMMITTED = 1, 2
MAX_KMAX = 2048
STATE_ARRAYS = ("actions", "budget", "depth", "episode", "done", "prev", "reward", "ep_len", "forced", "tie_u", "episode_value", "action",
                "action_idx", "r_policy", "r_idx", "r_value", "r_reward", "r_flags")
F32_SPECIALS = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x80000000, 0x7f800000, 0xff800000], dtype=np.uint32).view(np.float32)
# (quiet NaNs with and without payload and sign, -0.0, +inf, -inf: a gather moves their bits)


def _sp():
    from ipp_rl_amd.planning.mcts_zero import selfplay

    return selfplay


def action_table(A):
    """actions [A][3]: distinct triples of small integers."""
    a = np.arange(A)
    return np.stack([a % 61, a // 61, 5 + a % 7], axis=1).astype(np.float64)


def make_state(B, S, kmax, A, horizon=3, temp_threshold=3, temp_zero=0, random_init=1, gamma=0.9, seed=3, row_offset=0, rng=0):
    """A ring of S x B rows and its env fields as NumPy arrays, every array filled with recognisable values (an earlier policy in
    every row, odd budgets): what a call leaves alone is visible as such."""
    rs = np.random.RandomState(rng)
    cap = B * S
    st = dict(B=B, S=S, kmax=kmax, A=A, horizon=horizon, temp_threshold=temp_threshold, temp_zero=temp_zero, random_init=random_init,
              gamma=gamma, seed=seed, row_offset=row_offset)
    st["actions"] = action_table(A)
    st["budget"] = 100.0 + np.arange(B, dtype=np.float64)
    st["depth"] = np.zeros(B, np.int32)
    st["episode"] = (rs.randint(0, 9, B)).astype(np.int64)
    st["done"] = np.zeros(B, np.uint8)
    st["prev"] = st["actions"][rs.randint(0, A, B)].copy()
    st["reward"] = rs.uniform(0, 0.05, B).astype(np.float32)
    st["ep_len"] = np.zeros(B, np.int32)
    st["forced"] = np.zeros(B, np.uint8)
    st["tie_u"] = np.full(B, -1.0)
    st["episode_value"] = np.full(B, -2.0)
    st["action"] = np.full((B, 3), -3.0)
    st["action_idx"] = np.full(B, -9, np.int32)
    st["r_policy"] = rs.uniform(0.25, 0.5, (cap, kmax)).astype(np.float32)
    st["r_idx"] = np.full((cap, kmax), -1, np.int32)
    st["r_value"] = rs.uniform(-1, 1, cap)
    st["r_reward"] = rs.uniform(0, 0.05, cap)
    st["r_flags"] = rs.randint(0, 3, cap).astype(np.uint8)
    return st


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


class SyntheticRing:
    """ipp_selfplay over plain tensors: upload a state, call an entry point, read the state back."""

    def __init__(self, state, planes=None):
        import torch

        from ipp_rl_amd import _ffi

        self.torch, self.ffi, self.lib = torch, _ffi, _ffi.load()
        self.dev = torch.device("cuda:0")
        self.state = state
        self.t = {k: torch.as_tensor(np.ascontiguousarray(state[k]), device=self.dev) for k in STATE_ARRAYS}
        self.planes = None if planes is None else torch.as_tensor(np.ascontiguousarray(planes), device=self.dev)
        self.sp = _ffi.IppSelfPlay(num_envs=state["B"], slots=state["S"], kmax=state["kmax"], num_actions=state["A"],
                                   horizon=state["horizon"], temp_threshold=state["temp_threshold"], temp_zero=state["temp_zero"],
                                   random_init=state["random_init"], device=0, reserved=0, gamma=state["gamma"],
                                   seed=state["seed"] & (2 ** 64 - 1), row_offset=state["row_offset"])
        for k in STATE_ARRAYS:
            setattr(self.sp, k, self.t[k].data_ptr())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def download(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def record_rc(self, step, pol_t, pol_1, vidx, ok):
        self._keep = [self.up(np.asarray(pol_t, np.float64)), self.up(np.asarray(pol_1, np.float64)), self.up(np.asarray(vidx, np.int32)),
                      self.up(np.asarray(ok, np.int32))]
        return self.lib.ipp_selfplay_record(C.byref(self.sp), int(step), *[x.data_ptr() for x in self._keep], self.stream)

    def record(self, *args):
        self.ffi.check(self.record_rc(*args))
        return self.download()

    def commit_rc(self, step):
        return self.lib.ipp_selfplay_commit(C.byref(self.sp), int(step), self.stream)

    def commit(self, step):
        self.ffi.check(self.commit_rc(step))
        return self.download()

    def _outputs(self, rows, channels, side):
        torch, A = self.torch, self.state["A"]
        f = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=self.dev)  # noqa: E731
        return dict(states=f((rows, channels, side, side), torch.float32, 7.0) if channels else None, policy=f((rows, A), torch.float32, 7.0),
                    mask=f((rows, A), torch.uint8, 7), value=f((rows,), torch.float64, 7.0), reward=f((rows,), torch.float64, 7.0))

    def gather_rc(self, n, copies, seed, draw, channels=None, side=None, planes="own"):
        """ipp_replay_gather of minibatch number `draw`; returns (rc, outputs)."""
        torch = self.torch
        if channels is None:
            channels, side = (0, 0) if self.planes is None else self.planes.shape[1:3]
        cum = self.up(np.cumsum(self.state["r_flags"] == COMMITTED).astype(np.int32))
        rows = max(n, 1) * max(copies, 1)
        o = self._outputs(rows, channels, side)
        o["index"] = torch.full((rows,), -7, dtype=torch.int64, device=self.dev)
        o["offsets"] = torch.full((max(copies, 1), 2), -7, dtype=torch.int32, device=self.dev)
        pl = self.planes if planes == "own" else planes
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        rc = self.lib.ipp_replay_gather(C.byref(self.sp), n, copies, channels, side, ptr(pl), cum.data_ptr(), C.c_uint64(seed),
                                        C.c_uint64(_sp().REPLAY_STREAM + int(draw)), ptr(o["states"]), o["policy"].data_ptr(),
                                        o["mask"].data_ptr(), o["value"].data_ptr(), o["reward"].data_ptr(), o["index"].data_ptr(),
                                        o["offsets"].data_ptr(), self.stream)
        torch.cuda.synchronize()
        return rc, {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}

    def gather(self, n, copies, seed, draw):
        rc, out = self.gather_rc(n, copies, seed, draw)
        self.ffi.check(rc)
        return out

    def gather_rows(self, rows):
        channels, side = (0, 0) if self.planes is None else self.planes.shape[1:3]
        idx = self.up(np.asarray(rows, np.int64))
        o = self._outputs(len(rows), channels, side)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self.ffi.check(self.lib.ipp_replay_gather_rows(C.byref(self.sp), len(rows), channels, side, ptr(self.planes), idx.data_ptr(),
                                                       ptr(o["states"]), o["policy"].data_ptr(), o["mask"].data_ptr(), o["value"].data_ptr(),
                                                       o["reward"].data_ptr(), self.stream))
        self.torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


# ---------------------------------------------------------------------------------------------------- restatements
def argmax_pick(p, u):
    """Slot (within p) of the temperature-0 choice among the maxima of p at the uniform u, and the number of maxima."""
    ties = np.nonzero(p == p.max())[0]  # ascending slots
    return int(ties[min(int(u * len(ties)), len(ties) - 1)]), len(ties)


def has_mass(p):
    """The contract of a recordable policy on its valid set: no NaN, a finite positive maximum and a finite positive sum."""
    if len(p) == 0 or np.any(np.isnan(p)):
        return False
    tot = float(np.cumsum(p)[-1])
    return bool(0 < p.max() < np.inf and 0 < tot < np.inf)


def record_ref(state, step, pol_t, pol_1, vidx, ok):
    """ipp_selfplay_record: (policy [B][kmax] fp32, idx, flag of the step's ring rows; action_idx, action, ep_len, forced, budget)."""
    sp = _sp()
    B, S, kmax, A = state["B"], state["S"], state["kmax"], state["A"]
    rows = (step % S) * B + np.arange(B)
    out = dict(rows=rows, policy=state["r_policy"][rows].copy(), idx=state["r_idx"][rows].copy(), flag=state["r_flags"][rows].copy(),
               action_idx=state["action_idx"].copy(), action=state["action"].copy(), ep_len=state["ep_len"].copy(),
               forced=state["forced"].copy(), budget=state["budget"].copy(), slot=np.full(B, -1))
    gid = np.arange(B, dtype=np.int64) + state["row_offset"]
    for e in range(B):
        depth, ep = int(state["depth"][e]), int(state["episode"][e])
        valid = np.nonzero(vidx[e] >= 0)[0]
        t0 = bool(state["temp_zero"]) or depth >= state["temp_threshold"]
        p = np.asarray((pol_1 if t0 else pol_t)[e], np.float64)[valid]
        good = bool(ok[e]) and has_mass(p)
        if good:
            if t0:
                best, _ = argmax_pick(p, float(sp.step_uniform(sp.ARGMAX_STREAM, state["seed"], gid[e], ep, depth)))
                p = np.zeros(len(valid))
                p[best] = 1.0
            k = valid[sp.inverse_cdf(p, float(sp.step_uniform(sp.ACTION_STREAM, state["seed"], gid[e], ep, depth)))]
            a = int(vidx[e][k])
            good = 0 <= a < A
        if not good:  # ended like a root without a policy: no sample, the earlier row stays but is no committed sample any more
            out["forced"][e], out["budget"][e], out["action"][e], out["action_idx"][e], out["flag"][e] = 1, 0.0, state["prev"][e], -1, 0
            continue
        dense = np.zeros(kmax)
        dense[valid] = p
        out["policy"][e], out["idx"][e], out["flag"][e] = dense.astype(np.float32), vidx[e], PENDING
        out["action_idx"][e], out["action"][e], out["slot"][e] = a, state["actions"][a], k
        out["ep_len"][e] += 1
        out["forced"][e] = 0
    return out


def episode_rows(step, T, forced, S, B, e):
    """Ring rows of the T samples of env e's episode that ends at `step` (a forced end: its last sample is the step before)."""
    t_last = step - 1 if forced else step
    return np.array([((t_last - (T - 1 - j)) % S) * B + e for j in range(T)], dtype=np.int64)


def commit_ref(state, step):
    """ipp_selfplay_commit: r_reward, r_value, r_flags, episode_value (NaN: nothing ended), ep_len, prev, tie_u (and forced = 0)."""
    sp = _sp()
    B, S, A = state["B"], state["S"], state["A"]
    out = {k: state[k].copy() for k in ("r_reward", "r_value", "r_flags", "ep_len", "prev")}
    out["episode_value"] = np.full(B, np.nan)
    out["forced"] = np.zeros(B, np.uint8)
    gid = np.arange(B, dtype=np.int64) + state["row_offset"]
    for e in range(B):
        forced = bool(state["forced"][e])
        if not forced:
            out["r_reward"][(step % S) * B + e] = float(state["reward"][e])
        if forced or state["done"][e]:
            rows = episode_rows(step, int(state["ep_len"][e]), forced, S, B, e)
            vals, tot = sp.value_targets(out["r_reward"][rows], state["gamma"], state["horizon"])
            out["r_value"][rows], out["r_flags"][rows] = vals, COMMITTED
            out["episode_value"][e], out["ep_len"][e] = tot, 0
            if state["random_init"]:
                out["prev"][e] = state["actions"][int(sp.init_action_index(state["seed"], gid[e], int(state["episode"][e]), A))]
    out["tie_u"] = sp.step_uniform(sp.TIE_STREAM, state["seed"], gid, state["episode"], state["depth"])
    return out


def gather_rows_ref(state, planes, rows):
    """ipp_replay_gather_rows: the ring rows `rows` (outside [0, cap): the empty row) unshifted, policies and masks densified by a
    scatter.  states stay float32 (compare their bits)."""
    cap, A = state["B"] * state["S"], state["A"]
    rows = np.asarray(rows, dtype=np.int64)
    n = len(rows)
    out = dict(policy=np.zeros((n, A), np.float32), mask=np.zeros((n, A), np.uint8), value=np.full(n, np.nan), reward=np.full(n, np.nan),
               states=None)
    if planes is not None:
        out["states"] = np.full((n,) + planes.shape[1:], np.nan, np.float32)
    for o, r in enumerate(rows):
        if not 0 <= r < cap:
            continue
        idx, p = state["r_idx"][r], state["r_policy"][r]
        out["policy"][o, idx[idx >= 0]] = p[idx >= 0]
        out["mask"][o, idx[idx >= 0]] = 1
        out["value"][o], out["reward"][o] = state["r_value"][r], state["r_reward"][r]
        if planes is not None:
            out["states"][o] = planes[r]
    return out


def gather_ref(state, planes, n, copies, seed, draw):
    """ipp_replay_gather: minibatch number `draw` of n rows and its copies - 1 shifted copies, originals first."""
    sp = _sp()
    committed = np.nonzero(state["r_flags"] == COMMITTED)[0]
    rows, offs = sp.replay_draws(n, copies, seed, draw, committed if len(committed) else np.array([-1]))
    one = gather_rows_ref(state, planes, rows)
    out = {k: (None if v is None else np.concatenate([v] * copies)) for k, v in one.items()}
    if planes is not None:
        out["states"] = np.concatenate([sp.shift_planes(one["states"], offs[c]) for c in range(copies)])
    out["index"], out["offsets"] = np.tile(rows, copies), offs.astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------- record cases
B_RECORD = 64
HIGH_OFFSET = 3 * 4096 + 17       # (gid << 20) + depth >= 2^32 for every env
HUGE_OFFSET = (1 << 36) + 5
HIGH_SEED = (0x9E3779B9 << 32) | 0x12345
MAX_DEPTH = (1 << 20) - 1
# name -> kmax, the valid-set sizes (cycled over the 64 envs), what the policies look like (`layout`), temperature fields and keys
RECORD_CASES = {}


def _rc(name, kmax, Ks, layout, thr=3, temp_zero=0, depths=(2, 3), row_offset=0, seed=3, A=None, rng=None):
    RECORD_CASES[name] = dict(kmax=kmax, Ks=tuple(Ks), layout=layout, thr=thr, temp_zero=temp_zero, depths=tuple(depths),
                              row_offset=row_offset, seed=seed, A=A or max(2 * kmax, 8), rng=len(RECORD_CASES) + 11 if rng is None else rng)


for _k, _Ks in ((1, (1,)), (63, (1, 63, 30)), (64, (1, 64, 33)), (65, (1, 65, 64)), (130, (1, 130, 64, 65, 100)),
                (257, (1, 257, 64, 65, 200)), (2048, (1, 2048, 64, 65, 1500))):
    _rc(f"cdf-{_k}", _k, _Ks, "cdf")         # depth 2 = threshold - 1: pol_t; depth 3 = threshold: one-hot of pol_1
    _rc(f"ties-{_k}", _k, _Ks, "ties")
_rc("temp-zero-depth-0", 130, (1, 130, 64, 65, 100), "ties", temp_zero=1, depths=(0,))
_rc("high-counter", 130, (130, 65, 9), "ties", row_offset=HIGH_OFFSET)
_rc("huge-counter", 65, (65, 9), "cdf", row_offset=HUGE_OFFSET)
_rc("high-seed", 130, (130, 65, 9), "ties", seed=HIGH_SEED)
_rc("max-depth", 65, (65, 9), "ties", thr=MAX_DEPTH, depths=(MAX_DEPTH - 1, MAX_DEPTH), row_offset=HIGH_OFFSET)
_rc("refusals", 130, (130, 64, 5), "refusals")
TIE_CASES = tuple(n for n, c in RECORD_CASES.items() if c["layout"] == "ties")
REFUSAL_KINDS = ("ok0", "index>=A", "K=0", "zeros", "nan", "fine")


def refusal_kind(e):
    """What env e of the refusals case is (every kind at both depths and with every K)."""
    return REFUSAL_KINDS[(e // 6) % 6]


def build_record(name):
    """(state, step, pol_t, pol_1, vidx, ok) of a record case: 64 envs, ring of 3 step slots, step 7 (slot 1)."""
    c = RECORD_CASES[name]
    rs = np.random.RandomState(c["rng"])
    B, kmax, A = B_RECORD, c["kmax"], c["A"]
    st = make_state(B, 3, kmax, A, temp_threshold=c["thr"], temp_zero=c["temp_zero"], seed=c["seed"], row_offset=c["row_offset"], rng=c["rng"])
    st["depth"] = np.array([c["depths"][e % len(c["depths"])] for e in range(B)], np.int32)
    st["ep_len"] = (np.arange(B) % 5).astype(np.int32)
    st["forced"] = (np.arange(B) % 2).astype(np.uint8)
    pol_t, pol_1 = np.zeros((B, kmax)), np.zeros((B, kmax))
    vidx, ok = np.full((B, kmax), -1, np.int32), np.ones(B, np.int32)
    for e in range(B):
        q = e // len(c["depths"])
        K, var = c["Ks"][q % len(c["Ks"])], (q // len(c["Ks"])) % 8   # every K at every depth, every variant with every K
        ids = np.sort(rs.choice(A, K, replace=False))
        if e % 4 == 0:
            ids[0], ids[-1] = (0, 0) if K == 1 else (0, A - 1)  # the first and the last action
        vidx[e, :K] = ids
        # garbage on the padding: a kernel must not read a policy where the index is -1
        pol_t[e], pol_1[e] = rs.uniform(5, 6, kmax), rs.uniform(5, 6, kmax)
        pt, p1 = rs.uniform(0.01, 1, K), rs.uniform(0.01, 0.9, K)
        if c["layout"] in ("cdf", "refusals"):
            if var == 1 and K >= 3:      # zero mass on the leading and trailing valid slots
                pt[[0, 1, K - 1]] = 0.0
            elif var == 2:               # a single positive slot
                pt[:] = 0.0
                pt[rs.randint(K)] = 0.3
            elif var == 3:               # many slots of 1e-300 beside one of mass 1
                pt[:] = 1e-300
                pt[rs.randint(K)] = 1.0
            pt *= (1.0, 3.7, 0.01, 1.0)[q % 4] / (pt.sum() if var != 3 else 1.0)  # not every policy sums to 1
            p1 *= 0.9 / p1.sum()
            p1[(int(np.argmax(pt)) + 1) % K] = 0.95   # one maximum, elsewhere than pol_t's
        else:
            # pol_1: maxima on a chosen set of slots; pol_t's single maximum elsewhere (the wrong source shows)
            if var == 0 or K == 1:
                ties = [rs.randint(K)]                       # n_ties == 1
            elif var == 1:
                ties = np.arange(K)                          # n_ties == K
            elif var == 2:
                ties = np.arange(K)[::7]                     # through every ballot
            elif var == 3:
                ties = np.arange(K)[max(K - 70, 0)::3]       # the last ballots only
            elif var == 4:
                ties = np.arange(K)[K // 2:]                 # the upper half
            else:
                ties = np.sort(rs.choice(K, max(2, K // (var - 2)), replace=False)) if K > 1 else [0]
            p1[np.asarray(ties)] = 0.95
            pt /= pt.sum()
            pt[(int(np.asarray(ties)[0]) + 1) % K] = 2.0
        if c["layout"] == "refusals":
            kind = refusal_kind(e)
            if kind == "ok0":
                ok[e] = 0
            elif kind == "index>=A":     # all the mass on a slot whose index is not an action
                pt[:], p1[:] = 0.0, 0.0
                pt[K // 2] = p1[K // 2] = 1.0
                vidx[e, K // 2] = A + 3
            elif kind == "K=0":
                vidx[e], K = -1, 0
            elif kind == "zeros":
                pt[:], p1[:] = 0.0, 0.0
            elif kind == "nan":
                pt[K // 3], p1[K // 3] = np.nan, np.nan
        pol_t[e, :K], pol_1[e, :K] = pt[:K], p1[:K]
    return st, 7, pol_t, pol_1, vidx, ok


def tie_stats(name):
    """Per temperature-0 env of a record case: (ballot of the picked slot, its rank among the ties of that ballot, n_ties, K)."""
    sp = _sp()
    st, step, pol_t, pol_1, vidx, ok = build_record(name)
    gid = np.arange(st["B"], dtype=np.int64) + st["row_offset"]
    out = []
    for e in range(st["B"]):
        depth = int(st["depth"][e])
        if not (st["temp_zero"] or depth >= st["temp_threshold"]):
            continue
        K = int((vidx[e] >= 0).sum())
        p = pol_1[e, :K]
        slot, n = argmax_pick(p, float(sp.step_uniform(sp.ARGMAX_STREAM, st["seed"], gid[e], int(st["episode"][e]), depth)))
        rank = int((p[(slot // 64) * 64:slot] == p.max()).sum())
        out.append((slot // 64, rank, n, K))
    return out


# ---------------------------------------------------------------------------------------------------- commit cases
COMMIT_LENGTHS = (1, 2, 63, 64, 65, 130)
COMMIT_GAMMAS = (0.9, 0.97, 1.0)
B_COMMIT = 12
# env e of a commit launch: (length as a function of T, how the step ends it)
COMMIT_ENVS = (("T", "done"), ("T", "forced"), ("T", "on"), ("half", "done"), ("half", "forced"), ("1", "done"), ("T-1", "done"),
               ("T", "done"), ("T-1", "forced"), ("1", "on"), ("0", "forced"), ("T", "forced"))


def commit_horizons(T):
    return (0, 1, 3, T, T + 5)


def commit_steps(T):
    """Launch steps for episodes of up to T samples on a ring of S = T + 1 slots: at the first no episode wraps; at the others the long
    ones straddle slot S - 1 to 0 (at 2 S those ended by done, at 2 S + T // 2 the forced ones too)."""
    return (T, 2 * (T + 1), 2 * (T + 1) + T // 2)


def commit_launches(T):
    """(horizon, gamma, step, random_init) of the launches for length T: every horizon with every gamma, the steps and random_init in turn."""
    return [(h, g, commit_steps(T)[(hi + gi) % 3], (hi + gi) % 2) for hi, h in enumerate(commit_horizons(T)) for gi, g in enumerate(COMMIT_GAMMAS)]


def build_commit(T, horizon, gamma, step, random_init=1, seed=5, row_offset=0, depth=None, rng=0):
    """The state in front of a commit at `step`: every env's running episode pending in the ring with its earlier rewards, the
    record's ep_len and forced, the env step's reward, done, depth and episode.  Returns (state, episodes) with episodes[e] =
    (sample count, kind)."""
    B, S = B_COMMIT, T + 1
    rs = np.random.RandomState(1000 * T + 10 * horizon + int(100 * gamma) + step + rng)
    st = make_state(B, S, 1, 50, horizon=horizon, gamma=gamma, random_init=random_init, seed=seed, row_offset=row_offset, rng=T + rng)
    st["r_flags"][st["r_flags"] == PENDING] = 0   # (older rows: free or committed)
    st["depth"] = rs.randint(0, 200, B).astype(np.int32) if depth is None else np.full(B, depth, np.int32)
    st["episode"] = rs.randint(0, 1000, B).astype(np.int64)
    episodes = []
    for e, (length, kind) in enumerate(COMMIT_ENVS):
        Te = {"T": T, "half": max(T // 2, 1), "1": 1, "T-1": max(T - 1, 1), "0": 0}[length]
        forced = kind == "forced"
        assert step - (1 if forced else 0) - (Te - 1) >= 0, "the episode would start before step 0: out of bounds for the kernel"
        st["ep_len"][e], st["forced"][e], st["done"][e] = Te, forced, kind == "done"
        rows = episode_rows(step, Te, forced, S, B, e)
        st["r_flags"][rows] = PENDING
        st["r_reward"][rows] = rs.uniform(0, 0.05, Te).astype(np.float32).astype(np.float64)
        if forced:
            st["r_flags"][(step % S) * B + e] = 0   # (what the record left in the forced step's own slot)
        episodes.append((Te, kind))
    st["reward"] = rs.uniform(0, 0.05, B).astype(np.float32)
    return st, episodes


# ---------------------------------------------------------------------------------------------------- gather cases
GATHER_SIDES = (1, 3, 4, 6, 8, 18, 36)
ALL_OFFSETS = dict(n=3, copies=700, seed=21, draw=0)    # every (i, j) in [0, 8]^2 among its copies (asserted on the CPU)
FEW_OFFSETS = dict(n=3, copies=40, seed=21, draw=1)     # dx == 0 with dy != 0, dx == -4 and dx == +4 among its copies
GATHER_CONFIG = {1: ALL_OFFSETS, 3: ALL_OFFSETS, 4: ALL_OFFSETS, 6: ALL_OFFSETS, 8: ALL_OFFSETS, 18: FEW_OFFSETS, 36: FEW_OFFSETS}
DENSE_CASES = ((1, 1, 1), (5, 5, 7), (65, 64, 300), (257, 200, 5000), (2048, 2048, 4096))  # (kmax, K, A)
# (cap, committed pattern, n, draw): the rows of minibatch `draw`; where `ends` is set the first AND the last committed row are drawn
DRAW_CASES = tuple(dict(cap=cap, pattern=pat, n=n, draw=draw, ends=ends) for cap, pat, n, draw, ends in (
    (1, "all", 1, 0, True), (1, "none", 1, 0, False), (1, "all", 257, 1, True),
    (2, "first", 255, 0, True), (2, "last", 256, 0, True), (2, "all", 257, 0, True), (2, "all", 1, 2, False), (2, "none", 255, 0, False),
    (320, "first", 256, 0, True), (320, "last", 257, 0, True), (320, "every-other", 257, 2, True), (320, "every-other", 255, 1, False),
    (320, "all", 257, 6, True), (320, "all", 256, 1, False), (320, "none", 257, 0, False), (320, "all", 1, 3, False)))
DRAW_SEED = 77


def committed_pattern(cap, pattern):
    f = np.zeros(cap, np.uint8)
    if pattern == "first":
        f[0] = COMMITTED
    elif pattern == "last":
        f[cap - 1] = COMMITTED
    elif pattern == "every-other":
        f[1::2] = COMMITTED   # (an even count of committed rows; row 0 is not among them)
        f[0::4] = PENDING
    elif pattern == "all":
        f[:] = COMMITTED
    else:
        f[0::2] = PENDING
    return f


def build_ring(cap, kmax, K, A, side=0, channels=2, pattern="all", rng=0):
    """A filled ring of cap rows (num_envs x slots = cap) for the gathers: (state, planes or None).  Row r holds a valid set of K (row 0),
    or fewer, ascending actions with action 0 and action A - 1 in rows 0 and 1, an exact 0 among its probabilities, and planes with NaNs,
    -0.0 and infinities."""
    rs = np.random.RandomState(7919 * kmax + 31 * cap + side + rng)
    B = next(b for b in (32, 8, 2, 1) if cap % b == 0)
    st = make_state(B, cap // B, kmax, A, seed=DRAW_SEED, rng=kmax + cap)
    st["r_flags"] = committed_pattern(cap, pattern)
    st["r_policy"][:] = rs.uniform(0.1, 1, (cap, kmax)).astype(np.float32)   # (garbage on the padding too)
    for r in range(cap):
        Kr = K if r < 2 else int(rs.randint(1, K + 1))
        ids = np.sort(rs.choice(A, Kr, replace=False))
        if r < 2 and Kr >= 1:
            ids[0] = 0
            ids[-1] = A - 1 if Kr > 1 or r == 1 else ids[-1]
            ids = np.unique(ids)
            Kr = len(ids)
        st["r_idx"][r, :Kr] = ids
        st["r_policy"][r, rs.randint(Kr)] = 0.0   # an exact 0 on a valid slot: mask 1, policy 0
    planes = None
    if side:
        planes = rs.standard_normal((cap, channels, side, side)).astype(np.float32)
        flat = planes.reshape(-1)
        where = rs.choice(flat.size, max(flat.size // 9, min(flat.size, len(F32_SPECIALS))), replace=False)
        flat[where] = np.resize(F32_SPECIALS, len(where))
    return st, planes


def offsets_of(cfg):
    """[copies][2] shift offsets of a gather configuration."""
    return _sp().replay_draws(cfg["n"], cfg["copies"], cfg["seed"], cfg["draw"], np.arange(1))[1]


def bits(a):
    """An array's bits as unsigned integers (floats compared as stored: NaN payloads, -0.0)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])
