"""
The cases of tests/test_hip_mcts_tables.py (GPU) and tests/test_mcts_tables_host.py (CPU): csrc/k_mcts.h's select, backup and read-out
kernels on bare tables, with no engine and no search behind them.

  * blank_tables / TreeBuilder: an ipp_mcts_tables as a dict of NumPy arrays and scalars in the state a search starts from, plus
    hand-built trees; the padding (k >= K) of t_nsa, t_qsa and t_ps is NaN, that of t_idx is -1;
  * SyntheticTables: an _ffi.IppMctsTables whose pointers are plain torch tensors uploaded from such a dict; select / backup / policy
    call the entry point and return every buffer as NumPy;
  * select_ref / backup_ref / policy_ref: plain per-root sequential Python in fp64, written from the reference's
    planning/mcts_zero/mcts.py (simulate :166-265, backup :253-265, normalize_q_values / compute_uct :267-296, read-out :83-143) in
    the operand order the kernels document.  They know nothing of lanes, ballots or LDS; next to their results they return
    instrumentation (which lane would hold the winner, whether several lanes tie, probes of a lookup, sharing of an edge, why a
    take-back loop ended, ...) from which the host test proves that a case reaches the edge it is named for;
  * the frozen, seeded case builders: SELECT_CASES, BACKUP_CASES, READOUT_CASES.

The module imports neither torch nor the package at import time.
"""
import ctypes as C
import math

import numpy as np

from tests.mcts_noise_ref import M64, mix64, u01

EXPANDED, STORED = 1, 2
PATH = 6                     # device nodes on a path (kMctsPath)
MARGIN = 1e-9                # the margin rule: winner and runner-up are an exact tie of identical operands or this far apart
ROOT_KEY = 0x9E3779B97F4A7C15
EDGE_TABLES = ("t_idx", "t_ps", "t_nsa", "t_qsa", "t_num", "t_child")
NODE_TABLES = ("n_k", "n_ns", "n_flags", "n_hash", "n_value", "n_devpath")
ARRAYS = ("actions", "zkey") + EDGE_TABLES + NODE_TABLES + (
    "root_count", "dev_count", "h_keys", "h_vals", "p_node", "p_k", "p_cost", "p_len", "leaf", "pend_node", "pend_depth", "pend_sim",
    "pend_prev", "pend_budget", "counts", "rq_root", "rq_parent", "rq_k", "rq_child", "rq_newdev", "rq_cost", "rq_prev", "rq_action",
    "ts_paths", "ts_reward", "ts_status", "err")
SCALARS = ("roots", "kmax", "nodes_per_root", "dev_per_root", "table_size", "max_depth", "wave", "horizon", "num_actions",
           "use_flight_time", "tie_break", "gamma", "puct_init", "puct_base", "fpf", "vmax", "amax", "root_base", "dev_base", "ns_table")


def bits(a):
    """An array's bits as unsigned integers (floats compared as stored: NaN payloads, -0.0)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def action_table(A):
    """actions [A][3]: distinct waypoints on a 4 m grid at two altitudes; costs between them are generic square roots."""
    a = np.arange(A)
    return np.stack([4.0 * (a % 17) + 2.0, 4.0 * ((a // 17) % 19) + 2.0, 8.0 + 6.0 * (a % 2)], axis=1)


def table_size_for(npr):
    t = 1
    while t < 2 * npr:
        t *= 2
    return t


def blank_tables(R, kmax, A, npr=8, D=3, wave=1, horizon=2, dev_per_root=4, tie_break=0, gamma=0.9, puct_init=1.25, puct_base=19652.0,
                 fpf=2.0, root_base=0, dev_base=0, ns_table="present", table_size=None, seed=1):
    """The tables of R roots as a search finds them at its start (include/ipp_engine.h), the per-wave buffers filled with recognisable
    values: what a call leaves alone is visible as such.  ns_table: "present" (the host's table reaches every Ns), "absent" (NULL) or
    an integer n (a table of n entries: too short for a node with Ns >= n)."""
    cap, tsz = R * npr, table_size or table_size_for(npr)
    st = dict(roots=R, kmax=kmax, nodes_per_root=npr, dev_per_root=dev_per_root, table_size=tsz, max_depth=D, wave=wave, horizon=horizon,
              num_actions=A, use_flight_time=0, tie_break=tie_break, gamma=gamma, puct_init=puct_init, puct_base=puct_base, fpf=fpf,
              vmax=1.0, amax=1.0, root_base=root_base, dev_base=dev_base, ns_table=ns_table)
    st["actions"] = action_table(A)
    st["zkey"] = np.random.RandomState(12345 + seed).randint(1, 2 ** 62, size=A, dtype=np.int64).astype(np.uint64)
    st["t_idx"] = np.full((cap, kmax), -1, np.int32)
    for k in ("t_ps", "t_nsa", "t_qsa", "t_num"):
        st[k] = np.full((cap, kmax), np.nan)
    st["t_child"] = np.full((cap, kmax), -1, np.int32)
    st["n_k"] = np.zeros(cap, np.int32)
    st["n_ns"] = np.zeros(cap)
    st["n_flags"] = np.zeros(cap, np.uint8)
    st["n_hash"] = np.zeros(cap, np.uint64)
    st["n_value"] = np.zeros(cap)
    st["n_devpath"] = np.full((cap, PATH), -1, np.int32)
    roots = np.arange(R) * npr
    st["n_flags"][roots] = STORED
    st["n_hash"][roots] = ((np.arange(R, dtype=np.uint64) + np.uint64(1 + root_base)) * np.uint64(ROOT_KEY))
    st["root_count"] = np.ones(R, np.int32)
    st["dev_count"] = np.zeros(R, np.int32)
    st["h_keys"] = np.zeros((R, tsz), np.uint64)
    st["h_vals"] = np.full((R, tsz), -5, np.int32)
    st["p_node"] = np.full((wave, R, D), -7, np.int32)
    st["p_k"] = np.full((wave, R, D), -7, np.int32)
    st["p_cost"] = np.full((wave, R, D), -7.0)
    st["p_len"] = np.full((wave, R), -7, np.int32)
    st["leaf"] = np.full((wave, R), -7, np.int32)
    st["pend_node"] = np.full((R, wave), -7, np.int32)
    st["pend_depth"] = np.full((R, wave), -7, np.int32)
    st["pend_sim"] = np.full((R, wave), -7, np.int32)
    st["pend_prev"] = np.full((R, wave, 3), -7.0)
    st["pend_budget"] = np.full((R, wave), -7.0)
    st["counts"] = np.zeros(R + 1, np.int32)     # pend_count [R] and rq_count [1] in one buffer, as DeviceMCTS keeps them
    n = D * R * wave
    for k in ("rq_root", "rq_parent", "rq_k", "rq_child", "rq_newdev", "ts_status"):
        st[k] = np.full(n, -7, np.int32)
    st["rq_cost"] = np.full(n, -7.0)
    st["rq_prev"], st["rq_action"] = np.full((n, 3), -7.0), np.full((n, 3), -7.0)
    st["ts_paths"] = np.full((n, PATH), -7, np.int32)
    st["ts_reward"] = np.full(n, -7.0, np.float32)
    st["err"] = np.zeros(4, np.int32)
    return st


def copy_tables(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def ns_table_len(st):
    """Entries of the host's Ns table (0: none)."""
    mode = st["ns_table"]
    if mode == "absent":
        return 0
    return int(max(8, np.nanmax(st["n_ns"]) + 4 * st["wave"] + 8)) if mode == "present" else int(mode)


def validate(st, W=None):
    """Everything a kernel indexes with stays inside its buffer: checked before anything is uploaded."""
    R, kmax, npr, A, D, wave = st["roots"], st["kmax"], st["nodes_per_root"], st["num_actions"], st["max_depth"], st["wave"]
    assert st["table_size"] >= 2 * npr and st["table_size"] & (st["table_size"] - 1) == 0 and D <= 8 and st["horizon"] + 1 <= PATH
    assert np.all(st["n_k"] >= 0) and np.all(st["n_k"] <= kmax)
    for nd in np.nonzero(st["n_flags"] & EXPANDED)[0]:
        K, j = int(st["n_k"][nd]), nd // npr
        if nd % npr:
            assert K >= 1, "an expanded node below the root has a valid action"
        assert np.all((st["t_idx"][nd, :K] >= 0) & (st["t_idx"][nd, :K] < A))
        ch = st["t_child"][nd, :K]
        assert np.all((ch == -1) | ((ch >= j * npr) & (ch < (j + 1) * npr)))
    assert np.all((st["root_count"] >= 1) & (st["root_count"] <= npr)) and np.all((st["dev_count"] >= 0) & (st["dev_count"] <= st["dev_per_root"]))
    assert np.all((st["h_keys"] != 0).sum(axis=1) < st["table_size"] - npr), "a probe chain always ends at an empty slot"
    if W is not None:  # recorded descents in front of a backup
        assert 1 <= W <= wave
        for w in range(W):
            for j in range(R):
                n = int(st["p_len"][w, j])
                assert 0 <= n <= D and -1 <= st["leaf"][w, j] < R * npr
                assert np.all((st["p_node"][w, j, :n] >= j * npr) & (st["p_node"][w, j, :n] < (j + 1) * npr))
                assert np.all((st["p_k"][w, j, :n] >= 0) & (st["p_k"][w, j, :n] < kmax))


class SyntheticTables:
    """ipp_mcts_tables over plain tensors: upload a dict of tables, call an entry point, read every buffer back."""

    def __init__(self, st):
        import torch

        from ipp_rl_amd import _ffi

        validate(st)
        self.torch, self.ffi, self.lib = torch, _ffi, _ffi.load()
        self.dev = torch.device("cuda:0")
        self.st = st
        self.t = {k: self.up(st[k]) for k in ARRAYS}
        R = st["roots"]
        # expansion geometry: not read by the three calls, but the ABI wants the pointers
        self.geo = {k: self.up(np.zeros(4, np.int32)) for k in ("cell_action", "off_x", "off_y")}
        self.geo["uniform_ps"] = self.up(np.zeros(st["kmax"] + 1))
        tab = _ffi.IppMctsTables(
            roots=R, kmax=st["kmax"], nodes_per_root=st["nodes_per_root"], dev_per_root=st["dev_per_root"], table_size=st["table_size"],
            max_depth=st["max_depth"], wave=st["wave"], horizon=st["horizon"], grid_w=1, grid_h=1, n_levels=1, n_off=1,
            num_actions=st["num_actions"], use_flight_time=st["use_flight_time"], tie_break=st["tie_break"], device=0, res=4.0, max_dist=11.5,
            gamma=st["gamma"], puct_init=st["puct_init"], puct_base=st["puct_base"], fpf=st["fpf"], vmax=st["vmax"], amax=st["amax"],
            root_base=st["root_base"], dev_base=st["dev_base"], scratch_base=0)
        for k in ARRAYS:
            if k != "counts":
                setattr(tab, k, self.t[k].data_ptr())
        for k, v in self.geo.items():
            setattr(tab, k, v.data_ptr())
        tab.pend_count = self.t["counts"].data_ptr()
        tab.rq_count = self.t["counts"].data_ptr() + 4 * R
        n = ns_table_len(st)
        if n:
            ns = np.arange(n, dtype=np.float64)
            self.ns_tables = (self.up(st["puct_init"] + np.log((ns + st["puct_base"] + 1) / st["puct_base"])), self.up(np.sqrt(ns + 1)))
            tab.puct_c, tab.sqrt_ns1, tab.ns_table_n = self.ns_tables[0].data_ptr(), self.ns_tables[1].data_ptr(), n
        self.tab = tab
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.as_tensor(a.view(np.int64) if a.dtype == np.uint64 else a, device=self.dev)

    def download(self):
        self.torch.cuda.synchronize()
        return {k: (v.cpu().numpy().view(np.uint64) if self.st[k].dtype == np.uint64 else v.cpu().numpy()) for k, v in self.t.items()}

    def select(self, root_env, prev0, budget0, depth0, sim0, W, seed):
        self._keep = [self.up(np.asarray(root_env, np.int32)), self.up(np.asarray(prev0, np.float64)), self.up(np.asarray(budget0, np.float64))]
        self.ffi.check(self.lib.ipp_mcts_select(C.byref(self.tab), *[x.data_ptr() for x in self._keep], int(depth0), int(sim0), int(W),
                                                C.c_uint64(seed & M64), self.stream))
        return self.download()

    def backup(self, wave):
        validate_descents(self.st, wave)
        self.ffi.check(self.lib.ipp_mcts_backup(C.byref(self.tab), int(wave), self.stream))
        return self.download()

    def policy(self, tie_u, temperature, deploy_time, want_idx=True):
        torch, R, kmax = self.torch, self.st["roots"], self.st["kmax"]
        pol = torch.full((R, kmax), 7.0, dtype=torch.float64, device=self.dev)
        idx = torch.full((R, kmax), -9, dtype=torch.int32, device=self.dev)
        ok = torch.full((R,), -9, dtype=torch.int32, device=self.dev)
        u = None if tie_u is None else self.up(np.asarray(tie_u, np.float64))
        self.ffi.check(self.lib.ipp_mcts_policy(C.byref(self.tab), None if u is None else u.data_ptr(), float(temperature), int(deploy_time),
                                                pol.data_ptr(), idx.data_ptr() if want_idx else None, ok.data_ptr(), self.stream))
        out = self.download()
        out.update(policy=pol.cpu().numpy(), valid_idx=idx.cpu().numpy(), ok=ok.cpu().numpy())
        return out


def validate_descents(st, W):
    c = st["counts"].copy()
    st["counts"][:] = 0
    try:
        validate(st, W)
    finally:
        st["counts"][:] = c


# ---------------------------------------------------------------------------------------------------- restatements
def normalize_q(q, K, A):
    """normalize_q_values (mcts.py:267-278) of a node's Q on its K valid actions; the reference normalises the A-long array, whose
    entries outside the valid set are 0.  Returns (normalised q, branch): branch names what ran and what the zeros outside did."""
    q = np.asarray(q, np.float64)
    values = q if K == A else np.concatenate([q, [0.0]])
    if np.all(values == 0):
        return q.copy(), "allzero"
    lo, hi = np.min(values), np.max(values)
    sign = "positive" if np.min(q) > 0 else "negative" if np.max(q) < 0 else "mixed"
    if lo == hi:
        return q / hi, "flat"
    return (q - lo) / (hi - lo), ("range-" + sign + ("-widened" if K < A and sign != "mixed" else ""))


def puct_c(st, ns):
    return st["puct_init"] + np.log((ns + st["puct_base"] + 1) / st["puct_base"])


def uct_scores(st, node, force):
    """compute_uct (mcts.py:280-296) on the node's valid actions: (uct [K], branch, forced mask)."""
    K, A = int(st["n_k"][node]), st["num_actions"]
    q, nsa, ps, ns = st["t_qsa"][node, :K], st["t_nsa"][node, :K], st["t_ps"][node, :K], float(st["n_ns"][node])
    qn, branch = normalize_q(q, K, A)
    prior = puct_c(st, ns) * (ps * (np.sqrt(ns + 1) / (1 + nsa)))
    uct = qn + prior
    forced = np.zeros(K, bool)
    if force:
        nfp = np.ceil(np.sqrt(st["fpf"] * ps * ns))
        nfp[nsa == 0] = 0
        forced = nsa < nfp
        uct[forced] = np.inf
    return uct, branch, forced


def tie_draw(st, seed, node, k, sim):
    """The counter-based draw of edge k of `node` in simulation `sim` (tie_break = 1)."""
    gnode = (node + st["root_base"] * st["nodes_per_root"]) & 0xFFFFFFFF
    return u01(mix64((seed & M64) ^ mix64((gnode << 32) | ((k + 1) & 0xFFFFFFFF)) ^ ((sim << 20) & M64)))


def choose(st, uct, node, sim, seed, operands):
    """The action of mcts.py:236 under the deterministic tie rules: the largest score; among equal scores the largest draw
    (tie_break = 1), then the lowest k.  Returns (k, info): the lane (k mod 64) and register slot (k div 64) a wave would hold the
    winner in, whether several lanes hold a maximum (`lane_tie`), whether the lowest tied k sits on the lowest tied lane, and the gap
    to the runner-up score."""
    top = np.nonzero(uct == np.max(uct))[0]
    if st["tie_break"]:
        draws = np.array([tie_draw(st, seed, node, int(k), sim) for k in top])
        k = int(top[np.nonzero(draws == draws.max())[0][0]])
        lane_best = {}
        for kk, u in zip(top, draws):  # what each lane keeps: its largest draw
            if kk % 64 not in lane_best or u > lane_best[kk % 64][0]:
                lane_best[kk % 64] = (u, int(kk))
    else:
        k = int(top[0])
        lane_best = {}
        for kk in top:
            lane_best.setdefault(int(kk) % 64, (0.0, int(kk)))
    rest = uct[uct != np.max(uct)]
    gap = float(np.max(uct) - np.max(rest)) if len(rest) else math.inf
    if np.isnan(gap):
        gap = math.inf  # (inf - inf cannot happen: rest excludes the maximum; inf - finite = inf)
    ident = all(np.isinf(uct[t]) or all(same_bits(op[t], op[k]) for op in operands) for t in top)
    lowest_lane = min(lane_best)
    return k, dict(lane=k % 64, slot=k // 64, lane_tie=len(lane_best) > 1, n_top=len(top), lowest_k_on_lowest_lane=lane_best[lowest_lane][1] == k,
                   gap=gap, identical_ties=bool(ident))


def distance(a, p):
    d = a - p
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def edge_cost(st, a, p):
    """actions.py:8-41: the distance, or the trapezoidal flight time."""
    dist = distance(a, p)
    if not st["use_flight_time"]:
        return dist
    ramp = min(0.5 * dist, (st["vmax"] * st["vmax"]) / (2 * st["amax"]))
    return (dist - 2 * ramp) / st["vmax"] + 2 * math.sqrt(2 * ramp / st["amax"])


def probe(st, j, key, insert=None):
    """Look `key` up in root j's open-addressing table (linear probing from mix64(key) mod table_size); insert -> value when absent.
    Returns (value or None, probes, wrapped)."""
    tsz = st["table_size"]
    slot, probes, wrapped = mix64(key) & (tsz - 1), 1, False
    while True:
        kk = int(st["h_keys"][j, slot])
        if kk == key:
            return int(st["h_vals"][j, slot]), probes, wrapped
        if kk == 0:
            if insert is not None:
                st["h_keys"][j, slot], st["h_vals"][j, slot] = key, insert
            return None, probes, wrapped
        slot, probes = slot + 1, probes + 1
        if slot == tsz:
            slot, wrapped = 0, True


def select_ref(st0, root_env, prev0, budget0, depth0, sim0, W, seed):
    """ipp_mcts_select: W descents per root, one root after the other (mcts.py:166-265 without the recursion's way back).  Returns
    (tables after the call, requests, info): requests = the list of requested covariance steps as tuples (root env, parent, k, child,
    newdev, cost, prev, action, path) in root order; info[(j, w)] = list of per-level dicts."""
    st = copy_tables(st0)
    R, npr, D, H, wave = st["roots"], st["nodes_per_root"], st["max_depth"], st["horizon"], st["wave"]
    virtual = W > 1
    requests, info = [], {}
    for j in range(R):
        base = j * npr
        for w in range(W):
            node, prev, budget, leaf, plen, levels = base, np.array(prev0[j], np.float64), float(budget0[j]), -1, 0, []
            for d in range(depth0, H + 1):
                if not budget > 0:  # mcts.py:175-176
                    levels.append(dict(end="budget"))
                    break
                if not st["n_flags"][node] & EXPANDED:  # a leaf: evaluated once per wave of simulations
                    leaf = node
                    cnt = int(st["counts"][j])
                    seen = node in st["pend_node"][j, :cnt]
                    if not seen:
                        st["pend_node"][j, cnt], st["pend_depth"][j, cnt], st["pend_sim"][j, cnt] = node, d, sim0 + w
                        st["pend_prev"][j, cnt], st["pend_budget"][j, cnt] = prev, budget
                        st["counts"][j] = cnt + 1
                    levels.append(dict(end="leaf", pending_seen=bool(seen)))
                    break
                uct, branch, forced = uct_scores(st, node, force=(d == 0))
                K = int(st["n_k"][node])
                k, lv = choose(st, uct, node, sim0 + w, seed, (st["t_qsa"][node, :K], st["t_nsa"][node, :K], st["t_ps"][node, :K]))
                ns = float(st["n_ns"][node])
                n_tab = ns_table_len(st)
                lv.update(node=node, k=k, d=d, branch=branch, forced=int(forced.sum()), winner_forced=bool(forced[k]),
                          ns_from_table=bool(n_tab and ns == int(ns) and 0 <= ns < n_tab))
                a = int(st["t_idx"][node, k])
                action = st["actions"][a]
                cost = edge_cost(st, action, prev)
                child = int(st["t_child"][node, k])
                if child < 0:  # the same measurements in any order are one node
                    key = (int(st["n_hash"][node]) + int(st["zkey"][a])) & M64
                    lv["key_zero"] = key == 0
                    key = key or 1
                    child, probes, wrapped = probe(st, j, key)
                    lv.update(probes=probes, wrapped=wrapped, found=child is not None)
                    if child is None:
                        cnt = int(st["root_count"][j])
                        if cnt >= npr:
                            st["err"][0], child = 1, base
                            lv["nodes_exhausted"] = True
                        else:
                            child = base + cnt
                            st["root_count"][j] = cnt + 1
                            probe(st, j, key, insert=child)
                            st["n_hash"][child] = key
                    st["t_child"][node, k] = child
                if np.isnan(st["t_num"][node, k]):  # first traversal of the edge: one covariance step
                    st["t_num"][node, k] = np.inf
                    newdev, why = -1, "stored" if st["n_flags"][child] & STORED else "horizon" if d + 1 > H else ""
                    if not why:
                        dc = int(st["dev_count"][j])
                        if dc >= st["dev_per_root"]:
                            st["err"][1], why = 1, "exhausted"
                        else:
                            newdev, why = st["dev_base"] + j * st["dev_per_root"] + dc, "new"
                            st["dev_count"][j] = dc + 1
                            st["n_flags"][child] |= STORED
                    path = st["n_devpath"][node].copy()
                    requests.append((int(root_env[j]), node, k, child, newdev, cost, prev.copy(), action.copy(), path))
                    if newdev >= 0:
                        cp = path.copy()
                        cp[int((path >= 0).sum())] = newdev
                        st["n_devpath"][child] = cp
                    lv["request"] = why
                st["p_node"][w, j, plen], st["p_k"][w, j, plen], st["p_cost"][w, j, plen] = node, k, cost
                if virtual:
                    st["t_nsa"][node, k] += 1
                    st["n_ns"][node] += 1
                plen += 1
                budget -= cost
                prev = action.copy()
                node = child
                levels.append(lv)
            else:
                levels.append(dict(end="horizon"))
            st["p_len"][w, j], st["leaf"][w, j] = plen, leaf
            info[(j, w)] = levels
    n = len(requests)
    st["counts"][R] = n
    return st, requests, info


def requests_of(out):
    """The request list of downloaded tables as a set of tuples keyed by (parent, k): its order across roots is the atomic counter's."""
    n = int(out["counts"][-1])
    return {(int(out["rq_parent"][r]), int(out["rq_k"][r])): (int(out["rq_root"][r]), int(out["rq_child"][r]), int(out["rq_newdev"][r]),
            bits(out["rq_cost"][r:r + 1]).item(), bits(out["rq_prev"][r]).tobytes(), bits(out["rq_action"][r]).tobytes(),
            out["ts_paths"][r].tobytes()) for r in range(n)}


def requests_ref(requests):
    return {(p, k): (root, child, newdev, bits(np.array([cost])).item(), bits(prev).tobytes(), bits(action).tobytes(),
            np.asarray(path, np.int32).tobytes()) for root, p, k, child, newdev, cost, prev, action, path in requests}


def backup_ref(st0, W):
    """ipp_mcts_backup: the W recorded descents of every root in turn, the deepest step first (mcts.py:253-265, the virtual visit of
    each traversal taken back first).  Returns (tables, info): info[j] = {edge: [(descent, step index, count found)]}."""
    st = copy_tables(st0)
    virtual = W > 1
    info = {}
    for j in range(st["roots"]):
        edges = {}
        for w in range(W):
            lf = int(st["leaf"][w, j])
            value = float(st["n_value"][lf]) if lf >= 0 else 0.0
            for stp in range(int(st["p_len"][w, j]) - 1, -1, -1):
                node, k, cost = int(st["p_node"][w, j, stp]), int(st["p_k"][w, j, stp]), float(st["p_cost"][w, j, stp])
                if virtual:
                    st["t_nsa"][node, k] -= 1
                    st["n_ns"][node] -= 1
                reward = st["t_num"][node, k] / (cost + 1.0)  # rewards.py:31
                value = reward + st["gamma"] * value
                nsa = st["t_nsa"][node, k]
                edges.setdefault((node, k), []).append((w, stp, float(nsa)))
                if nsa > 0:
                    st["t_qsa"][node, k] = (nsa * st["t_qsa"][node, k] + value) / (nsa + 1)
                    st["t_nsa"][node, k] = nsa + 1
                else:
                    st["t_qsa"][node, k] = value
                    st["t_nsa"][node, k] = nsa + 1
                st["n_ns"][node] += 1
        info[j] = edges
    st["counts"][:] = 0
    return st, info


def pick_tie(ties, u):
    """np.random.choice among the ties as a function of one uniform (None: the first)."""
    return int(ties[min(int(u * len(ties)), len(ties) - 1)]) if u is not None else int(ties[0])


def policy_ref(st, tie_u, temperature, deploy_time):
    """ipp_mcts_policy: get_policy's read-out (mcts.py:96-143, temperature > 0) of every root.  Returns (policy [R][kmax], valid_idx,
    ok, info): info[j] = dict(branch, n_ties, pick, chunk, rank_in_chunk, best, taken = {k: (playouts taken back, why the loop
    ended)}, dropped_single = [k], min_margin)."""
    R, kmax, npr, A = st["roots"], st["kmax"], st["nodes_per_root"], st["num_actions"]
    policy, ok, info = np.zeros((R, kmax)), np.zeros(R, np.int32), {}
    for j in range(R):
        root = j * npr
        K = int(st["n_k"][root])
        info[j] = dict(bad="unexpanded" if not st["n_flags"][root] & EXPANDED else "K=0" if K == 0 else "")
        if info[j]["bad"]:
            continue
        visits = st["t_nsa"][root, :K].copy()
        nsa, q, ps, ns = st["t_nsa"][root, :K], st["t_qsa"][root, :K], st["t_ps"][root, :K], float(st["n_ns"][root])
        if not deploy_time:
            ties = np.nonzero(visits == np.max(visits))[0]
            u = None if tie_u is None else float(tie_u[j])
            # (the reference's arg-max runs over all A actions: with every valid action unvisited and K < A it may land outside the
            # valid set, where the score is -inf -- nothing is kept and nothing can be taken back)
            best = pick_tie(ties, u) if np.max(visits) > 0 or K == A else -1
            rank = int(np.nonzero(ties == best)[0][0]) if best >= 0 else -1
            nfp = np.ceil(np.sqrt(st["fpf"] * ps * ns))
            nfp[nsa == 0] = 0
            uct, branch, _ = uct_scores(st, root, force=False)
            max_puct = uct[best] if best >= 0 else -np.inf
            qn, _ = normalize_q(q, K, A)
            taken, margin = {}, math.inf
            for k in range(K):
                if k == best or nfp[k] <= 0:
                    continue
                n, why = 0, "count"
                for _ in range(int(nfp[k])):
                    visits[k] -= 1
                    with np.errstate(divide="ignore"):
                        prior = puct_c(st, ns) * (ps[k] * (np.sqrt(ns + 1) / (1 + visits[k])))
                    pruned = qn[k] + prior
                    if pruned >= max_puct:
                        visits[k] += 1
                        why = "inf" if np.isinf(prior) else "equal" if pruned == max_puct else "above"
                        break
                    n += 1
                    if np.isfinite(pruned) and np.isfinite(max_puct):
                        margin = min(margin, abs(pruned - max_puct))
                if why == "above" and np.isfinite(max_puct):
                    margin = min(margin, abs(pruned - max_puct))
                taken[k] = (n, why)
            single = [int(k) for k in np.nonzero(visits == 1)[0]]
            visits[visits == 1] = 0
            info[j].update(branch=branch, n_ties=len(ties), best=best, pick=rank, chunk=best // 64 if best >= 0 else -1,
                           rank_in_chunk=int((ties[ties < best] >= 64 * (best // 64)).sum()) if best >= 0 else -1,
                           last_in_chunk=bool(best >= 0 and not np.any((ties > best) & (ties < 64 * (best // 64 + 1)))),
                           taken=taken, dropped_single=single, started_single=[int(k) for k in np.nonzero(nsa == 1)[0]], min_margin=margin,
                           vmax=float(np.max(nsa)))
        if np.sum(visits) == 0:
            info[j]["bad"] = "no visits"
            continue
        vt = np.array([v ** (1.0 / temperature) for v in visits])
        policy[j, :K] = vt / np.sum(vt)
        ok[j] = 1
    return policy, st["t_idx"][np.arange(R) * npr].copy(), ok, info


# ---------------------------------------------------------------------------------------------------- building trees
class TreeBuilder:
    """Hand-built trees in blank tables.  Nodes are numbered per root (0 = the root node); expand() gives a node its row, child()
    hangs a node below an edge the way a finished simulation leaves it (the child in the hash table, the edge's numerator known)."""

    def __init__(self, st, seed=0):
        self.st, self.rs = st, np.random.RandomState(seed)

    def node(self, j, local):
        return j * self.st["nodes_per_root"] + local

    def expand(self, j, local, idx, ps=None, nsa=None, qsa=None, ns=None, value=0.0):
        st, nd = self.st, self.node(j, local)
        K = len(idx)
        assert K <= st["kmax"] and list(idx) == sorted(set(idx))
        st["t_idx"][nd, :K] = idx
        st["t_ps"][nd, :K] = np.full(K, 1.0 / K) if ps is None else ps
        st["t_nsa"][nd, :K] = 0.0 if nsa is None else nsa
        st["t_qsa"][nd, :K] = 0.0 if qsa is None else qsa
        st["t_num"][nd, :K] = np.nan
        st["t_num"][nd, :K][st["t_nsa"][nd, :K] > 0] = 1.0  # (a visited edge has its numerator; cases set their own where it matters)
        st["t_child"][nd, :K] = -1
        st["n_k"][nd] = K
        st["n_ns"][nd] = float(np.sum(st["t_nsa"][nd, :K])) if ns is None else ns
        st["n_flags"][nd] |= EXPANDED
        st["n_value"][nd] = value
        return nd

    def child(self, j, parent_local, k, stored=True, link=True, num=None):
        """A node below edge k of the parent: allocated, keyed, in the hash table; link=False leaves the edge's t_child at -1 (the
        child is found through the table: a transposition)."""
        st, p = self.st, self.node(j, parent_local)
        a = int(st["t_idx"][p, k])
        key = ((int(st["n_hash"][p]) + int(st["zkey"][a])) & M64) or 1
        got, _, _ = probe(st, j, key)
        if got is None:
            cnt = int(st["root_count"][j])
            got = j * st["nodes_per_root"] + cnt
            st["root_count"][j] = cnt + 1
            probe(st, j, key, insert=got)
            st["n_hash"][got] = key
            if stored:
                st["n_flags"][got] |= STORED
        if link:
            st["t_child"][p, k] = got
            st["t_num"][p, k] = self.rs.uniform(0.2, 2.0) if num is None else num
        return got - j * st["nodes_per_root"]


def random_row(rs, K, q_kind, ns=None, visited=0.7, least=1):
    """(ps, nsa, qsa, ns) of a node: priors that sum to 1, integer visit counts (0, or `least` to 5), Q of the given kind."""
    ps = rs.uniform(0.2, 1.0, K)
    ps /= ps.sum()
    nsa = np.where(rs.uniform(size=K) < visited, rs.randint(least, 6, K), 0).astype(np.float64)
    q = {"zero": np.zeros(K), "flat": np.full(K, 0.375), "positive": rs.uniform(0.1, 1.0, K), "negative": -rs.uniform(0.1, 1.0, K),
         "mixed": rs.uniform(-1.0, 1.0, K)}[q_kind]
    if q_kind in ("positive", "negative", "mixed"):
        q = np.where(nsa > 0, q, 0.0) if q_kind == "mixed" else q
    return ps, nsa, q, float(nsa.sum()) if ns is None else ns


Q_KINDS = ("flat", "zero", "positive", "negative", "mixed")   # root 0 has K == A: flat non-zero; the others K < A


# ---------------------------------------------------------------------------------------------------- select cases
SELECT_CASES = {}


def _sel(name):
    def deco(f):
        SELECT_CASES[name] = f
        return f
    return deco


def _random_select(kmax, W, ns_table="present", tie_break=0, seed=0, depth0=0, plant=True):
    """5 roots (four per block: the last block is partial), two expanded levels below each root; root 0 has K == kmax == A and a flat
    non-zero Q, roots 1-4 have K < A and Q all zero / positive / negative / mixed.  With `plant` a winner is planted in the highest
    register slot the row has on roots 2 and 3."""
    R, A, npr = 5, kmax, 40
    st = blank_tables(R, kmax, A, npr=npr, D=3, wave=max(W, 1), horizon=2, dev_per_root=32, ns_table=ns_table, tie_break=tie_break,
                      root_base=0, seed=seed)
    tb = TreeBuilder(st, seed)
    rs = np.random.RandomState(100 + seed + kmax)
    for j in range(R):
        K = kmax if j == 0 else kmax - 1 if j == 2 else int(rs.randint(max(2, kmax - 40), kmax))
        if j == 4:
            K = min(kmax - 1, 65) if kmax > 65 else kmax - 1
        idx = np.sort(rs.choice(A, K, replace=False))
        # roots 2 and 3 owe no forced playouts (no edge with 1 or 2 visits: ceil(sqrt(2 ps Ns)) is 3 or less there), so a finite
        # score wins at the root; the others start with ties of forced playouts
        ps, nsa, q, ns = random_row(rs, K, Q_KINDS[j], least=4 if j in (2, 3) else 1, visited=1.0 if j in (2, 3) else 0.7)
        if plant and j in (2, 3):
            k_star = K - 1 if j == 2 else min(67, K - 2)  # (root 2: in the row's last register slot; root 3: in the second)
            ps[k_star] = 3.0 * ps.max()
            ps /= ps.sum()
            nsa[k_star], q[k_star] = np.ceil(np.sqrt(st["fpf"] * ps[k_star] * ns)), q.max() + 0.5 * abs(q.max())
            assert np.all((nsa == 0) | (nsa >= np.ceil(np.sqrt(st["fpf"] * ps * ns))))
        tb.expand(j, 0, idx, ps, nsa, q, ns)
        # children of the most promising edges: expanded nodes with their own rows (second level), some with a third level below
        uct, _, _ = uct_scores(st, tb.node(j, 0), force=(depth0 == 0))
        for rank, k in enumerate(np.argsort(-uct, kind="stable")[:3]):
            if rank == 2:
                continue  # (the third stays without a child: a new node when a descent reaches it)
            c = tb.child(j, 0, int(k))
            Kc = int(rs.randint(2, min(kmax, 70)))
            cidx = np.sort(rs.choice(A, Kc, replace=False))
            cps, cnsa, cq, cns = random_row(rs, Kc, Q_KINDS[(j + rank + 1) % 5] if Kc < A else "flat")
            tb.expand(j, c, cidx, cps, cnsa, cq, cns)
            if rank == 0:
                cu, _, _ = uct_scores(st, tb.node(j, c), force=False)
                g = tb.child(j, c, int(np.argmax(cu)))
                tb.expand(j, g, np.sort(rs.choice(A, 3, replace=False)), None, np.array([1.0, 0.0, 2.0]), np.array([0.3, 0.0, -0.2]))
    prev0 = st["actions"][rs.randint(0, A, R)] + np.array([1.0, 0.5, 0.25])
    budget0 = np.full(R, 500.0)
    return dict(st=st, root_env=np.arange(R) * 3 + 1, prev0=prev0, budget0=budget0, depth0=depth0, sim0=0, W=W, seed=11 + seed)


for _kmax in (64, 65, 130, 256, 257):
    SELECT_CASES[f"kmax-{_kmax}"] = (lambda kmax=_kmax: _random_select(kmax, 4, seed=kmax))
SELECT_CASES["w1"] = lambda: _random_select(64, 1, seed=7)
SELECT_CASES["w8"] = lambda: _random_select(64, 8, seed=8)
SELECT_CASES["table-absent"] = lambda: _random_select(65, 4, ns_table="absent", seed=9)
SELECT_CASES["table-short"] = lambda: _random_select(65, 4, ns_table=6, seed=9)
SELECT_CASES["random-ties-257"] = lambda: _random_select(257, 4, tie_break=1, seed=10)


def _forced_rows(depth0):
    """Exact ties from forced playouts (uct = inf on several edges) in chosen positions; kmax 130 (three register slots).  The same
    rows with depth0 = 1 (forced playouts off): the winner is the planted finite maximum."""
    R, kmax, A = 4, 130, 140
    st = blank_tables(R, kmax, A, npr=8, D=3, wave=4, horizon=2, dev_per_root=4, seed=3)
    tb = TreeBuilder(st, 3)
    rs = np.random.RandomState(33)
    forced_at = ((70, 10), (129, 64, 3), (5, 69, 100), (70, 75, 129))  # root 2: two ties on ONE lane (5) and one on lane 36
    for j in range(R):
        K = 130
        ps = rs.uniform(0.5, 1.0, K)
        ps /= ps.sum()
        nsa = rs.randint(3, 7, K).astype(np.float64)
        ns = 400.0
        for k in forced_at[j]:  # visited once, owed ceil(sqrt(2 ps Ns)) >= 2 playouts
            nsa[k] = 1.0
        q = rs.uniform(0.1, 0.9, K)
        tb.expand(j, 0, np.arange(K) + j, ps, nsa, q, ns)
        assert np.all(np.ceil(np.sqrt(st["fpf"] * ps * ns)) == 3)
    prev0 = st["actions"][[5, 6, 7, 8]] + 0.5
    return dict(st=st, root_env=np.array([4, 2, 0, 9]), prev0=prev0, budget0=np.full(R, 300.0), depth0=depth0, sim0=8, W=4, seed=5)


SELECT_CASES["forced-ties"] = lambda: _forced_rows(0)
SELECT_CASES["forced-off"] = lambda: _forced_rows(1)


def _tie_break_random(kmax):
    """tie_break = 1 with root_base != 0 and sim0 != 0: exact ties of identical operands (fresh rows: Q 0, no visits, equal priors) and of
    forced playouts; the winner is the largest draw.  kmax 130, 256 and 300: the register forms NE = 3 and 4 and the general form, each
    with several tied edges on one lane."""
    R, A = 3, kmax + 70
    st = blank_tables(R, kmax, A, npr=12, D=3, wave=4, horizon=2, dev_per_root=8, tie_break=1, root_base=37, seed=4)
    tb = TreeBuilder(st, 4)
    rs = np.random.RandomState(44)
    tb.expand(0, 0, np.arange(kmax), None, None, None, 0.0)                      # all edges tie
    ps = np.full(100, 0.004)
    ps[70:90] = 0.03                                                             # 20 equal maxima in the second slot
    tb.expand(1, 0, np.arange(100) * 2, ps, None, None, 0.0)
    ps, nsa = rs.uniform(0.5, 1.0, kmax), rs.randint(3, 7, kmax).astype(np.float64)
    ps /= ps.sum()
    nsa[[3, 66, 67, kmax - 1]] = 1.0                                             # forced: inf on four edges
    ns = 400.0 * kmax / 130
    assert np.all(np.ceil(np.sqrt(st["fpf"] * ps * ns)) == 3)
    tb.expand(2, 0, np.arange(kmax) + 9, ps, nsa, rs.uniform(0.1, 0.9, kmax), ns)
    return dict(st=st, root_env=np.array([0, 1, 2]), prev0=st["actions"][[1, 2, 3]] + 0.5, budget0=np.full(R, 300.0), depth0=0, sim0=5, W=4,
                seed=0xABCDEF0123456789)


SELECT_CASES["tie-break-random"] = lambda: _tie_break_random(130)
SELECT_CASES["tie-break-random-256"] = lambda: _tie_break_random(256)
SELECT_CASES["tie-break-random-300"] = lambda: _tie_break_random(300)


@_sel("budget-horizon")
def _budget_horizon():
    """Root 0: budget 0 at the root.  Root 1: the budget runs out after the first edge.  Root 2: every node down to the horizon is
    expanded (path of max_depth edges, leaf = -1).  Root 3: unexpanded root (both descents end there: one pending entry).  Root 4: both
    descents reach the same leaf below the root (K = 1)."""
    R, kmax, A = 5, 5, 9
    st = blank_tables(R, kmax, A, npr=8, D=3, wave=2, horizon=2, dev_per_root=4, seed=5)
    tb = TreeBuilder(st, 5)
    for j in (0, 1):
        tb.expand(j, 0, [1, 3, 4], [0.5, 0.3, 0.2], [2.0, 1.0, 0.0], [0.4, 0.1, 0.0])
        c = tb.child(j, 0, 0)
        tb.expand(j, c, [0, 2], [0.6, 0.4], [1.0, 0.0], [0.2, 0.0])
    tb.expand(2, 0, [0, 2, 5, 7, 8], None, [3.0, 1.0, 0.0, 0.0, 0.0], [0.5, -0.1, 0.0, 0.0, 0.0])
    c = tb.child(2, 0, 0)
    tb.expand(2, c, [1, 3], [0.7, 0.3], [2.0, 0.0], [0.3, 0.0])
    g = tb.child(2, c, 0)
    tb.expand(2, g, [4, 6, 7], None, [1.0, 0.0, 0.0], [0.25, 0.0, 0.0])
    tb.expand(4, 0, [6], [1.0], [2.0], [0.4])
    tb.child(4, 0, 0)
    prev0 = st["actions"][[0, 1, 2, 3, 4]] + np.array([0.0, 0.0, 1.0])
    first = min(distance(st["actions"][a], prev0[1]) for a in (1, 3, 4))  # whichever edge root 1 takes costs more than it has
    budget0 = np.array([0.0, 0.5 * first, 400.0, 50.0, 50.0])
    return dict(st=st, root_env=np.arange(R), prev0=prev0, budget0=budget0, depth0=0, sim0=2, W=2, seed=1)


@_sel("first-traversal")
def _first_traversal():
    """Edges with t_num = NaN.  Root 0: a new child gets a device node, its n_devpath written at depth 0.  Root 1: the same one level
    down (depth 1, below a stored child with a path of its own).  Root 2: the child is already stored (found through the table).  Root 3:
    the edge at the horizon (d + 1 > horizon).  Root 4: the device range is used up (err[1])."""
    R, kmax, A = 5, 4, 12
    st = blank_tables(R, kmax, A, npr=8, D=3, wave=1, horizon=2, dev_per_root=2, dev_base=40, seed=6)
    tb = TreeBuilder(st, 6)
    tb.expand(0, 0, [2, 5, 9])
    tb.expand(1, 0, [1, 4], [0.8, 0.2], [2.0, 0.0], [0.3, 0.0])
    c = tb.child(1, 0, 0)
    tb.expand(1, c, [3, 7, 8])
    st["n_devpath"][tb.node(1, c), 0] = 40 + 1 * 2 + 0
    st["dev_count"][1] = 1
    tb.expand(2, 0, [2, 6])
    tb.child(2, 0, 0, stored=True, link=False)
    tb.expand(3, 0, [0, 10], [0.9, 0.1], [1.0, 0.0], [0.2, 0.0])
    c = tb.child(3, 0, 0)
    tb.expand(3, c, [5, 11], [0.9, 0.1], [1.0, 0.0], [0.2, 0.0])
    g = tb.child(3, c, 0)
    tb.expand(3, g, [2, 3])
    tb.expand(4, 0, [3, 4, 8])
    st["dev_count"][4] = 2
    return dict(st=st, root_env=np.array([7, 6, 5, 4, 3]), prev0=st["actions"][[0, 0, 1, 1, 2]] + 0.25, budget0=np.full(R, 90.0), depth0=0,
                sim0=0, W=1, seed=2)


def find_root_key(st, j, a, want_slot, zero=False):
    """A key for root j's node (brute force on the CPU) whose child through action a hashes to `want_slot`; zero: the child's key is 0."""
    z = int(st["zkey"][a])
    if zero:
        return (-z) & M64
    h = 0x1234567 * (j + 1)
    while mix64(((h + z) & M64) or 1) & (st["table_size"] - 1) != want_slot:
        h += 1
    return h


@_sel("transposition")
def _transposition():
    """Root 0: a new node.  Root 1: an existing node reached from a second parent (a then b before, now b then a).  Root 2: hcur + zkey
    == 0 (the key becomes 1).  Root 3: the probe chain starts at the table's last slot, which is taken, as are slots 0 and 1: the lookup
    wraps and inserts at slot 2 (a stride of 2 would end at slot 3).  Root 4: the node range is used up (err[0], the child is the root node)."""
    R, kmax, A = 5, 3, 10
    st = blank_tables(R, kmax, A, npr=4, D=3, wave=1, horizon=2, dev_per_root=4, seed=7)
    tb = TreeBuilder(st, 7)
    tsz = st["table_size"]
    tb.expand(0, 0, [1, 5])
    # root 1: root -a(k=0)-> n1 (expanded, edge b leads to n2 = {a, b}); root -b(k=1)-> n3 (expanded, edge a unlinked): a descent that
    # takes b first finds n2 through the table
    tb.expand(1, 0, [2, 7], [0.3, 0.7], [4.0, 1.0], [0.1, 0.9])
    n1 = tb.child(1, 0, 0)
    tb.expand(1, n1, [7, 8], [0.6, 0.4], [1.0, 0.0], [0.2, 0.0])
    tb.child(1, n1, 0)
    n3 = tb.child(1, 0, 1)
    tb.expand(1, n3, [2, 9], [0.9, 0.1])
    st["n_hash"][tb.node(2, 0)] = find_root_key(st, 2, 4, 0, zero=True)
    tb.expand(2, 0, [4])
    st["n_hash"][tb.node(3, 0)] = find_root_key(st, 3, 6, tsz - 1)
    tb.expand(3, 0, [6])
    st["h_keys"][3, tsz - 1], st["h_vals"][3, tsz - 1] = 0xDEADBEEF, tb.node(3, 0)
    st["h_keys"][3, 0], st["h_vals"][3, 0] = 0xFEEDFACE, tb.node(3, 0)
    st["h_keys"][3, 1], st["h_vals"][3, 1] = 0xC0FFEE, tb.node(3, 0)
    tb.expand(4, 0, [0, 3])
    st["root_count"][4] = 4
    return dict(st=st, root_env=np.arange(R), prev0=st["actions"][[9, 8, 7, 6, 5]] + 0.25, budget0=np.full(R, 90.0), depth0=0, sim0=0, W=1,
                seed=3)


def check_margin(case, info):
    """The margin rule: every level's winner beats the runner-up by MARGIN unless the two are an exact tie of identical operands."""
    for (j, w), levels in info.items():
        for lv in levels:
            if "k" in lv:
                assert lv["gap"] >= MARGIN and lv["identical_ties"], (case, j, w, lv)


def build_select(name):
    c = SELECT_CASES[name]()
    validate(c["st"])
    st = c["st"]
    assert np.all(st["counts"] == 0) and np.all(st["n_k"][(st["n_flags"] & EXPANDED) != 0] >= 1) and c["W"] <= st["wave"]
    assert st["horizon"] + 1 - c["depth0"] <= st["max_depth"]
    want, requests, info = select_ref(c["st"], c["root_env"], c["prev0"], c["budget0"], c["depth0"], c["sim0"], c["W"], c["seed"])
    check_margin(name, info)
    return c, want, requests, info


# ---------------------------------------------------------------------------------------------------- backup cases
# name -> (W, max_depth, tables.wave of the wave form, tables.wave of the serial form, gamma)
BACKUP_CASES = {
    "w1-d3": (1, 3, 1, 22, 1.0),
    "w8-d8": (8, 8, 8, 9, 0.9),         # lane 63 in use
    "w4-d5-wave12": (4, 5, 12, 13, 0.9),  # 64 % D != 0; the lanes of w >= 4 idle
    "w4-d5-gamma1": (4, 5, 12, 13, 1.0),
    "w3-d7": (3, 7, 9, 10, 0.9),        # 63 lanes; W D = 21
    "w3-d6-wave5": (3, 6, 5, 11, 0.9),  # wave = 3 < tables.wave = 5
}
BACKUP_KMAX, BACKUP_K = 5, 3


def backup_descents(W, D, j, rs):
    """The W descents of root j as tuples of edge slots from the root down, and how each ends ("leaf": at an unexpanded node with a
    value; "none": leaf = -1).  The roots differ in structure: 0 = all descents along one chain with different lengths (every edge of
    the chain shared by a different number of descents, at different positions from their ends); 1 = a shared prefix, then they part;
    2 = lengths 0 beside one full-length descent; 3 = random walks over two slots per level; 4 = three descents over one two-edge
    prefix with different lengths, the rest on their own."""
    chain = tuple(int(x) for x in rs.randint(0, BACKUP_K, D))
    if j == 0:
        paths = [chain[:max(1, D - ((W - 1 - w) % D))] for w in range(W)]  # (the last descent has the full length: its deepest lane is W D - 1)
    elif j == 1:
        paths = [chain[:1] + tuple([(w + 1) % BACKUP_K] * min(D - 1, 1 + w % 3)) for w in range(W)]
    elif j == 2:
        paths = [() for _ in range(W)]
        paths[W // 2] = chain
    elif j == 3:
        paths = [tuple(int(x) for x in rs.randint(0, 2, int(rs.randint(1, D + 1)))) for w in range(W)]
    else:
        paths = [chain[:2] + chain[2:2 + (w % 3)] if w < 3 else tuple([(chain[0] + 1 + w) % BACKUP_K] * (1 + w % 2)) for w in range(W)]
        paths = [p[:D] for p in paths]
    ends = ["none" if (len(p) == D or (w + j) % 3 == 0) else "leaf" for w, p in enumerate(paths)]
    return paths, ends


def build_backup(name, form):
    """The tables in front of ipp_mcts_backup for the case, declared for the wave kernel (form "wave": tables.wave x max_depth <= 64)
    or the serial kernel (form "serial": a larger tables.wave, the same descents and the same wave argument).  Returns (tables, W)."""
    W, D, wave_w, wave_s, gamma = BACKUP_CASES[name]
    wave = wave_w if form == "wave" else wave_s
    assert (wave * D <= 64) == (form == "wave") and W <= wave
    R, npr = 5, 72
    st = blank_tables(R, BACKUP_KMAX, 11, npr=npr, D=D, wave=wave, horizon=min(D - 1, 5), gamma=gamma, seed=2)
    rs = np.random.RandomState(1000 + 17 * W + D)
    virtual = W > 1
    for j in range(R):
        paths, ends = backup_descents(W, D, j, rs)
        nodes = {(): j * npr}  # prefix -> node

        def node_of(prefix):
            if prefix not in nodes:
                nodes[prefix] = j * npr + len(nodes)
                assert len(nodes) <= npr
            return nodes[prefix]

        def expand(nd):
            if st["n_flags"][nd] & EXPANDED:
                return
            st["n_flags"][nd] |= EXPANDED
            st["n_k"][nd] = BACKUP_K
            st["t_idx"][nd, :BACKUP_K] = np.sort(rs.choice(11, BACKUP_K, replace=False))
            st["t_ps"][nd, :BACKUP_K] = 1.0 / BACKUP_K
            nsa = rs.choice([0.0, 0.0, 1.0, 3.0], BACKUP_K)
            st["t_nsa"][nd, :BACKUP_K] = nsa
            st["t_qsa"][nd, :BACKUP_K] = np.where(nsa > 0, rs.uniform(-1, 1, BACKUP_K), 0.0)
            st["t_num"][nd, :BACKUP_K] = rs.uniform(0.1, 2.0, BACKUP_K)
            st["n_ns"][nd] = nsa.sum() + float(rs.randint(0, 3))

        st["root_count"][j] = 1
        for w, (p, end) in enumerate(zip(paths, ends)):
            for s in range(len(p)):
                nd = node_of(p[:s])
                expand(nd)
                st["p_node"][w, j, s], st["p_k"][w, j, s] = nd, p[s]
                # the cost belongs to the edge and the way to it: one value per (prefix, slot); every third edge costs 0
                st["p_cost"][w, j, s] = 0.0 if (sum(p[:s + 1]) + s) % 3 == 0 else 1.0 + 0.37 * ((7 * sum(p[:s + 1]) + 3 * s) % 11)
                st["t_child"][nd, p[s]] = node_of(p[:s + 1])
                if virtual:
                    st["t_nsa"][nd, p[s]] += 1
                    st["n_ns"][nd] += 1
            st["p_len"][w, j] = len(p)
            lf = -1
            if end == "leaf":
                lf = node_of(p)
                if st["n_flags"][lf] & EXPANDED:
                    lf = -1  # (another descent goes on through it: this one ended on its budget)
                else:
                    st["n_value"][lf] = 0.3 + 0.05 * (lf % 7)
            st["leaf"][w, j] = lf
        st["root_count"][j] = len(nodes)
    # what select leaves for the backup to clear
    st["counts"][:R] = np.minimum(W, 1 + np.arange(R) % 2)
    st["counts"][R] = 3
    return st, W


def edge_positions(st, W):
    """{(node, k): set of step indices} over all recorded descents: the invariant the wave backup rests on is one index per edge."""
    pos = {}
    for w in range(W):
        for j in range(st["roots"]):
            for s in range(int(st["p_len"][w, j])):
                pos.setdefault((int(st["p_node"][w, j, s]), int(st["p_k"][w, j, s])), set()).add(s)
    return pos


# ---------------------------------------------------------------------------------------------------- read-out cases
READOUT_CASES = {}
TEMPERATURES = (1.0, 0.5, 2.0, 0.25)
ALMOST_ONE = 1.0 - 2.0 ** -53


def _readout_tables(kmax, A, rows, seed=0, **kw):
    """rows: per root dict(idx, ps, nsa, q, ns) or None (unexpanded) -> tables of len(rows) roots, two nodes per root."""
    st = blank_tables(len(rows), kmax, A, npr=2, D=1, wave=1, horizon=0, seed=seed, **kw)
    tb = TreeBuilder(st, seed)
    for j, r in enumerate(rows):
        if r is None:
            continue
        if len(r["idx"]) == 0:  # expanded with an empty valid set
            st["n_flags"][tb.node(j, 0)] |= EXPANDED
            continue
        tb.expand(j, 0, r["idx"], r["ps"], r["nsa"], r["q"], r["ns"])
    return st


def _searched_row(rs, K, A, q_kind, ns_scale=1.0):
    """A root row the way a search leaves it: visits that sum to Ns, priors that sum to 1 on the valid set, Q = 0 where nothing was
    visited (the all-positive and all-negative rows have every action visited)."""
    ps, nsa, q, ns = random_row(rs, K, q_kind, visited=1.0 if q_kind in ("positive", "negative") else 0.7)
    nsa = np.floor(nsa * ns_scale)
    return dict(idx=np.sort(rs.choice(A, K, replace=False)), ps=ps, nsa=nsa, q=np.where(nsa > 0, q, 0.0) if q_kind != "flat" else q, ns=float(nsa.sum()))


def _ro(name):
    def deco(f):
        READOUT_CASES[name] = f
        return f
    return deco


def _sizes_case(kmax):
    """5 roots: K == kmax == A is impossible together with K < A in one table (A is one number), so A = kmax and root 0 has K == A
    (flat non-zero Q), roots 1-4 K < A: K = 1, and all-zero / positive / negative / mixed Q."""
    rs = np.random.RandomState(300 + kmax)
    Ks = [kmax, 1, max(2, kmax - 1), max(2, kmax // 2 + 1), max(2, min(kmax - 1, 66))]
    rows = [_searched_row(rs, K, kmax, kind, ns_scale=6.0) for K, kind in zip(Ks, ("flat", "positive", "zero", "negative", "mixed"))]
    rows[1]["nsa"][:] = 5.0
    rows[1]["ns"] = 5.0
    st = _readout_tables(kmax, kmax, rows, seed=kmax)
    return dict(st=st, tie_u=rs.uniform(size=5))


for _kmax in (5, 64, 65, 130):
    READOUT_CASES[f"kmax-{_kmax}"] = (lambda kmax=_kmax: _sizes_case(kmax))


def _tie_row(K, A, ties, top=9.0, rs=None):
    nsa = rs.randint(0, 5, K).astype(np.float64)
    nsa[np.asarray(ties)] = top
    ps = rs.uniform(0.2, 1.0, K)
    ps /= ps.sum()
    return dict(idx=np.arange(K) + (A - K), ps=ps, nsa=nsa, q=np.where(nsa > 0, rs.uniform(-1, 1, K), 0.0), ns=float(nsa.sum()))


def _ties_case(us):
    """kmax 130, K 130 < A: 1 tie; 2 ties; many ties through all three 64-lane chunks; ties in the second chunk only; in the third only."""
    rs = np.random.RandomState(77)
    layouts = ([17], [3, 100], list(range(2, 130, 7)), [64, 70, 99, 127], [128, 129])
    rows = [_tie_row(130, 150, t, rs=rs) for t in layouts]
    st = _readout_tables(130, 150, rows, seed=21)
    return dict(st=st, tie_u=None if us is None else np.asarray(us, np.float64), layouts=layouts)


def u_for(i, n):
    """A uniform whose pick among n ties is the i-th."""
    return (i + 0.5) / n


_MANY = len(range(2, 130, 7))  # 19 ties: k = 2 .. 128; chunk 0: 2 .. 58 (9), chunk 1: 65 .. 121 (9), chunk 2: 128 (1)
READOUT_CASES["ties-u0"] = lambda: _ties_case([0.0] * 5)
READOUT_CASES["ties-u-almost-1"] = lambda: _ties_case([ALMOST_ONE] * 5)
# root 0 stays inside its own row even if a pick were not clamped (row - 1 is below the buffer), so it gets no u of 1
READOUT_CASES["ties-u-1"] = lambda: _ties_case([0.5, 1.0, 1.0, 1.0, 1.0])
READOUT_CASES["ties-null"] = lambda: _ties_case(None)
READOUT_CASES["ties-first-of-chunk-1"] = lambda: _ties_case([0.3, u_for(1, 2), u_for(9, _MANY), u_for(0, 4), u_for(0, 2)])
READOUT_CASES["ties-last-of-chunk-1"] = lambda: _ties_case([0.3, u_for(1, 2), u_for(17, _MANY), u_for(3, 4), u_for(1, 2)])
READOUT_CASES["ties-last-of-chunk-0"] = lambda: _ties_case([0.3, u_for(0, 2), u_for(8, _MANY), u_for(2, 4), u_for(1, 2)])
READOUT_CASES["ties-chunk-2"] = lambda: _ties_case([0.3, u_for(1, 2), u_for(18, _MANY), u_for(1, 4), u_for(0, 2)])


@_ro("take-back")
def _take_back():
    """K = 6 < A, the kept action k = 0 (most visited, the best Q).  Root 0: k = 1 is taken back completely (2 -> 1 -> 0, the loop
    ends on the infinite prior of 1 + (-1) == 0); k = 2 stops early on the comparison; k = 3 meets the kept action's score exactly at
    its first step (same Q, half the prior over half the denominator: powers of two, so the products are the same numbers) and keeps its
    visits; k = 4 owes two playouts, ends at one visit and is dropped; k = 5 starts at one visit and is dropped.  Root 1: negative Q.  Root
    2: a flat row: every other action is owed playouts but stays above the kept action."""
    ns = 400.0
    ps = np.array([0.25, 0.02, 0.2, 0.125, 0.004, 0.401])
    nsa = np.array([7.0, 2.0, 6.0, 4.0, 3.0, 1.0])
    q = np.array([0.9, 0.0, 0.85, 0.9, 0.05, 0.1])
    rows = [dict(idx=np.arange(6), ps=ps, nsa=nsa, q=q, ns=ns), _searched_row(np.random.RandomState(9), 6, 8, "negative", 6.0),
            dict(idx=np.arange(6) + 2, ps=np.full(6, 1 / 6), nsa=np.array([5.0, 5.0, 4.0, 4.0, 3.0, 3.0]), q=np.full(6, 0.5), ns=24.0)]
    st8 = _readout_tables(6, 8, rows, seed=31)
    return dict(st=st8, tie_u=np.array([0.0, 0.0, 0.7]))


@_ro("take-back-K-eq-A")
def _take_back_full():
    c = _take_back()
    st = c["st"]
    rows = [dict(idx=np.arange(6), ps=st["t_ps"][2 * j, :6].copy(), nsa=st["t_nsa"][2 * j, :6].copy(), q=st["t_qsa"][2 * j, :6].copy(),
                 ns=float(st["n_ns"][2 * j])) for j in range(3)]
    return dict(st=_readout_tables(6, 6, rows, seed=32), tie_u=c["tie_u"])


@_ro("bad-roots")
def _bad_roots():
    """Root 0: K = 1 with one visit (dropped: ok = 0, a row of zeros).  Root 1: unexpanded.  Root 2: expanded with K = 0.  Root 3: no
    visit at all with K < A (nothing kept: vmax == 0).  Root 4: a healthy row between them."""
    rs = np.random.RandomState(5)
    rows = [dict(idx=[3], ps=[1.0], nsa=[1.0], q=[0.2], ns=1.0), None, dict(idx=[], ps=[], nsa=[], q=[], ns=0.0),
            dict(idx=[1, 4, 6], ps=[0.5, 0.25, 0.25], nsa=[0.0, 0.0, 0.0], q=[0.0, 0.0, 0.0], ns=0.0), _searched_row(rs, 5, 9, "mixed", 4.0)]
    return dict(st=_readout_tables(7, 9, rows, seed=33), tie_u=np.array([0.1, 0.2, 0.3, 0.4, 0.5]))


@_ro("no-visits-K-eq-A")
def _no_visits_full():
    """vmax == 0 with K == A: an action is kept among the K ties, nothing is visited, ok = 0.  Beside a visited K == A row."""
    rs = np.random.RandomState(6)
    rows = [dict(idx=np.arange(5), ps=np.full(5, 0.2), nsa=np.zeros(5), q=np.zeros(5), ns=0.0), _searched_row(rs, 5, 5, "positive", 4.0),
            dict(idx=np.arange(5), ps=np.full(5, 0.2), nsa=np.zeros(5), q=np.zeros(5), ns=3.0)]
    return dict(st=_readout_tables(5, 5, rows, seed=34), tie_u=np.array([0.5, 0.5, ALMOST_ONE]))


def build_readout(name):
    c = READOUT_CASES[name]()
    validate(c["st"])
    return c


def readout_modes(name):
    """(temperature, deploy_time, want_idx) of the launches of a read-out case: every case at temperature 1 in training mode; the size
    and take-back cases at the other temperatures and at deploy time as well."""
    modes = [(1.0, 0, True)]
    if name.startswith("kmax-") or name.startswith("take-back") or name == "bad-roots":
        modes += [(0.5, 0, False), (2.0, 0, True), (0.25, 0, True), (1.0, 1, True), (0.5, 1, False)]
    return modes
