"""
CPU-only: the restatements of tests/mcts_table_cases.py (select_ref, backup_ref, policy_ref) against the reference's own compute_uct,
normalize_q_values and get_policy (tests/golden/mcts_tables.npz, gen_mcts_tables_golden.py), against the host drivers' arithmetic
(VectorMCTS._uct_rows, VectorMCTS._policy_sparse, DeviceMCTS._policies_rows) and, composed into a whole search, against
VectorMCTS.get_policy; and the frozen cases against the edges of csrc/k_mcts.h that tests/test_hip_mcts_tables.py names them for,
proved from the instrumentation the restatements return.  A case that stops reaching its edge (another seed, another size) fails
here, not silently on the GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mcts_table_cases as mc
from tests.conftest import load_golden
from tests.golden.gen_mcts_tables_golden import SCORE_CASES, digest
from tests import test_mcts_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_imports_without_torch():
    code = "import sys; import tests.mcts_table_cases; sys.exit(int('torch' in sys.modules or 'ipp_rl_amd' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def dense(st, node, values, fill):
    K = int(st["n_k"][node])
    out = np.full(st["num_actions"], fill, dtype=np.float64)
    out[st["t_idx"][node, :K]] = values
    return out


# ---------------------------------------------------------------------------------------------------- against the reference
def test_fixture_belongs_to_the_cases():
    g = load_golden("mcts_tables")
    for case in SCORE_CASES:
        assert np.array_equal(g[f"digest/sel/{case}"], digest(mc.SELECT_CASES[case]()["st"])), case
    for case in mc.READOUT_CASES:
        assert np.array_equal(g[f"digest/ro/{case}"], digest(mc.READOUT_CASES[case]()["st"])), case
    assert not [k for k in g.files if k.split("/")[0] not in ("digest", "sel", "ro")]


@pytest.mark.parametrize("case", SCORE_CASES)
def test_select_scores_equal_the_reference_bit_for_bit(case):
    g = load_golden("mcts_tables")
    st = mc.SELECT_CASES[case]()["st"]
    nodes = np.nonzero(st["n_flags"] & mc.EXPANDED)[0]
    assert len(nodes) >= st["roots"] - 1
    for node in nodes:
        K = int(st["n_k"][node])
        for force in (0, 1):
            uct, _, _ = mc.uct_scores(st, node, force=bool(force))
            assert mc.same_bits(dense(st, node, uct, -np.inf), g[f"sel/{case}/{node}/uct{force}"]), (case, node, force)
        qn, _ = mc.normalize_q(st["t_qsa"][node, :K], K, st["num_actions"])
        assert mc.same_bits(qn, g[f"sel/{case}/{node}/qn"][st["t_idx"][node, :K]]), (case, node)   # (on the valid set)


@pytest.mark.parametrize("case", list(mc.READOUT_CASES))
def test_policy_ref_equals_the_reference(case):
    g = load_golden("mcts_tables")
    c = mc.build_readout(case)
    st = c["st"]
    R, npr = st["roots"], st["nodes_per_root"]
    recorded = [j for j in range(R) if f"ro/{case}/{j}/kept" in g.files]
    assert recorded == [j for j in range(R) if st["n_flags"][j * npr] & mc.EXPANDED]
    tie_u = np.array([float(g[f"ro/{case}/{j}/tie_u"]) if j in recorded else 0.0 for j in range(R)])
    for t, d, _ in mc.readout_modes(case):
        policy, idx, ok, info = mc.policy_ref(st, tie_u, t, d)
        for j in recorded:
            want = g[f"ro/{case}/{j}/T{t}d{d}"]
            assert bool(ok[j]) == (want.size > 0), (case, j, t, d)
            if not d and info[j].get("best") is not None:
                kept = int(g[f"ro/{case}/{j}/kept"])
                assert kept == (int(idx[j, info[j]["best"]]) if info[j]["best"] >= 0 else -1), (case, j)
            if not ok[j]:
                assert not policy[j].any()
                continue
            got = dense(st, j * npr, policy[j, :int(st["n_k"][j * npr])], 0.0)
            if t == 1.0:
                assert mc.same_bits(got, want), (case, j, t, d, np.abs(got - want).max())
            else:
                assert np.abs(got - want).max() <= 1e-15, (case, j, t, d, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------- against the host drivers
class PickRng:
    """np.random-like: choice() picks among the ties with the given uniform (like policy_ref), gamma() draws nothing."""

    def __init__(self, u):
        self.u = u

    def choice(self, ties):
        return mc.pick_tie(np.asarray(ties), self.u)

    def random_sample(self, n):
        return np.asarray(self.u, dtype=np.float64)

    def gamma(self, shape, size=None):
        return 1.0 if size is None else np.ones(size)


def host_object(cls, st, rows):
    """A driver object holding the given node rows as its tables (no engine, no search)."""
    m = cls.__new__(cls)
    m.actions_np = st["actions"]
    m.puct_init, m.puct_base, m.fpf, m.max_dist = st["puct_init"], st["puct_base"], st["fpf"], 11.5
    m.t_idx, m.t_Ps, m.t_Nsa, m.t_Qsa = st["t_idx"][rows].astype(np.int64), st["t_ps"][rows], st["t_nsa"][rows], st["t_qsa"][rows]
    m.n_K, m.n_Ns, m.n_expanded = st["n_k"][rows].astype(np.int64), st["n_ns"][rows], (st["n_flags"][rows] & mc.EXPANDED).astype(bool)
    return m


@pytest.mark.parametrize("case", list(mc.SELECT_CASES))
def test_select_scores_equal_the_vector_driver(case):
    from ipp_rl_amd.planning.mcts_zero.vector_mcts import VectorMCTS

    st = mc.SELECT_CASES[case]()["st"]
    nodes = np.nonzero(st["n_flags"] & mc.EXPANDED)[0]
    m = host_object(VectorMCTS, st, np.arange(len(st["n_k"])))
    for force in (False, True):
        with np.errstate(all="ignore"):
            rows = m._uct_rows(nodes, force_playouts=force)
        for node, row in zip(nodes, rows):
            K = int(st["n_k"][node])
            uct, _, _ = mc.uct_scores(st, node, force=force)
            assert mc.same_bits(row[:K], uct) and np.all(row[K:] == -np.inf), (case, node, force)


@pytest.mark.parametrize("case", list(mc.READOUT_CASES))
def test_policy_ref_equals_the_host_read_outs(case):
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS
    from ipp_rl_amd.planning.mcts_zero.vector_mcts import VectorMCTS

    c = mc.build_readout(case)
    st, tie_u = c["st"], c["tie_u"]
    R, npr = st["roots"], st["nodes_per_root"]
    roots = np.arange(R) * npr
    for t, d, _ in mc.readout_modes(case):
        policy, idx, ok, _ = mc.policy_ref(st, tie_u, t, d)
        v = host_object(VectorMCTS, st, np.arange(len(st["n_k"])))
        dm = host_object(DeviceMCTS, st, roots)
        dm._shared_rng = PickRng(np.zeros(R) if tie_u is None else tie_u)
        with np.errstate(all="ignore"):
            rows = dm._policies_rows(R, t, bool(d), None)
        for j in range(R):
            K = int(st["n_k"][roots[j]])
            with np.errstate(all="ignore"):
                one = v._policy_sparse(int(roots[j]), np.array([2.0, 2.0, 14.0]), 50.0, t, bool(d), PickRng(None if tie_u is None else float(tie_u[j])))
            assert (one is None) == (rows[j] is None) == (not ok[j]), (case, j, t, d)
            if not ok[j]:
                continue
            assert mc.same_bits(np.asarray(one[0])[idx[j, :K]], policy[j, :K]), (case, j, t, d)
            got = np.zeros(K)
            for a, p in rows[j][0].items():
                got[int(np.nonzero(idx[j, :K] == a)[0][0])] = p
            assert np.array_equal(rows[j][1], idx[j, :K])
            if t == 1.0:
                assert mc.same_bits(got, policy[j, :K]), (case, j, d)
            else:  # (the row-wise read-out sums the padded row)
                assert np.abs(got - policy[j, :K]).max() <= 1e-15, (case, j, t, d)


@pytest.mark.parametrize("W", [1, 4])
def test_a_search_composed_of_the_restatements_is_the_vector_drivers(W):
    """select_ref + the host's valid sets with uniform priors + MockEngine rewards + backup_ref + policy_ref, wave by wave, against
    VectorMCTS.get_policy(tie_break="first"): the roots' Nsa, Qsa, Ns and the policies bit for bit."""
    from ipp_rl_amd.planning.mcts_zero.vector_mcts import VectorMCTS

    dim, R, S = 60, 4, 28
    hyper, meta = host.setup(dim, S, 0.0)
    rs = np.random.RandomState(1)
    prev0 = np.stack([4.0 * rs.randint(0, dim, R) + 2, 4.0 * rs.randint(0, dim, R) + 2, np.full(R, 14.0)], 1)
    budget0 = np.full(R, 60.0)
    tie_u = np.array([0.1, 0.6, 0.95, 0.4])
    v = VectorMCTS(host.MockEngine(dim), hyper, meta, host.stub, sims_in_flight=W, tie_break="first")
    out = v.get_policy(list(range(R)), prev0, budget0, rngs=[PickRng(float(u)) for u in tie_u])
    A, kmax, npr, D = v.num_actions, int(min(v.Kmax, v.num_actions)), 2 * S + 2 * W + 8, v.horizon + 1
    assert A > v.DENSE_ACTIONS
    st = mc.blank_tables(R, kmax, A, npr=npr, D=D, wave=W, horizon=v.horizon, dev_per_root=npr, gamma=v.gamma, puct_init=v.puct_init,
                         puct_base=v.puct_base, fpf=v.fpf, ns_table="absent")
    st["actions"], st["zkey"] = v.actions_np, v._z
    st.update(use_flight_time=1, vmax=float(meta["uav_specifications"]["max_v"]), amax=float(meta["uav_specifications"]["max_a"]))
    eng, sim, x = host.MockEngine(dim), 0, 1.0 / A
    while sim < S:
        w = min(W, S - sim)
        st, requests, _ = mc.select_ref(st, np.arange(R), prev0, budget0, 0, sim, w, 0)
        for root, parent, k, child, newdev, cost, prev, action, path in requests:
            r, _ = eng.tree_step(np.array([root]), path[None], action[None], prev[None], new_ids=np.array([newdev]))
            st["t_num"][parent, k] = float(r.numpy()[0]) * (cost + 1.0)
        for j in range(R):
            for s in range(int(st["counts"][j])):
                nd = int(st["pend_node"][j, s])
                idx, K = v.valid_sets(st["pend_prev"][j, s][None], st["pend_budget"][j, s][None])
                K = int(K[0])
                if K == 0:
                    continue  # mcts.py:201-202: stays a leaf worth 0
                st["t_idx"][nd], st["t_idx"][nd, :K] = -1, idx[0, :K]
                st["t_ps"][nd, :K] = x / float(np.sum(np.full(K, x)))
                st["t_nsa"][nd, :K], st["t_qsa"][nd, :K], st["t_num"][nd, :K], st["t_child"][nd, :K] = 0.0, 0.0, np.nan, -1
                st["n_k"][nd], st["n_ns"][nd], st["n_value"][nd] = K, 0.0, 0.3 + 0.05 * (K % 7)
                st["n_flags"][nd] |= mc.EXPANDED
        st, _ = mc.backup_ref(st, w)
        sim += w
    assert not st["err"].any()
    policy, idx, ok, _ = mc.policy_ref(st, tie_u, 1.0, 0)
    for j in range(R):
        rt, nd = int(v.root_ids[j]), j * npr
        K = int(v.n_K[rt])
        assert K == st["n_k"][nd] and np.array_equal(v.t_idx[rt, :K], st["t_idx"][nd, :K])
        assert mc.same_bits(v.t_Nsa[rt, :K], st["t_nsa"][nd, :K]) and mc.same_bits(v.t_Qsa[rt, :K], st["t_qsa"][nd, :K]), j
        assert v.n_Ns[rt] == st["n_ns"][nd] == S - W and ok[j] and out[j] is not None
        got = {int(idx[j, k]): float(policy[j, k]) for k in range(K) if policy[j, k] > 0}
        assert got == out[j][0], j
    assert eng.steps == v.stats["device_steps"]


# ---------------------------------------------------------------------------------------------------- select cases reach their edges
def levels_of(info):
    return [(j, w, i, lv) for (j, w), levels in sorted(info.items()) for i, lv in enumerate(levels) if "k" in lv]


@pytest.mark.parametrize("name", list(mc.SELECT_CASES))
def test_margin_rule_holds_for_every_select_case(name):
    c, want, requests, info = mc.build_select(name)  # (asserts the rule)
    lv = levels_of(info)
    assert lv or name == "none"
    assert all(x["gap"] >= mc.MARGIN and x["identical_ties"] for _, _, _, x in lv)
    assert c["st"]["roots"] >= 3


def test_select_cases_reach_every_instantiation_and_register_slot():
    slots = {}
    for kmax, ne in ((64, 1), (65, 2), (130, 3), (256, 4), (257, 0)):
        c, want, _, info = mc.build_select(f"kmax-{kmax}")
        st = c["st"]
        assert st["kmax"] == kmax and ((kmax + 63) // 64 if kmax <= 256 else 0) == ne and st["roots"] == 5
        assert st["n_k"][0] == kmax == st["num_actions"] and all(st["n_k"][j * st["nodes_per_root"]] < kmax for j in range(1, 5))
        slots[kmax] = {lv["slot"] for _, _, _, lv in levels_of(info)}
        branches = {lv["branch"] for _, _, _, lv in levels_of(info)}
        assert {"allzero", "flat", "range-positive-widened", "range-negative-widened", "range-mixed"} <= branches, (kmax, branches)
        assert any(len(levels) == 3 for levels in info.values()) and want["counts"][-1] > 0   # three levels deep; first traversals
    assert slots[64] == {0} and {1, 2} <= slots[130] and 3 in slots[256] and max(slots[257]) >= 3


def test_forced_playout_ties_sit_where_the_tie_path_matters():
    c, want, _, info = mc.build_select("forced-ties")
    first = {j: info[(j, 0)][0] for j in range(4)}
    for j in range(4):
        assert first[j]["lane_tie"] and first[j]["winner_forced"] and first[j]["forced"] >= 2 and np.isinf(first[j]["gap"])
    assert [first[j]["k"] for j in range(4)] == [10, 3, 5, 70]
    assert [first[j]["lowest_k_on_lowest_lane"] for j in range(4)] == [False, False, True, False]
    assert first[3]["k"] >= 64 and first[3]["lane"] == 6           # the winner's k is not its lane: `& 63`
    # the virtual visits work the ties off: a later descent of every root meets fewer of them
    assert all(info[(j, 3)][0]["forced"] < first[j]["forced"] for j in range(4))
    off, want_off, _, info_off = mc.build_select("forced-off")
    for k in mc.EDGE_TABLES + mc.NODE_TABLES:
        assert mc.same_bits(off["st"][k], c["st"][k]), k               # the same rows ...
    assert off["depth0"] == 1 and all(lv["forced"] == 0 and not lv["lane_tie"] for _, _, _, lv in levels_of(info_off))
    assert all(info_off[(j, 0)][0]["k"] != first[j]["k"] for j in range(4))  # ... another winner


@pytest.mark.parametrize("name", ["tie-break-random", "tie-break-random-256", "tie-break-random-300", "random-ties-257"])
def test_random_tie_break_cases_draw_with_the_high_keys(name):
    """The winner of every tied level is the largest draw; in each case a lane holds an earlier tied edge than the winner (the lane has
    to replace its record on the draw alone), also at kmax > 256 (the general kernel form)."""
    c, want, _, info = mc.build_select(name)
    st = c["st"]
    assert st["tie_break"] == 1 and c["seed"] and (name == "random-ties-257" or (st["root_base"] != 0 and c["sim0"] != 0 and c["seed"] >> 32))
    tied, lows, replaced = [], 0, 0
    for j, w, i, lv in levels_of(info):
        if lv["n_top"] > 1 and i == 0:
            before = mc.select_ref(st, c["root_env"], c["prev0"], c["budget0"], c["depth0"], c["sim0"], w, c["seed"])[0] if w else st
            if w == 1:  # (a single descent leaves no virtual visit: take the first of two)
                before = mc.copy_tables(st)
                first = info[(j, 0)][0]
                before["t_nsa"][first["node"], first["k"]] += 1
                before["n_ns"][first["node"]] += 1
            uct, _, _ = mc.uct_scores(before, lv["node"], force=True)
            top = np.nonzero(uct == uct.max())[0]
            assert len(top) == lv["n_top"], (name, j, w)
            draws = [mc.tie_draw(st, c["seed"], lv["node"], int(k), c["sim0"] + w) for k in top]
            assert lv["k"] == int(top[int(np.argmax(draws))]), (name, j, w)
            tied.append(lv)
            lows += lv["k"] == int(top[0])
            replaced += any(t % 64 == lv["k"] % 64 and t < lv["k"] for t in top)
    assert len(tied) >= 4 and lows < len(tied) / 2 and replaced >= 1, (name, len(tied), lows, replaced)
    if name != "random-ties-257":
        assert info[(0, 0)][0]["n_top"] == st["kmax"] and any(lv["winner_forced"] for lv in tied) and max(lv["slot"] for lv in tied) >= 2


def test_ns_table_cases_take_the_table_the_kernel_or_both():
    got = {}
    for name in ("kmax-65", "table-absent", "table-short"):
        c, _, _, info = mc.build_select(name)
        got[name] = [lv["ns_from_table"] for _, _, _, lv in levels_of(info)]
    assert all(got["kmax-65"]) and not any(got["table-absent"]) and any(got["table-short"]) and not all(got["table-short"])
    a, s = mc.SELECT_CASES["table-absent"]()["st"], mc.SELECT_CASES["table-short"]()["st"]
    assert all(mc.same_bits(a[k], s[k]) for k in mc.EDGE_TABLES + mc.NODE_TABLES)


def test_wave_cases_show_the_virtual_visits():
    c, want, _, info = mc.build_select("w1")
    assert c["W"] == 1 and mc.same_bits(want["t_nsa"], c["st"]["t_nsa"]) and mc.same_bits(want["n_ns"], c["st"]["n_ns"])
    for name, W in (("kmax-64", 4), ("w8", 8)):
        c, want, _, info = mc.build_select(name)
        assert c["W"] == W
        plen = want["p_len"][:W]
        assert np.nansum(want["t_nsa"]) - np.nansum(c["st"]["t_nsa"]) == plen.sum() == want["n_ns"].sum() - c["st"]["n_ns"].sum()
        # the next descent takes another first edge than the one before (the planted winners of roots 2 and 3 may stay ahead)
        moved = [j for j in range(5) if any(info[(j, w)][0]["k"] != info[(j, w + 1)][0]["k"] for w in range(W - 1))]
        assert len(moved) >= 3 and {0, 1, 4} <= set(moved), (name, moved)


def test_budget_and_horizon_case():
    c, want, _, info = mc.build_select("budget-horizon")
    D = c["st"]["max_depth"]
    assert info[(0, 0)] == [dict(end="budget")] and want["p_len"][0, 0] == 0 and want["leaf"][0, 0] == -1
    assert all(want["p_len"][w, 1] == 1 and want["leaf"][w, 1] == -1 and info[(1, w)][-1] == dict(end="budget") for w in (0, 1))
    assert any(info[(2, w)][-1] == dict(end="horizon") and want["p_len"][w, 2] == D and want["leaf"][w, 2] == -1 for w in (0, 1))
    for j, depth in ((3, 0), (4, 1)):  # two descents end at one leaf: one pending entry
        ends = [info[(j, w)][-1] for w in (0, 1)]
        assert [e["pending_seen"] for e in ends] == [False, True] and want["counts"][j] == 1 and want["pend_depth"][j, 0] == depth
        assert want["leaf"][0, j] == want["leaf"][1, j] == want["pend_node"][j, 0] >= 0


def test_first_traversal_case():
    c, want, requests, info = mc.build_select("first-traversal")
    st = c["st"]
    why = {j: [lv["request"] for lv in info[(j, 0)] if "request" in lv] for j in range(5)}
    assert why == {0: ["new"], 1: ["new"], 2: ["stored"], 3: ["horizon"], 4: ["exhausted"]}
    assert [lv["d"] for lv in info[(1, 0)] if "request" in lv] == [1] and [lv["d"] for lv in info[(3, 0)] if "request" in lv] == [2]
    assert want["err"].tolist() == [0, 1, 0, 0] and len(requests) == 5 == want["counts"][-1]
    by_root = {r[0]: r for r in requests}
    assert by_root[7][4] == 40 and by_root[6][4] == 43 and [by_root[e][4] for e in (5, 4, 3)] == [-1, -1, -1]
    assert want["n_devpath"][by_root[7][3]].tolist() == [40, -1, -1, -1, -1, -1]
    assert want["n_devpath"][by_root[6][3]].tolist() == [42, 43, -1, -1, -1, -1]                # written at its depth
    assert np.isinf(want["t_num"]).sum() == 5 and not np.isinf(st["t_num"]).any()
    assert info[(2, 0)][0]["found"] and want["n_flags"][by_root[4][3]] & mc.STORED == 0          # root 3's child at the horizon stays unstored


def test_transposition_case():
    c, want, requests, info = mc.build_select("transposition")
    st = c["st"]
    npr, tsz = st["nodes_per_root"], st["table_size"]
    assert info[(0, 0)][0]["found"] is False and want["root_count"][0] == 2
    second = info[(1, 0)][1]
    assert second["found"] is True and want["root_count"][1] == st["root_count"][1] == 4
    # ... the node found is the one below the OTHER parent's edge
    other = st["t_child"][npr + 1, 0]
    assert want["t_child"][second["node"], second["k"]] == other >= 0 and second["node"] != npr + 1
    assert info[(2, 0)][0]["key_zero"] and want["n_hash"][want["t_child"][2 * npr, 0]] == 1
    third = info[(3, 0)][0]
    assert third["wrapped"] and third["probes"] == 4 and want["h_keys"][3, 2] != 0 and st["h_keys"][3, 2] == 0
    assert want["h_vals"][3, 2] == want["t_child"][3 * npr, 0] == 3 * npr + 1 and (want["h_keys"][3] != 0).sum() == 4
    assert info[(4, 0)][0].get("nodes_exhausted") and want["err"].tolist() == [1, 0, 0, 0] and want["t_child"][4 * npr, info[(4, 0)][0]["k"]] == 4 * npr
    assert want["p_len"][0, 4] == 3 and np.all(want["p_node"][0, 4] == 4 * npr)


# ---------------------------------------------------------------------------------------------------- backup cases reach their edges
def test_backup_cases_reach_both_kernels_and_their_lanes():
    seen = dict(share=set(), zero=0, full=0, noleaf=0, leaf=0, first=0, mean=0, cost0=0, fan=0, gammas=set())
    for name, (W, D, wave_w, wave_s, gamma) in mc.BACKUP_CASES.items():
        a, _ = mc.build_backup(name, "wave")
        b, _ = mc.build_backup(name, "serial")
        assert a["wave"] * D <= 64 < b["wave"] * D and a["roots"] == 5
        for k in mc.ARRAYS:  # the same recorded descents and tables in both forms (the per-wave buffers differ in size only)
            if k[:2] in ("t_", "n_") or k in ("actions", "zkey", "err"):
                assert mc.same_bits(a[k], b[k]), (name, k)
        for k in ("p_node", "p_k", "p_cost", "p_len", "leaf"):
            assert mc.same_bits(a[k][:W], b[k][:W]), (name, k)
        mc.validate(a, W), mc.validate(b, W)
        assert all(len(s) == 1 for s in mc.edge_positions(a, W).values()), name   # the invariant of the wave form
        want, info = mc.backup_ref(a, W)
        assert not want["counts"].any() and a["counts"].all()
        plen = a["p_len"][:W]
        seen["zero"] += int((plen == 0).sum()); seen["full"] += int((plen == D).sum())
        seen["noleaf"] += int(((a["leaf"][:W] == -1) & (plen > 0)).sum()); seen["leaf"] += int((a["leaf"][:W] >= 0).sum())
        seen["cost0"] += int(sum((a["p_cost"][w, j, :plen[w, j]] == 0).sum() for w in range(W) for j in range(5)))
        seen["gammas"].add(gamma)
        for j, edges in info.items():
            for (node, k), hits in edges.items():
                lengths = {int(plen[w, j]) for w, _, _ in hits}
                if len(hits) > 1 and len(lengths) > 1:
                    seen["share"].add(len(hits) if len(hits) < W else "all")
                seen["first"] += sum(1 for _, _, n in hits if n == 0)
                seen["mean"] += sum(1 for _, _, n in hits if n > 0)
                # the same edge, first without and then with a count
                seen["fan"] += int(len({kk for (nn, kk) in edges if nn == node}) > 1)
        if W > 1:  # the virtual visits were there and are gone
            for j in range(5):
                for (node, k), hits in info[j].items():
                    assert want["t_nsa"][node, k] == a["t_nsa"][node, k]
            assert mc.same_bits(want["n_ns"], a["n_ns"])
        else:
            assert want["n_ns"].sum() == a["n_ns"].sum() + plen.sum()
    assert {2, 3, "all"} <= seen["share"] and {1.0, 0.9} == seen["gammas"]
    assert all(seen[k] > 0 for k in ("zero", "full", "noleaf", "leaf", "first", "mean", "cost0", "fan")), seen
    W, D, wave_w, _, _ = mc.BACKUP_CASES["w8-d8"]
    a, _ = mc.build_backup("w8-d8", "wave")
    assert W * D == 64 == wave_w * D and (a["p_len"][7] == 8).any()                     # lane 63 holds a step
    assert 64 % mc.BACKUP_CASES["w4-d5-wave12"][1] and mc.BACKUP_CASES["w4-d5-wave12"][0] < mc.BACKUP_CASES["w4-d5-wave12"][2]
    assert 64 % mc.BACKUP_CASES["w3-d7"][1] and mc.BACKUP_CASES["w3-d6-wave5"][0] < mc.BACKUP_CASES["w3-d6-wave5"][2]
    assert mc.BACKUP_CASES["w1-d3"][0] == 1


# ---------------------------------------------------------------------------------------------------- read-out cases reach their edges
def readout_info(name, t=1.0, d=0):
    c = mc.build_readout(name)
    policy, idx, ok, info = mc.policy_ref(c["st"], c["tie_u"], t, d)
    return c, policy, ok, info


def test_readout_size_cases():
    for kmax in (5, 64, 65, 130):
        c, policy, ok, info = readout_info(f"kmax-{kmax}")
        st = c["st"]
        Ks = st["n_k"][::st["nodes_per_root"]].tolist()
        assert st["kmax"] == kmax == st["num_actions"] == Ks[0] and Ks[1] == 1 and all(K < kmax for K in Ks[1:]) and ok.all()
        assert info[0]["branch"] == "flat" and info[2]["branch"] == "allzero" and info[1]["branch"] == "range-positive-widened"
        assert info[3]["branch"] == "range-negative-widened" and (kmax == 5 or info[4]["branch"] == "range-mixed")
        assert np.isnan(st["t_nsa"][st["nodes_per_root"], 1:]).all() and (st["t_idx"][st["nodes_per_root"], 1:] == -1).all()
        assert any(n for i in info.values() for n, _ in i["taken"].values())
    assert [m[:2] for m in mc.readout_modes("kmax-65")] == [(1.0, 0), (0.5, 0), (2.0, 0), (0.25, 0), (1.0, 1), (0.5, 1)]
    assert {m[2] for m in mc.readout_modes("kmax-65")} == {True, False}


def test_readout_tie_cases():
    want = {"ties-u0": [17, 3, 2, 64, 128], "ties-null": [17, 3, 2, 64, 128], "ties-u-almost-1": [17, 100, 128, 127, 129],
            "ties-u-1": [17, 100, 128, 127, 129], "ties-first-of-chunk-1": [17, 100, 65, 64, 128], "ties-last-of-chunk-1": [17, 100, 121, 127, 129],
            "ties-last-of-chunk-0": [17, 3, 58, 99, 129], "ties-chunk-2": [17, 100, 128, 70, 128]}
    for name, best in want.items():
        c, policy, ok, info = readout_info(name)
        assert [info[j]["best"] for j in range(5)] == best and [info[j]["n_ties"] for j in range(5)] == [1, 2, 19, 4, 2] and ok.all(), name
        assert all(info[j]["min_margin"] >= mc.MARGIN for j in range(5)), name
    assert mc.build_readout("ties-null")["tie_u"] is None
    u = mc.build_readout("ties-u-almost-1")["tie_u"]
    assert np.all(u < 1.0) and np.all(np.nextafter(u, 2.0) == 1.0)
    assert mc.build_readout("ties-u-1")["tie_u"].tolist() == [0.5, 1.0, 1.0, 1.0, 1.0]   # (no u of 1 on root 0: see the case)
    c, _, _, info = readout_info("ties-first-of-chunk-1")
    assert (info[2]["chunk"], info[2]["rank_in_chunk"], info[2]["pick"]) == (1, 0, 9) and (info[3]["chunk"], info[3]["rank_in_chunk"]) == (1, 0)
    c, _, _, info = readout_info("ties-last-of-chunk-1")
    assert info[2]["chunk"] == 1 and info[2]["last_in_chunk"] and info[2]["rank_in_chunk"] == 8 and info[3]["last_in_chunk"]
    c, _, _, info = readout_info("ties-last-of-chunk-0")
    assert info[2]["chunk"] == 0 and info[2]["last_in_chunk"] and info[2]["rank_in_chunk"] == 8
    c, _, _, info = readout_info("ties-chunk-2")
    assert info[2]["chunk"] == 2 and info[2]["pick"] == 18 and info[4]["chunk"] == 2


def test_take_back_cases():
    for name, A in (("take-back", 8), ("take-back-K-eq-A", 6)):
        c, policy, ok, info = readout_info(name)
        assert c["st"]["num_actions"] == A and ok.all()
        assert info[0]["taken"] == {1: (2, "inf"), 2: (1, "above"), 3: (0, "equal"), 4: (2, "count"), 5: (0, "above")}
        assert info[0]["dropped_single"] == [4, 5] and info[0]["started_single"] == [5] and info[0]["best"] == 0
        assert policy[0].tolist() == [7 / 16, 0.0, 5 / 16, 4 / 16, 0.0, 0.0]
        assert info[2]["branch"] == ("flat" if A == 6 else "range-positive-widened") and info[2]["best"] == 1
        assert all(t == (0, "above") for t in info[2]["taken"].values()) and len(info[2]["taken"]) == 5
        assert all(i["min_margin"] >= mc.MARGIN for i in info.values())
    c, policy, ok, info = readout_info("take-back", d=1)   # deploy time: the visit counts as they are
    assert policy[0].tolist() == (c["st"]["t_nsa"][0, :6] / 23.0).tolist()


def test_bad_root_cases():
    c, policy, ok, info = readout_info("bad-roots")
    assert ok.tolist() == [0, 0, 0, 0, 1] and not policy[:4].any()
    assert [info[j]["bad"] for j in range(5)] == ["no visits", "unexpanded", "K=0", "no visits", ""]
    assert info[0]["dropped_single"] == [0] and info[3]["best"] == -1 and info[3]["vmax"] == 0 and c["st"]["n_k"][6] < c["st"]["num_actions"]
    c, policy, ok, info = readout_info("no-visits-K-eq-A")
    assert ok.tolist() == [0, 1, 0] and info[0]["vmax"] == 0 and info[0]["best"] == 2 and info[2]["best"] == 4 and info[0]["n_ties"] == 5
    assert all(c["st"]["n_k"][2 * j] == c["st"]["num_actions"] for j in range(3))


def test_every_readout_case_keeps_the_margin():
    for name in mc.READOUT_CASES:
        c, policy, ok, info = readout_info(name)
        assert c["st"]["roots"] >= 3
        assert all(i.get("min_margin", 1.0) >= mc.MARGIN for i in info.values()), name
