"""
Host side of the device tree search (planning/device_ctree.py, csrc/k_ctree.h).  No GPU.

1. search_host, the restatement of ipp_ctree_search, against the project's own host tree: ClassicMCTS._search generators
   (planning/mcts_mission.py) and search_host are driven from the same stub answers -- rewards that are distinct fp32 values of (path,
   action), rollout values of (path, how many rollouts the root has had), epsilon_expand = 0 so that every expansion is greedy and the
   candidate order cannot matter, the tie uniforms replayed to the host tree's random.choice as floor(u n).  Every root must end with
   the same tree as tests/test_hip_rollout.py::same_tree means it: actions, visits, number of children, float(value_sum) bit for bit.
2. The four restatements on hand-built tables (tests/ctree_cases.py) against the outcomes written down with the cases.
3. The binding against the header.
"""
import ctypes as C
import math
import os
import re
import types
import zlib

import numpy as np
import pytest

from ipp_rl_amd import _ffi
from ipp_rl_amd.planning import device_ctree as dc
from ipp_rl_amd.planning import device_rollout as dr
from tests import ctree_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipp_ctree_descend", "ipp_ctree_attach", "ipp_ctree_backup", "ipp_ctree_best", "ipp_ctree_search")
UAV = {"max_v": 2.0, "max_a": 2.0}


# ----------------------------------------------------------------------------------------------- 1. against ClassicMCTS._search
def same_tree(a, b):
    assert np.array_equal(a.action, b.action) and a.visits == b.visits and len(a.children) == len(b.children)
    assert float(a.value_sum) == float(b.value_sum)
    for x, y in zip(a.children, b.children):
        same_tree(x, y)


def unit(*key):
    """A number in [0, 1) from the bytes of the key."""
    return zlib.crc32(np.asarray(key, dtype=np.float64).tobytes()) / 2.0 ** 32


def stub_reward(root, chain, action):
    return np.float32(0.05 + unit(root, *[x for a in chain for x in a], *action))


def stub_value(root, chain, nth):
    """Children of a node are duplicates here (greedy expansion): every other rollout of a root repeats the value of its path, so that
    exact UCT ties occur and the tie uniforms decide."""
    return 0.25 * (1 + len(chain)) * unit(7.0, root, *[x for a in chain for x in a], float(nth % 2))


class TieReplay:
    """random.Random stand-in: choice(children) of simulation s at level l = child number floor(u[s, l] n)."""

    def __init__(self, tie):
        self.tie, self.sizes = tie, []

    def choice(self, seq):
        node = seq[0].parent
        level = len(node.path)
        while node.parent is not None:
            node = node.parent
        self.sizes.append(len(seq))
        return seq[min(int(math.floor(self.tie[node.visits, level] * len(seq))), len(seq) - 1)]


def chain_of(node):
    out = []
    while node.parent is not None:
        out.append(tuple(float(x) for x in node.action))
        node = node.parent
    return tuple(reversed(out))


def host_tree(mcts, root, wp, budget, tie, n_sims):
    """ClassicMCTS._search of one root, its requests answered by the stubs."""
    from ipp_rl_amd.planning.mcts_mission import Node

    s = mcts.new_search(root, np.array(wp), budget, 0, 0)
    s.py_rng = TieReplay(tie)
    gen, nodes, rollouts = mcts._search(s, n_sims), 0, 0
    try:
        req = next(gen)
        while True:
            node = req[1]
            if req[0] == "score":
                ans = np.array([stub_reward(root, chain_of(node), a) for a in req[2]], dtype=np.float64)
            elif req[0] == "step":
                nodes += 1
                ans = Node(root, nodes, node.path + [nodes], parent=node, action=req[2], edge_reward=float(stub_reward(root, chain_of(node), req[2])))
            else:
                assert req[0] == "rollout"
                ans = stub_value(root, chain_of(node), rollouts)
                rollouts += 1
            req = gen.send(ans)
    except StopIteration:
        pass
    return s.root, s.py_rng.sizes


def restated_tree(kw, root, wp, budget, u, index, roots):
    chains, counter = {}, [0]

    def chain(st):
        return chains[st["path"][st["plen"] - 1]] if st["plen"] else ()

    def score_fn(st, cands):
        return np.array([stub_reward(root, chain(st), a) if np.isfinite(a).all() else 0.0 for a in cands], dtype=np.float32), None

    def step_fn(st, action, new_id):
        chains[new_id] = chain(st) + (tuple(float(x) for x in action),)
        return stub_reward(root, chain(st), action), _ffi.STATUS_OK

    def rollout_fn(st, uu):
        counter[0] += 1
        return stub_value(root, chain(st), counter[0] - 1), dr.END

    T = dc.search_host(score_fn, step_fn, rollout_fn, root, wp, budget, u, node_base=40, index=index, roots=roots, **kw)
    assert T["err"] == 0
    return dc.table_to_nodes(T, root), T


@pytest.mark.parametrize("radius, alts", [(4.0, (10.0, 12.0, 2.0)), (6.0, (8.0, 14.0, 6.0))])
def test_search_host_builds_the_trees_of_the_host_search(radius, alts):
    """3 roots, 12 simulations, horizon 3, two altitude levels; radius 4 m is half = 1 (from a cell centre only the other altitude is in
    reach: off-centre roots, narrow trees), radius 6 m (half = 2) adds the four neighbours."""
    from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

    R, sims, horizon = 3, 12, 3
    cfg = types.SimpleNamespace(x_dim=10, y_dim=10, resolution=4.0, n_cells=100)
    engine = types.SimpleNamespace(TREE_DEPTH=6, _c=types.SimpleNamespace(node_capacity=4096), set_uav=lambda *a: None)
    mcts = ClassicMCTS(engine, cfg, UAV, *alts, num_simulations=sims, episode_horizon=horizon, k=4.0, alpha=0.75, epsilon_expand=0.0,
                       max_greedy_radius=radius, batched=True)
    kw = dict(n_sims=sims, horizon=horizon, c=2.0, thr=dc.widening_table(4.0, 0.75, sims), epsilon_expand=0.0, x_dim=10, y_dim=10, resolution=4.0,
              min_altitude=alts[0], max_altitude=alts[1], altitude_spacing=alts[2], radius=radius, uav=UAV)
    assert int(np.ceil(radius / 4.0)) == (1 if radius == 4.0 else 2) and len(dc.altitude_levels(*alts)) == 2
    u = dc.uniform_tables(np.random.RandomState(12), sims, R, horizon)
    u["expand"][..., 0] = 0.5   # (> epsilon_expand = 0: greedy, as the host's np_rng.uniform(0, 1) > 0)
    wps = [(21.0, 17.5, 11.0), (2.0, 2.0, alts[0]), (30.5, 9.0, alts[1])]
    budgets = [60.0, 9.0, 14.0]
    tie_sizes, depths = [], []
    for i in range(R):
        mine, T = restated_tree(kw, i, np.array(wps[i]), budgets[i], {k: v[:, i] for k, v in u.items()}, i, R)
        theirs, sizes = host_tree(mcts, i, wps[i], budgets[i], u["tie"][:, i], sims)
        same_tree(theirs, mine)
        assert mine.visits == sims and int(T["count"]) >= 3
        tie_sizes += sizes
        depths.append(int(T["plen"][: T["count"]].max()))
        # ids: the node of simulation s is 40 + s R + i; every node's path ends with its own id
        for s in range(1, int(T["count"])):
            assert (int(T["dev"][s]) - 40 - i) % R == 0 and int(T["path"][s, T["plen"][s] - 1]) == int(T["dev"][s])
    assert max(tie_sizes) >= 2, "no UCT tie in any search: the tie uniforms were not exercised"
    assert max(depths) >= 2


# ----------------------------------------------------------------------------------------------- 2. hand-built tables
ALL_DESCEND = {**cases.descend_cases(), **cases.widening_cases()}


@pytest.mark.parametrize("name", sorted(ALL_DESCEND))
def test_descend_host_on_hand_built_tables(name):
    cs = ALL_DESCEND[name]
    T = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in cs["T"].items()}
    before = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in T.items()}
    kind, row = dc.descend_host(T, 5, cs["wp"], cs["budget"], cs["tie"], cs["P"])
    if cs["kind"] is None:
        assert T["err"] != 0 and row is None
        if name == "err_root_untouched":
            for k, v in before.items():
                assert np.array_equal(T[k], v), k
        else:
            assert T["err"] == dc.ERR_RANGE
        return
    assert T["err"] == 0 and kind == cs["kind"] == T["leaf_kind"]
    assert [int(x) for x in T["t_slot"][: T["t_len"]]] == cs["trace"]
    leaf = cs["trace"][-1]
    assert T["leaf_depth"] == cases.HORIZON - (len(cs["trace"]) - 1)
    want_budget = cs["budget"]
    for a, b in zip(cs["trace"], cs["trace"][1:]):
        want_budget = want_budget - dr.cost_host(T["action"][b], T["action"][a], cases.UAV)
    assert T["leaf_budget"] == want_budget
    if kind == dc.TERMINAL:
        assert row is None
    else:
        assert row["root"] == 5 and row["plen"] == int(T["plen"][leaf]) and row["path"] == [int(x) for x in T["path"][leaf]]
        assert np.array_equal(row["cur"], T["action"][leaf]) and np.array_equal(row["charge_from"], T["action"][leaf])
        assert row["budget"] == want_budget and row["depth_left"] == (T["leaf_depth"] if kind == dc.ROLLOUT else 1)
        assert row["value"] == 0.0 and row["disc"] == 1.0 and row["live"] == 1 and row["flag"] == dr.RUNNING
    for k in dc.NODE_FIELDS + ("count",):   # a descent changes nothing in the tree
        assert np.array_equal(T[k], before[k]), k


def test_widening_threshold_is_exact_at_sixteen_visits():
    from ipp_rl_amd.planning.rollout import RolloutPolicy

    thr = dc.widening_table(4.0, 0.75, 100)
    assert len(thr) == 203 and thr[16] == 32.0 and thr[0] == 0.0 and thr[1] == 4.0
    for v in range(len(thr)):
        for n in (max(int(thr[v]), 1), int(thr[v]) + 1):
            assert (n <= thr[v]) == RolloutPolicy.widen(n, v, 4.0, 0.75, 10 ** 6)


@pytest.mark.parametrize("name", sorted(cases.attach_cases()))
def test_attach_host_on_hand_built_tables(name):
    cs = cases.attach_cases()[name]
    T = cs["T"]
    before = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in T.items()}
    live, flag, action, new_id, reward, status = cs["ex"]
    row = dc.attach_host(T, 5, live, flag, action, new_id, reward, status, cs["P"])
    assert T["err"] == cs["err"] and T["leaf_kind"] == cs["kind"]
    made = cs["err"] == 0 and live
    assert T["count"] == before["count"] + (1 if made else 0) and T["t_len"] == before["t_len"] + (1 if made else 0)
    if not made:
        assert row is None
        for k in dc.NODE_FIELDS:
            assert np.array_equal(T[k], before[k]), k
        return
    c, node = before["count"], int(before["t_slot"][before["t_len"] - 1])
    pl = int(T["plen"][node])
    assert T["parent"][c] == node and T["dev"][c] == new_id and T["plen"][c] == pl + 1 and T["t_slot"][T["t_len"] - 1] == c
    assert T["path"][c].tolist() == T["path"][node][:pl].tolist() + [new_id] + [-1] * (5 - pl)
    assert np.array_equal(T["action"][c], action) and T["visits"][c] == 0 and T["value_sum"][c] == 0.0 and T["edge_reward"][c] == float(reward)
    budget = before["leaf_budget"] - dr.cost_host(action, T["action"][node], cases.UAV)
    assert T["leaf_budget"] == budget and T["leaf_depth"] == before["leaf_depth"] - 1
    if cs["kind"] == dc.ROLLOUT:
        assert row["budget"] == budget and row["depth_left"] == T["leaf_depth"] and row["path"] == T["path"][c].tolist() and row["live"] == 1
        assert np.array_equal(row["cur"], action) and np.array_equal(row["charge_from"], action)
    else:
        assert row is None and (T["leaf_depth"] == 0 or budget < 4.0)


@pytest.mark.parametrize("name", sorted(cases.backup_cases()))
def test_backup_host_on_hand_built_tables(name):
    cs = cases.backup_cases()[name]
    T = cs["T"]
    dc.backup_host(T, cs["value"], cs["flag"], cs["P"])
    assert T["err"] == cs["err"]
    assert T["visits"][:4].tolist() == cs["visits"]
    assert [float(x) for x in T["value_sum"][:4]] == [float(x) for x in cs["value_sum"]]   # bit for bit: the sums in simulate's order


@pytest.mark.parametrize("name", sorted(cases.best_cases()))
def test_best_host_on_hand_built_tables(name):
    cs = cases.best_cases()[name]
    action, has = dc.best_host(cs["T"], cs["wp"])
    assert has == cs["has"] and np.array_equal(action, cs["action"])
    if has:   # what the project's select_best_child says of the same tree
        from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

        assert np.array_equal(ClassicMCTS.select_best_child(dc.table_to_nodes(cs["T"], 0)).action, action)


def test_a_whole_search_with_an_unreachable_expansion_goes_on():
    """NO_ACTION on an expansion: from a cell centre at radius 4 m with ONE altitude level nothing is in reach.  The root is rolled out
    once; every later simulation wants to expand it, finds nothing and counts as terminal: no child, no visit, no error."""
    kw = dict(n_sims=4, horizon=3, c=2.0, thr=dc.widening_table(4.0, 0.75, 4), epsilon_expand=0.0, x_dim=10, y_dim=10, resolution=4.0,
              min_altitude=10.0, max_altitude=10.0, altitude_spacing=2.0, radius=4.0, uav=UAV)
    u = {k: v[:, 0] for k, v in dc.uniform_tables(np.random.RandomState(1), 4, 1, 3).items()}
    calls = []
    T = dc.search_host(lambda st, c: (np.zeros(len(c), dtype=np.float32), None), lambda st, a, i: calls.append(i), lambda st, uu: (0.5, dr.NO_ACTION),
                       0, np.array(cases.CENTRE), 30.0, u, **kw)
    assert T["err"] == 0 and T["count"] == 1 and T["visits"][0] == 1 and T["value_sum"][0] == 0.5 and not calls
    assert dc.best_host(T, cases.CENTRE)[1] == 0


# ----------------------------------------------------------------------------------------------- 3. the binding
def test_prototypes_and_struct_match_the_header():
    assert _ffi.ABI_VERSION == 17
    raw = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    assert "#define IPP_ABI_VERSION 17" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert name in _ffi.PROTOTYPES
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_args == len(_ffi.PROTOTYPES[name][1]), (name, n_args)
    assert len(_ffi.PROTOTYPES["ipp_ctree_search"][1]) == 9
    # ipp_ctree: same fields in the same order; int32 / double scalars first, then device pointers
    body = re.search(r"typedef struct ipp_ctree \{(.*?)\} ipp_ctree;", text, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        kind = "p" if "*" in stmt else ("d" if stmt.startswith("double") else "i")
        names = re.sub(r"^(const\s+)?(int32_t|uint32_t|double|float)\s*\*?", "", stmt)
        fields += [(nm.strip().lstrip("*").strip(), kind) for nm in names.split(",")]
    want = [(nm, "p" if t is C.c_void_p else "d" if t is C.c_double else "i") for nm, t in _ffi.IppCtree._fields_]
    assert fields == want
    kinds = [k for _, k in fields]
    assert "p" not in kinds[: kinds.index("p")] and set(kinds[kinds.index("p"):]) == {"p"}
    assert C.sizeof(_ffi.IppCtree) == 6 * 4 + 8 + 20 * 8
    for macro in ("IPP_CTREE_TERMINAL", "IPP_CTREE_ROLLOUT", "IPP_CTREE_EXPAND", "IPP_CTREE_ERR_RANGE", "IPP_CTREE_ERR_SELECT", "IPP_CTREE_ERR_PICK",
                  "IPP_CTREE_ERR_STEP", "IPP_CTREE_ERR_FULL", "IPP_CTREE_ERR_ROLLOUT"):
        assert re.search(rf"#define\s+{macro}\s+{getattr(_ffi, macro)}\b", raw), macro
    # the existing structs keep their layouts
    assert C.sizeof(_ffi.IppRollout) == 12 * 4 + 6 * 8 + 22 * 8


def test_the_policy_has_the_tree_switch_and_the_planner_is_exported():
    import inspect

    from ipp_rl_amd.planning import DeviceClassicMCTS, VecMctsPolicy
    from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

    assert inspect.signature(VecMctsPolicy.__init__).parameters["tree"].default == "host"
    mine, theirs = inspect.signature(DeviceClassicMCTS.__init__).parameters, inspect.signature(ClassicMCTS.__init__).parameters
    assert list(mine)[: len(theirs)] == list(theirs)
    assert {"search", "check", "to_host"} <= set(dir(DeviceClassicMCTS))
