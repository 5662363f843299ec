"""
Host side of the classic MCTS for a batch (planning/device_rollout.py, csrc/k_rollout.h): the host restatement of the device rollout
reproduces the rollouts recorded from the reference (tests/golden/gen_rollout_golden.py: the reference's fp64 rewards and its draws as
uniforms), the pick's edge rules, and the binding and the header agree on the new entry points.  No GPU.
"""
import os
import re

import numpy as np
import pytest

from ipp_rl_amd import _ffi
from ipp_rl_amd.planning import device_rollout as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipp_tree_score_nodes", "ipp_tree_score_nodes_scratch_bytes", "ipp_rollout_candidates", "ipp_rollout_pick", "ipp_rollout_advance",
       "ipp_rollout_run")
UAV = {"max_v": 2, "max_a": 2}


def host_kwargs(g, gcb):
    amin, amax, aspc = (float(x) for x in g["alts"])
    return dict(x_dim=int(g["dim"]), y_dim=int(g["dim"]), resolution=float(g["resolution"]), min_altitude=amin, max_altitude=amax,
                altitude_spacing=aspc, radius=float(g["radius"]), gamma=float(g["gamma"]), epsilon=float(g["epsilon_rollout"]), gcb=gcb,
                uav={"max_v": float(g["max_v"]), "max_a": float(g["max_a"])})


def fixture_score_fn(g, i, seen):
    """score_fn of rollout i from the fixture: the reference's fp64 reward of every action it found available at the level (looked up
    by waypoint), 0 elsewhere; `seen` collects per level the device-order candidates that got a reward."""
    def score(st, cands):
        lv = len(st["actions"])
        avail, rw, count = g["avail"][i, lv], g["reward"][i, lv], int(g["count"][i, lv])
        out = np.zeros(len(cands))
        hit = np.zeros(len(cands), dtype=bool)
        for a, r in zip(avail[:count], rw[:count]):
            j = np.flatnonzero((cands == a).all(axis=1))
            assert len(j) == 1, "an action the reference found available is not among the device's candidates"
            out[j[0]], hit[j[0]] = r, True
        seen.append(hit)
        return out, None
    return score


def test_rollout_host_reproduces_the_recorded_reference_rollouts(golden):
    g = golden("rollout")
    n = len(g["case"])
    per_mode = [int((g["case"] == c).sum()) for c in (0, 1)]
    assert min(per_mode) >= 8 and int(g["kmax"]) == 98
    for c in (0, 1):
        deep = (g["case"] == c) & (g["depth"] == 3) & (g["levels"] == 3)
        assert int(deep.sum()) >= 3
    assert np.any(g["levels"] < g["depth"])  # a rollout the budget ended early
    for i in range(n):
        gcb = bool(g["case"][i])
        kw = host_kwargs(g, gcb)
        cur = g["start_actions"][i, int(g["start_len"][i]) - 1] if int(g["start_len"][i]) else None
        if cur is None:
            cur = np.load(os.path.join(ROOT, "tests", "golden", "mcts_mission.npz"))[f"{str(g['case_names'][int(g['case'][i])])}_prev"]
        seen = []
        st = dr.rollout_host(fixture_score_fn(g, i, seen), cur, float(g["budget"][i]), int(g["depth"][i]), g["u"][i], max_depth=3, **kw)
        L = int(g["levels"][i])
        assert len(st["actions"]) == L, (i, len(st["actions"]), L)
        assert np.array_equal(np.array(st["actions"]).reshape(L, 3), g["chosen"][i, :L])
        assert np.array_equal(np.array(st["budgets"]), g["budget_after"][i, :L])  # exactly: waypoint differences are whole metres, so
        # the sum of squares is exact and both square roots round the same number; the flight-time formula then runs the same operations
        assert abs(st["value"] - float(g["value"][i])) < 1e-12
        # the availability mask of every level is the reference's (get_next_actions_mask), and an early end is the budget's
        for lv, hit in enumerate(seen[:L]):
            cands = dr.radius_candidates((g["chosen"][i, lv - 1] if lv else cur), kw["x_dim"], kw["y_dim"], kw["resolution"], kw["min_altitude"],
                                         kw["max_altitude"], kw["altitude_spacing"], kw["radius"])
            cost = np.array([dr.cost_host(a, (g["chosen"][i, lv - 1] if lv else cur), kw["uav"]) if np.isfinite(a).all() else np.nan for a in cands])
            before = float(g["budget"][i]) if lv == 0 else float(g["budget_after"][i, lv - 1])
            assert np.array_equal(dr.available_host(cands, cost, before), hit)
        if L < int(g["depth"][i]):
            assert st["flag"] == dr.END and st["budget"] < kw["resolution"]


def _pick(reward, cost, budget=100.0, depth_left=2, u0=0.9, u1=0.0, epsilon=0.5, gcb=False, status=None, cand=None):
    k = len(reward)
    cand = np.zeros((k, 3)) if cand is None else cand
    return dr.pick_host(cand, np.asarray(reward), np.asarray(cost, dtype=np.float64), status, budget, depth_left, u0, u1, resolution=4.0,
                        epsilon=epsilon, gcb=gcb)


def test_pick_host_edge_rules():
    r = np.array([0.1, 0.7, 0.7, 0.3], dtype=np.float32)
    c = [3.0, 3.0, 3.0, 3.0]
    assert _pick(r, c, u0=0.9) == (1, dr.RUNNING)                    # greedy: the FIRST maximiser
    assert _pick(r, c, u0=0.5, u1=0.0) == (0, dr.RUNNING)            # u0 == epsilon is NOT greedy (np.random.uniform(0, 1) > epsilon)
    assert _pick(r, c, u0=0.5, u1=1.0 - 2.0 ** -53) == (3, dr.RUNNING)
    assert _pick(r, c, u0=0.1, u1=0.5) == (2, dr.RUNNING)            # floor(0.5 x 4) = 2
    assert _pick(r, [3.0, 0.0, 200.0, np.nan], u0=0.9) == (0, dr.RUNNING)  # cost 0, cost > budget, NaN cost: not available
    # count 0 in both modes, whatever u0 says: NO_ACTION
    for gcb in (False, True):
        for u0 in (0.1, 0.9):
            assert _pick(r, [0.0, 0.0, 200.0, np.nan], u0=u0, gcb=gcb) == (-1, dr.NO_ACTION)
    # a NaN reward never wins; all NaN: an error
    assert _pick(np.array([np.nan, 0.2, np.nan, 0.1], dtype=np.float32), c, u0=0.9) == (1, dr.RUNNING)
    assert _pick(np.full(4, np.nan, dtype=np.float32), c, u0=0.9) == (-1, dr.ERR_NAN)
    assert _pick(np.full(4, np.nan, dtype=np.float32), c, u0=0.1, u1=0.3) == (1, dr.RUNNING)  # the random branch does not look at rewards
    # the ends come first and consume nothing
    assert _pick(r, c, depth_left=0) == (-1, dr.END)
    assert _pick(r, c, budget=3.999) == (-1, dr.END)
    # a rejected footprint on an available candidate is an error, on an unavailable one it is not
    st = np.array([0, 4, 0, 0])
    assert _pick(r, c, status=st) == (-1, dr.ERR_FOOTPRINT)
    assert _pick(r, [3.0, 0.0, 3.0, 3.0], status=st) == (2, dr.RUNNING)
    # a NaN candidate row is no candidate
    cand = np.zeros((4, 3))
    cand[1, 2] = np.nan
    assert _pick(r, c, cand=cand) == (2, dr.RUNNING)


def test_pick_host_cost_benefit_rule():
    c = [3.0] * 4
    eq = np.zeros(4, dtype=np.float32)  # equal rewards: four intervals of 1/4; side = "right": u1 on a boundary goes up
    assert _pick(eq, c, gcb=True, u1=0.0) == (0, dr.RUNNING)
    assert _pick(eq, c, gcb=True, u1=0.25) == (1, dr.RUNNING)
    assert _pick(eq, c, gcb=True, u1=0.7499) == (2, dr.RUNNING)
    assert _pick(eq, c, gcb=True, u1=1.0 - 2.0 ** -53) == (3, dr.RUNNING)
    r = np.log(np.array([1.0, 2.0, 5.0, 2.0])).astype(np.float32)  # p = 0.1, 0.2, 0.5, 0.2; the second is not available
    cc = [3.0, 0.0, 3.0, 3.0]                                       # p = 1/8, 5/8, 2/8 over the others
    assert _pick(r, cc, gcb=True, u1=0.12) == (0, dr.RUNNING)
    assert _pick(r, cc, gcb=True, u1=0.13) == (2, dr.RUNNING)
    assert _pick(r, cc, gcb=True, u1=0.76) == (3, dr.RUNNING)
    assert _pick(np.array([0.1, np.nan, 0.2, 0.3], dtype=np.float32), c, gcb=True, u1=0.5) == (-1, dr.ERR_NAN)
    # the same choice legacy NumPy makes with the same uniform: cdf.searchsorted(u, side="right")
    rs = np.random.RandomState(3)
    for _ in range(50):
        rr = rs.normal(size=7).astype(np.float32)
        u = rs.random_sample()
        p = np.exp(rr.astype(np.float64)) / np.sum(np.exp(rr.astype(np.float64)))
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        if np.min(np.abs(cdf - u)) < 1e-9:
            continue
        assert _pick(rr, [3.0] * 7, gcb=True, u1=u)[0] == int(cdf.searchsorted(u, side="right"))


def test_advance_host_charges_the_grandparent():
    st = dr.new_state(0, [5], [10.0, 10.0, 8.0], 30.0, 3)
    a1, a2 = np.array([14.0, 10.0, 8.0]), np.array([14.0, 18.0, 14.0])
    dr.advance_host(st, a1, 100, np.float32(0.5), 0, gamma=0.9, uav=UAV)
    assert st["budget"] == 30.0 - dr.cost_host(a1, [10.0, 10.0, 8.0], UAV)  # level 0: charged from the node's own waypoint
    assert st["path"][:2] == [5, 100] and st["plen"] == 2 and st["depth_left"] == 2 and st["value"] == 0.5 and st["disc"] == 0.9
    b1 = st["budget"]
    dr.advance_host(st, a2, 101, np.float32(0.25), 0, gamma=0.9, uav=UAV)
    assert st["budget"] == b1 - dr.cost_host(a2, [10.0, 10.0, 8.0], UAV)    # level 1: from the GRANDPARENT, not from a1
    assert st["budget"] != b1 - dr.cost_host(a2, a1, UAV)
    assert st["value"] == 0.5 + 0.9 * 0.25 and np.array_equal(st["cur"], a2) and np.array_equal(st["charge_from"], a1)
    dr.advance_host(st, a1, 102, np.float32(1.0), _ffi.STATUS_RANK_FULL, gamma=0.9, uav=UAV)  # the reward counts, then the rollout ends
    assert st["flag"] == dr.RANK_FULL and not st["live"] and st["value"] == 0.5 + 0.9 * 0.25 + (0.9 * 0.9) * 1.0 and st["plen"] == 3
    st2 = dr.new_state(0, [], [10.0, 10.0, 8.0], 30.0, 3)
    dr.advance_host(st2, a1, 7, np.float32(1.0), _ffi.STATUS_NOT_PD, gamma=0.9, uav=UAV)
    assert st2["flag"] == dr.ERR_STEP and st2["value"] == 0.0


def test_cost_host_is_action_costs():
    from ipp_rl_amd.planning.common.actions import action_costs

    rs = np.random.RandomState(0)
    for _ in range(100):
        a, p = rs.uniform(0, 40, 3), rs.uniform(0, 40, 3)
        for uav in (None, UAV):
            assert abs(dr.cost_host(a, p, uav) - action_costs(a, p, uav)) < 1e-12


def test_prototypes_match_header():
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
    # ipp_rollout: same fields in the same order; int32 / uint32 / double scalars, everything else a device pointer
    body = re.search(r"typedef struct ipp_rollout \{(.*?)\} ipp_rollout;", text, flags=re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        kind = "p" if "*" in stmt else ("d" if stmt.startswith("double") else "i")
        names = re.sub(r"^(const\s+)?(int32_t|uint32_t|double|float)\s*\*?", "", stmt)
        fields += [(nm.strip().lstrip("*").strip(), kind) for nm in names.split(",")]
    import ctypes as C

    want = [(nm, "p" if t is C.c_void_p else "d" if t is C.c_double else "i") for nm, t in _ffi.IppRollout._fields_]
    assert fields == want
    for macro, val in (("IPP_ROLLOUT_RUNNING", 0), ("IPP_ROLLOUT_END", 1), ("IPP_ROLLOUT_NO_ACTION", 2), ("IPP_ROLLOUT_RANK_FULL", 3),
                       ("IPP_ROLLOUT_ERR_FOOTPRINT", 4), ("IPP_ROLLOUT_ERR_NAN", 5), ("IPP_ROLLOUT_ERR_STEP", 6)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", raw) and getattr(_ffi, macro) == val


def test_classic_mcts_has_the_batched_switch_and_the_policy_is_exported():
    import inspect

    from ipp_rl_amd.planning import VecMctsPolicy
    from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

    assert inspect.signature(ClassicMCTS.__init__).parameters["batched"].default is False
    assert {"act", "run"} <= set(dir(VecMctsPolicy))
