"""
Hand-built tables for the device tree search's kernels (csrc/k_ctree.h) and their host restatements (planning/device_ctree.py), shared
by tests/test_ctree_host.py (the restatements against the outcomes written down here) and tests/test_hip_ctree_kernels.py (the kernels
against the restatements).

Geometry of every case but the widening one: a 10x10 grid of 4 m cells, altitudes 10 / 12, greedy radius 4 m -- half = 1, kmax = 18 --
and flight-time costs (max_v = max_a = 2).  From a cell centre exactly one action is available, the other altitude (2 m, cost 2);
the hand-built children sit wherever a case needs them.  Tables hold cap = 9 slots, the horizon is 3.
"""
import numpy as np

UAV = {"max_v": 2.0, "max_a": 2.0}
CAP, HORIZON, C_UCT = 9, 3, 2.0
CENTRE = (22.0, 18.0, 10.0)
GEO = dict(x_dim=10, y_dim=10, resolution=4.0, min_altitude=10.0, max_altitude=12.0, altitude_spacing=2.0, radius=4.0, uav=UAV)
WIDE = dict(GEO, radius=12.0)   # half = 3, kmax = 98: more than 33 actions available from the centre of the grid


def params(thr=None, geo=GEO, horizon=HORIZON):
    from ipp_rl_amd.planning.device_ctree import widening_table

    return dict(geo, c=C_UCT, horizon=horizon, thr=widening_table(4.0, 0.75, 20) if thr is None else np.asarray(thr, dtype=np.float64))


NEVER_WIDEN = np.zeros(43)      # thr = 0: a node with a child never widens


def table(waypoint, nodes=(), root_visits=0, root_value=0.0, cap=CAP, horizon=HORIZON):
    """Tables of one root: slot 0 (waypoint, root_visits, root_value) and nodes = [(parent slot, action, visits, value_sum, edge_reward)]
    in slot order; node s gets the engine id 100 + s."""
    from ipp_rl_amd.planning.device_ctree import new_table

    T = new_table(cap, horizon, waypoint)
    T["visits"][0], T["value_sum"][0] = root_visits, root_value
    for s, (parent, action, visits, value_sum, edge) in enumerate(nodes, start=1):
        pl = int(T["plen"][parent])
        T["parent"][s], T["dev"][s], T["plen"][s] = parent, 100 + s, pl + 1
        T["path"][s, :pl] = T["path"][parent, :pl]
        T["path"][s, pl] = 100 + s
        T["action"][s] = action
        T["visits"][s], T["value_sum"][s], T["edge_reward"][s] = visits, value_sum, edge
    T["count"] = 1 + len(nodes)
    return T


EAST, WEST, NORTH, FAR = (26.0, 18.0, 10.0), (18.0, 18.0, 10.0), (22.0, 22.0, 10.0), (38.0, 38.0, 12.0)   # costs 3, 3, 3 and > 10 from CENTRE
UP = (22.0, 18.0, 12.0)


def descend_cases():
    """name -> dict(T, wp, budget, tie [3], P, kind, trace): what k_ctree_descend must leave (kind, trace: None = err is set)."""
    from ipp_rl_amd.planning import device_ctree as dc

    cs = {}

    def add(name, T, kind, trace, budget=30.0, tie=(0.3, 0.3, 0.3), P=None, wp=CENTRE):
        cs[name] = dict(T=T, wp=np.array(wp), budget=budget, tie=np.array(tie), P=P or params(NEVER_WIDEN), kind=kind, trace=trace)

    # the three branches of Node.uct; a child that wins is unvisited below, so the descent rolls it out
    add("uct_max_is_zero", table(CENTRE, [(0, EAST, 2, 0.0, 0.1), (0, WEST, 2, -1.0, 0.2)], 4), dc.TERMINAL, [0, 1], budget=5.0)
    add("uct_max_equals_min", table(CENTRE, [(0, EAST, 2, 1.4, 0.1), (0, WEST, 1, 0.7, 0.2)], 4), dc.TERMINAL, [0, 2], budget=5.0)
    # values 1.0 (3 visits) and 0.5 (1 visit): `value - min / (max - min)` prefers the second, (value - min) / (max - min) the first
    add("uct_precedence_quirk", table(CENTRE, [(0, EAST, 3, 3.0, 0.1), (0, WEST, 1, 0.5, 0.2)], 4), dc.TERMINAL, [0, 2], budget=5.0)
    add("unvisited_child_is_infinite", table(CENTRE, [(0, EAST, 5, 50.0, 0.1), (0, WEST, 0, 0.0, 0.2)], 4), dc.ROLLOUT, [0, 2])
    # the better child costs more than the budget
    add("barred_by_cost", table(CENTRE, [(0, FAR, 1, 9.0, 0.1), (0, WEST, 3, 0.3, 0.2)], 4), dc.TERMINAL, [0, 2], budget=6.0)
    # every child barred: all tie at -inf, the tie uniform picks the second of three; the budget goes negative, terminal below
    add("all_barred_tie", table(CENTRE, [(0, FAR, 1, 1.0, 0.1), (0, FAR, 2, 9.0, 0.2), (0, CENTRE, 3, 2.0, 0.3)], 4), dc.TERMINAL, [0, 2],
        budget=6.0, tie=(0.5, 0.3, 0.3))
    twins = [(0, EAST, 2, 1.0, 0.1), (0, EAST, 2, 1.0, 0.1)]
    add("exact_tie_low", table(CENTRE, twins, 4), dc.TERMINAL, [0, 1], budget=5.0, tie=(0.49999, 0.3, 0.3))
    add("exact_tie_high", table(CENTRE, twins, 4), dc.TERMINAL, [0, 2], budget=5.0, tie=(0.5, 0.3, 0.3))
    add("largest_uniform", table(CENTRE, twins, 4), dc.TERMINAL, [0, 2], budget=5.0, tie=(1.0 - 2.0 ** -53, 0.3, 0.3))
    add("terminal_root", table(CENTRE, twins, 4), dc.TERMINAL, [0], budget=3.999)
    add("unvisited_root", table(CENTRE), dc.ROLLOUT, [0])
    add("first_expansion", table(CENTRE, [], 1, 0.4), dc.EXPAND, [0], P=params())
    # one child, one available action: no widening (children < available fails); the chain ends when the depth is used up
    chain = [(0, UP, 2, 1.0, 0.1), (1, CENTRE, 2, 1.0, 0.2), (2, UP, 2, 1.0, 0.3)]
    add("depth_used_up", table(CENTRE, chain, 3, 2.0), dc.TERMINAL, [0, 1, 2, 3], P=params())
    add("widen_below_the_root", table(CENTRE, chain[:1] + [(1, CENTRE, 2, 1.0, 0.2), (1, CENTRE, 2, 5.0, 0.2)], 3, 2.0), dc.EXPAND, [0, 1, 3],
        P=params(NEVER_WIDEN))   # (slot 3 wins below slot 1 and has no child: the first expansion of a node ignores thr)
    # budget 2.0 at the child: 2 < resolution
    add("budget_ends_below", table(CENTRE, chain, 3, 2.0), dc.TERMINAL, [0, 1], budget=4.0, P=params())
    bad = table(CENTRE, twins, 4)
    bad["count"] = CAP + 1
    add("count_out_of_range", bad, None, None)
    bad = table(CENTRE, twins, 4)
    bad["visits"][0] = 43
    add("visits_past_the_table", bad, None, None)
    stopped = table(CENTRE, twins, 4)
    stopped["err"] = dc.ERR_STEP
    add("err_root_untouched", stopped, None, None)
    return cs


def widening_cases():
    """thr[16] = 4 x 16^0.75 = 32 exactly: 32 children widen (32 <= 32 and 32 < available), 33 do not.  cap = 40, radius 12 m."""
    from ipp_rl_amd.planning import device_ctree as dc

    P = params(geo=WIDE)
    assert P["thr"][16] == 32.0
    cs = {}
    assert dc.n_available_host(np.array(CENTRE), 30.0, P) > 33
    for n, trace in ((32, [0]), (33, [0, 1])):   # (33: the best child, slot 1, is selected and expands in its turn)
        kids = [(0, EAST, 1, 1.0 - 0.01 * j, 0.1) for j in range(n)]
        cs[f"widen_{n}_children"] = dict(T=table(CENTRE, kids, 16, 3.0, cap=40), wp=np.array(CENTRE), budget=30.0, tie=np.array([0.3] * 3), P=P,
                                         kind=dc.EXPAND, trace=trace)
    return cs


def attach_cases():
    """name -> dict(T (after a descent that ended in EXPAND), ex = (live, flag, action, new_id, step_reward, step_status), P, kind, err)."""
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc
    from ipp_rl_amd.planning import device_rollout as dr

    cs = {}

    def add(name, T, ex, kind, err=0, budget=30.0, depth=HORIZON, trace=(0,)):
        T["t_len"], T["leaf_kind"], T["leaf_budget"], T["leaf_depth"] = len(trace), dc.EXPAND, budget, depth
        T["t_slot"][: len(trace)] = trace
        cs[name] = dict(T=T, ex=ex, P=params(), kind=kind, err=err)

    ok = (1, dr.RUNNING, np.array(UP), 555, np.float32(0.3125), _ffi.STATUS_OK)
    add("child_rolls_out", table(CENTRE, [], 1, 0.4), ok, dc.ROLLOUT)
    chain = [(0, UP, 2, 1.0, 0.1), (1, CENTRE, 2, 1.0, 0.2)]
    add("child_at_depth_two", table(CENTRE, chain, 3, 2.0), ok, dc.ROLLOUT, budget=20.0, depth=2, trace=(0, 1))
    add("terminal_child_by_depth", table(CENTRE, chain, 3, 2.0), ok, dc.TERMINAL, budget=20.0, depth=1, trace=(0, 1, 2))
    add("terminal_child_by_budget", table(CENTRE, [], 1, 0.4), ok, dc.TERMINAL, budget=5.0)   # 5 - 2 < 4
    add("no_action", table(CENTRE, [], 1, 0.4), (0, dr.NO_ACTION, np.full(3, np.nan), -1, np.float32(0), _ffi.STATUS_BAD_FOOTPRINT), dc.TERMINAL)
    add("pick_error", table(CENTRE, [], 1, 0.4), (0, dr.ERR_NAN, np.full(3, np.nan), -1, np.float32(0), _ffi.STATUS_BAD_FOOTPRINT), dc.EXPAND,
        err=dc.ERR_PICK | (dr.ERR_NAN << 8))
    add("rank_full", table(CENTRE, [], 1, 0.4), ok[:5] + (_ffi.STATUS_RANK_FULL,), dc.EXPAND, err=dc.ERR_STEP | (_ffi.STATUS_RANK_FULL << 8))
    full = table(CENTRE, [(0, EAST, 1, 1.0, 0.1)] * (CAP - 1), 9, 1.0)
    add("table_full", full, ok, dc.EXPAND, err=dc.ERR_FULL)
    bad = table(CENTRE, [], 1, 0.4)
    add("trace_out_of_range", bad, ok, dc.EXPAND, err=dc.ERR_RANGE, trace=(0, 5))
    return cs


def backup_cases():
    """name -> dict(T (trace and leaf kind set), value, flag, P, visits, value_sum): the counters and sums k_ctree_backup must leave."""
    from ipp_rl_amd.planning import device_ctree as dc
    from ipp_rl_amd.planning import device_rollout as dr

    cs = {}
    chain = [(0, UP, 2, 1.0, 0.125), (1, CENTRE, 0, 0.0, 0.25), (0, EAST, 1, 7.0, 0.5)]

    def add(name, kind, trace, value, flag, visits, value_sum, err=0):
        T = table(CENTRE, chain, 3, 2.0)
        T["t_len"], T["leaf_kind"] = len(trace), kind
        T["t_slot"][: len(trace)] = trace
        cs[name] = dict(T=T, value=value, flag=flag, P=params(), visits=visits, value_sum=value_sum, err=err)

    # root -> 1 -> 2, slot 2 rolled out (value 0.75): slot 2 counts twice (leaf, then as the child), slot 1 twice, the root once
    add("double_increment", dc.ROLLOUT, (0, 1, 2), 0.75, dr.END, [4, 4, 2, 1], [2.0 + (0.125 + (0.25 + 0.75)), 1.0 + (0.25 + 0.75), 0.75, 7.0])
    # the terminal child: not visited by itself, counted once as the child
    add("terminal_child_counted_once", dc.TERMINAL, (0, 1, 2), 123.0, dr.RUNNING, [4, 4, 1, 1], [2.0 + (0.125 + 0.25), 1.0 + 0.25, 0.0, 7.0])
    add("terminal_root", dc.TERMINAL, (0,), 123.0, dr.RUNNING, [3, 2, 0, 1], [2.0, 1.0, 0.0, 7.0])
    add("rollout_no_action_keeps_its_value", dc.ROLLOUT, (0, 3), 0.5, dr.NO_ACTION, [4, 2, 0, 3], [2.0 + (0.5 + 0.5), 1.0, 0.0, 7.5])
    add("rollout_error_flag", dc.ROLLOUT, (0, 3), 0.5, dr.ERR_STEP, [3, 2, 0, 1], [2.0, 1.0, 0.0, 7.0], err=dc.ERR_ROLLOUT | (dr.ERR_STEP << 8))
    add("still_expanding", dc.EXPAND, (0, 3), 0.5, dr.RUNNING, [3, 2, 0, 1], [2.0, 1.0, 0.0, 7.0], err=dc.ERR_RANGE)
    return cs


def best_cases():
    """name -> dict(T, wp, action, has)."""
    from ipp_rl_amd.planning import device_ctree as dc

    cs = {}
    kids = [(0, EAST, 2, 1.0, 0.1), (0, WEST, 4, 3.0, 0.1), (1, UP, 1, 99.0, 0.1), (0, NORTH, 8, 6.0, 0.1), (0, UP, 3, 1.5, 0.1)]
    cs["first_of_equals"] = dict(T=table(CENTRE, kids, 9, 1.0), wp=np.array(CENTRE), action=np.array(WEST), has=1)   # 0.5, 0.75, (grandchild), 0.75, 0.5
    cs["no_child"] = dict(T=table(CENTRE, [], 1, 1.0), wp=np.array(CENTRE), action=np.array(CENTRE), has=0)
    stopped = table(CENTRE, kids, 9, 1.0)
    stopped["err"] = dc.ERR_FULL
    cs["err_root"] = dict(T=stopped, wp=np.array(CENTRE), action=np.array(CENTRE), has=0)
    cs["negative_values"] = dict(T=table(CENTRE, [(0, EAST, 2, -4.0, 0.1), (0, WEST, 2, -1.0, 0.1)], 4, 1.0), wp=np.array(CENTRE),
                                 action=np.array(WEST), has=1)
    return cs
