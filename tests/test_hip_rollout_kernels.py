"""
GPU tests of the rollout policy kernels on bare buffers, no engine (csrc/k_rollout.h: ipp_rollout_pick, ipp_rollout_advance;
ipp_rollout_candidates beside them) against the host restatements of planning/device_rollout.py.  Indices, flags and node ids must
match exactly.  The fp64 outputs (value, discount, budget, waypoints) must be BIT-equal: the kernels are compiled without fused
multiply-adds and every operation they use there -- +, -, x, /, sqrt, min -- is correctly rounded in IEEE-754 binary64 on the device
as in CPython, in the same order (cost_host / advance_host), so there is nothing for an ulp to come from.  (The softmax draw compares
exp() values, which need not agree to the last bit between the two maths libraries; its output is an index, and the uniforms of these
tests stay 1e-9 away from every interval end.)
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
UAV = {"max_v": 2.0, "max_a": 2.0}
RES, EPS, GAMMA = 4.0, 0.5, 0.95
SHAPES = {1: (0, 1), 63: (1, 7), 64: (0, 64), 65: (0, 65), 98: (3, 2), 130: (0, 130)}  # kmax -> (half, n_levels): kmax = (2 half + 1)^2 levels


def make(n, kmax, gcb, max_depth=3, node_base=1000, flight=True):
    import torch

    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_rollout as dr

    dev = torch.device("cuda:0")
    half, n_levels = SHAPES[kmax]
    t = dr.rollout_buffers(torch, dev, n, kmax, max_depth)
    levels = torch.linspace(8.0, 8.0 + 6.0 * (n_levels - 1), n_levels, dtype=torch.float64, device=dev)
    ro = dr.rollout_struct(t, levels, gcb=gcb, grid_w=10, grid_h=10, half=half, node_base=node_base, device_index=0,
                           flags=_ffi.IPP_ADAPTIVE | (_ffi.IPP_USE_FLIGHT_TIME if flight else 0), resolution=RES, radius=9.0, gamma=GAMMA,
                           epsilon=EPS, vmax=UAV["max_v"], amax=UAV["max_a"])
    return t, ro, levels


def put(t, **arrays):
    import torch

    for name, a in arrays.items():
        t[name].copy_(torch.as_tensor(np.ascontiguousarray(a)).to(t[name].device).reshape(t[name].shape))


def get(t, *names):
    return [t[n].detach().cpu().numpy() for n in names]


def check_pick(rows, kmax, gcb, level=1, max_depth=3, node_base=1000):
    """rows: dicts with cand [k, 3], reward [k] f32, cost [k], status [k], budget, depth_left, u0, u1, live.  One ipp_rollout_pick launch
    for all of them, compared row by row with pick_host.  Returns the picked indices."""
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_rollout as dr

    n = len(rows)
    t, ro, levels = make(n, kmax, gcb, max_depth, node_base)
    u = np.zeros((n, max_depth, 2))
    for i, r in enumerate(rows):
        u[i, level] = (r["u0"], r["u1"])
    put(t, cand=np.array([r["cand"] for r in rows]), reward=np.array([r["reward"] for r in rows], dtype=np.float32),
        cost=np.array([r["cost"] for r in rows]), status=np.array([r["status"] for r in rows], dtype=np.int32),
        budget=np.array([r["budget"] for r in rows]), depth_left=np.array([r["depth_left"] for r in rows], dtype=np.int32),
        live=np.array([r["live"] for r in rows], dtype=np.int32), u=u, pick_idx=np.full((n, max_depth), -1, dtype=np.int32),
        flag=np.zeros(n, dtype=np.int32), action=np.full((n, 3), 7.0), new_id=np.full(n, 77, dtype=np.int32))
    _ffi.check(_ffi.load().ipp_rollout_pick(C.byref(ro), level, None))
    action, new_id, pick_idx, live, flag = get(t, "action", "new_id", "pick_idx", "live", "flag")
    picked = []
    for i, r in enumerate(rows):
        if not r["live"]:
            idx, fl = -1, 0   # a rollout that ended earlier: a NaN action, nothing else changes
        else:
            idx, fl = dr.pick_host(r["cand"], np.asarray(r["reward"], dtype=np.float32), r["cost"], r["status"], r["budget"], r["depth_left"],
                                   r["u0"], r["u1"], resolution=RES, epsilon=EPS, gcb=gcb)
        picked.append(idx)
        if idx >= 0:
            assert int(pick_idx[i, level]) == idx, (i, int(pick_idx[i, level]), idx)
            assert np.array_equal(action[i], r["cand"][idx]) and int(new_id[i]) == node_base + i * max_depth + level
            assert int(live[i]) == 1 and int(flag[i]) == dr.RUNNING
        else:
            assert np.isnan(action[i]).all() and int(new_id[i]) == -1 and int(live[i]) == 0 and int(flag[i]) == fl, (i, int(flag[i]), fl)
            assert int(pick_idx[i, level]) == -1
        assert np.array_equal(pick_idx[i, [q for q in range(max_depth) if q != level]], [-1] * (max_depth - 1))
    return picked


def generic_row(rs, k, **over):
    cand = rs.uniform(0, 40, size=(k, 3))
    cand[rs.uniform(size=k) < 0.3] = np.nan                       # no candidate
    cost = rs.uniform(0.5, 12.0, size=k)
    cost[rs.uniform(size=k) < 0.1] = 0.0                          # the waypoint itself
    cost[np.isnan(cand).any(axis=1)] = np.nan
    row = dict(cand=cand, reward=rs.uniform(0, 2, size=k).astype(np.float32), cost=cost, status=np.zeros(k, dtype=np.int32),
               budget=float(rs.uniform(5.0, 11.0)), depth_left=2, u0=float(rs.uniform()), u1=float(rs.uniform()), live=1)
    row.update(over)
    return row


@pytest.mark.parametrize("gcb", [False, True])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("kmax", [1, 63, 64, 65, 98, 130])
def test_pick_equals_the_host_restatement(kmax, n, gcb):
    rs = np.random.RandomState(1000 * kmax + 10 * n + int(gcb))
    rows = [generic_row(rs, kmax) for _ in range(n)]
    if n == 5:
        rows[1].update(u0=0.9)                     # greedy for sure (eps mode)
        rows[2].update(u0=0.1)                     # random for sure
        rows[3].update(live=0)                     # ended earlier
        rows[4].update(budget=3.5)                 # budget < resolution
    else:
        rows[0].update(u0=0.9 if kmax % 2 else 0.1)
    check_pick(rows, kmax, gcb)


@pytest.mark.parametrize("gcb", [False, True])
def test_pick_edge_cases(gcb):
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_rollout as dr

    k = 130
    rs = np.random.RandomState(5)

    def base(**over):
        row = dict(cand=rs.uniform(0, 40, size=(k, 3)), reward=rs.uniform(0, 1, size=k).astype(np.float32), cost=np.full(k, 3.0),
                   status=np.zeros(k, dtype=np.int32), budget=50.0, depth_left=2, u0=0.9, u1=0.37, live=1)
        row.update(over)
        return row

    rows = []
    r = base()                                   # 0: equal maxima at lanes 63 and 64 (two waves' worth of candidates): the first wins
    r["reward"][63] = r["reward"][64] = np.float32(5.0)
    rows.append(r)
    c = np.zeros(k)                              # 1: only the last candidate is available
    c[k - 1] = 2.0
    rows.append(base(cost=c, u0=0.1, u1=0.999))
    rows.append(base(cost=c, u0=0.9))            # 2: ... greedy
    r = base()                                   # 3: NaN rewards among finite ones never win, also not in front
    r["reward"][[0, 5, 64, 129]] = np.nan
    rows.append(r)
    rows.append(base(cost=np.zeros(k), u0=0.9))  # 4, 5: count 0, greedy draw and random draw
    rows.append(base(cost=np.full(k, 60.0), u0=0.1))
    rows.append(base(budget=3.999))              # 6: budget < resolution
    rows.append(base(depth_left=0))              # 7: depth_left == 0
    rows.append(base(reward=np.full(k, 0.25, dtype=np.float32), u1=64.5 / k))  # 8: equal rewards (cost-benefit: k intervals of 1 / k)
    s = np.zeros(k, dtype=np.int32)              # 9: BAD_FOOTPRINT on an available candidate
    s[70] = _ffi.STATUS_BAD_FOOTPRINT
    rows.append(base(status=s))
    c = np.full(k, 3.0)                          # 10: ... on an unavailable one: no error
    c[70] = 0.0
    rows.append(base(status=s, cost=c))
    r = base(u0=EPS, u1=0.0)                     # 11: u0 == epsilon is not greedy: the first available
    rows.append(r)
    rows.append(base(u0=0.2, u1=1.0 - 2.0 ** -53))  # 12: the largest uniform: the last available
    r = base()                                   # 13: every reward NaN
    r["reward"][:] = np.nan
    rows.append(r)
    picked = check_pick(rows, k, gcb)
    if not gcb:
        assert picked[0] == 63 and picked[1] == k - 1 and picked[2] == k - 1 and picked[11] == 0 and picked[12] == k - 1
        assert picked[3] == int(np.nanargmax(rows[3]["reward"])) and picked[8] == 0 and picked[10] >= 0
    else:
        assert picked[1] == k - 1 and picked[2] == k - 1 and picked[8] == 64 and picked[10] >= 0
    # the flags, literally (check_pick compared them with pick_host)
    want = {4: dr.NO_ACTION, 5: dr.NO_ACTION, 6: dr.END, 7: dr.END, 9: dr.ERR_FOOTPRINT, 13: dr.ERR_NAN}
    if gcb:
        want[3] = dr.ERR_NAN                      # a NaN among the softmax's inputs
    for i, fl in want.items():
        assert picked[i] == -1
        assert dr.pick_host(rows[i]["cand"], rows[i]["reward"], rows[i]["cost"], rows[i]["status"], rows[i]["budget"], rows[i]["depth_left"],
                            rows[i]["u0"], rows[i]["u1"], resolution=RES, epsilon=EPS, gcb=gcb)[1] == fl


@pytest.mark.parametrize("flight", [True, False])
@pytest.mark.parametrize("n", [1, 5])
def test_advance_equals_the_host_restatement_bit_for_bit(n, flight):
    """Two levels: the first charges the flight from the node's own waypoint, the second from the GRANDPARENT's (mcts_mission.py:226)."""
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_rollout as dr

    rs = np.random.RandomState(40 + n)
    uav = UAV if flight else None
    t, ro, levels = make(n, 1, False, flight=flight)
    cur = rs.uniform(0, 40, size=(n, 3))
    budget = rs.uniform(20, 60, size=n)
    plen = np.array([0, 1, 4, 5, 2][:n], dtype=np.int32)
    path = np.full((n, 6), -1, dtype=np.int32)
    for i in range(n):
        path[i, : plen[i]] = 10 * i + np.arange(plen[i])
    states = [dr.new_state(i, path[i], cur[i], budget[i], 3) for i in range(n)]
    put(t, root=np.arange(n, dtype=np.int32), path=path, plen=plen, cur=cur, charge_from=cur, budget=budget,
        depth_left=np.full(n, 3, dtype=np.int32), value=np.zeros(n), disc=np.ones(n), live=np.ones(n, dtype=np.int32), flag=np.zeros(n, dtype=np.int32))
    statuses = [[0, 0, 0, 0, _ffi.STATUS_NOT_PD][:n], [0, _ffi.STATUS_RANK_FULL, 0, 0, 0][:n]]
    for level in range(2):
        action = rs.uniform(0, 40, size=(n, 3))
        reward = rs.uniform(0, 2, size=n).astype(np.float32)
        new_id = (500 + 3 * np.arange(n) + level).astype(np.int32)
        put(t, action=action, new_id=new_id, step_reward=reward, step_status=np.array(statuses[level], dtype=np.int32))
        _ffi.check(_ffi.load().ipp_rollout_advance(C.byref(ro), None))
        for i in range(n):
            dr.advance_host(states[i], action[i], int(new_id[i]), reward[i], statuses[level][i], gamma=GAMMA, uav=uav)
        value, disc, bud, cu, cf, pa, pl, dl, live, flag = get(t, "value", "disc", "budget", "cur", "charge_from", "path", "plen", "depth_left",
                                                               "live", "flag")
        for i, st in enumerate(states):
            for got, want in ((value[i], st["value"]), (disc[i], st["disc"]), (bud[i], st["budget"])):
                assert np.float64(got).tobytes() == np.float64(want).tobytes(), (level, i, got, want)
            assert np.array_equal(cu[i], st["cur"]) and np.array_equal(cf[i], st["charge_from"])
            assert pa[i].tolist() == st["path"] and int(pl[i]) == st["plen"] and int(dl[i]) == st["depth_left"]
            assert int(live[i]) == st["live"] and int(flag[i]) == st["flag"]
    # the quirk itself: after the second level the budget is the start minus the two flights FROM THE START waypoint
    i = 0
    assert states[i]["live"] and states[i]["depth_left"] == 1
    assert states[i]["budget"] == (budget[i] - dr.cost_host(states[i]["charge_from"], cur[i], uav)) - dr.cost_host(states[i]["cur"], cur[i], uav)
    if n == 5:
        assert [s["flag"] for s in states] == [0, dr.RANK_FULL, 0, 0, dr.ERR_STEP]
        assert states[3]["plen"] == 6 and states[3]["path"][5] == 500 + 3 * 3  # a full path is not written past its end


@pytest.mark.parametrize("n", [1, 5])
def test_candidates_equal_radius_candidates(n):
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning.vec_greedy import radius_candidates

    t, ro, levels = make(n, 98, False)
    cur = np.array([[2.0, 2.0, 14.0], [22.0, 18.0, 8.0], [38.0, 38.0, 14.0], [21.0, 17.5, 11.0], [6.0, 34.0, 8.0]][:n])
    live = np.array([1, 1, 1, 1, 0][:n], dtype=np.int32)
    put(t, cur=cur, live=live, cand=np.full((n, 98, 3), 5.0))
    _ffi.check(_ffi.load().ipp_rollout_candidates(C.byref(ro), None))
    (cand,) = get(t, "cand")
    for i in range(n):
        want = radius_candidates(cur[i], 10, 10, RES, 8.0, 14.0, 6.0, 9.0) if live[i] else np.full((98, 3), np.nan)
        assert np.array_equal(cand[i], want, equal_nan=True), i
