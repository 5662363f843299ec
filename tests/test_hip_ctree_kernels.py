"""
GPU tests of the device tree search's kernels on bare tables, no engine (csrc/k_ctree.h: ipp_ctree_descend, _attach, _backup, _best)
against the host restatements of planning/device_ctree.py, on the hand-built tables of tests/ctree_cases.py: three roots per launch,
cap = 9 slots, horizon 3, kmax = 18 (the two widening cases need 33 children and more than 33 available actions: cap = 40, kmax = 98).

Slot choices, counters, kinds, traces and flags must match exactly.  Budgets and value_sum must be BIT-equal: they are sums,
differences, one sqrt and divisions, compiled without fused multiply-adds, correctly rounded on the device as in CPython and taken in
the same order.  UCT values involve log(): the cases keep the best and the second UCT more than 1e-6 apart, except the exact-tie
cases, whose children have identical fields and so identical UCT values on either side.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctree_cases as cases

pytestmark = pytest.mark.gpu
R = 3
SENTINEL = -7.0


def chunks(names, n=R):
    names = sorted(names)
    out = [names[i:i + n] for i in range(0, len(names), n)]
    out[-1] = (out[-1] + names)[:n]   # the last launch is filled up with the first cases
    return out


def launch_setup(tables, P, cap):
    """Device tables holding `tables` (one per root) and the two states (every row dead, sentinels in what a kernel may write)."""
    import torch

    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc
    from ipp_rl_amd.planning import device_rollout as dr

    dev = torch.device("cuda:0")
    n, horizon = len(tables), int(P["horizon"])
    t = dc.ctree_buffers(torch, dev, n, cap, horizon, len(P["thr"]))

    def put(buf, name, arr):
        buf[name].copy_(torch.as_tensor(np.ascontiguousarray(arr)).to(dev).reshape(buf[name].shape))

    put(t, "thr", P["thr"])
    put(t, "root_slot", np.arange(5, 5 + n, dtype=np.int32))
    for name in dc.NODE_FIELDS + dc.ROOT_FIELDS:
        put(t, name, np.array([T[name] for T in tables]))
    levels = torch.as_tensor(dc.altitude_levels(P["min_altitude"], P["max_altitude"], P["altitude_spacing"]), dtype=torch.float64, device=dev)
    half = int(np.ceil(P["radius"] / P["resolution"]))
    kmax = (2 * half + 1) ** 2 * int(levels.numel())
    kw = dict(grid_w=P["x_dim"], grid_h=P["y_dim"], half=half, device_index=0, flags=_ffi.IPP_ADAPTIVE | _ffi.IPP_USE_FLIGHT_TIME,
              resolution=P["resolution"], radius=P["radius"], gamma=0.95, vmax=P["uav"]["max_v"], amax=P["uav"]["max_a"])
    ex_t, ro_t = dr.rollout_buffers(torch, dev, n, kmax, 1), dr.rollout_buffers(torch, dev, n, kmax, horizon)
    for st in (ex_t, ro_t):
        for name in ("budget", "value", "disc", "cur", "charge_from"):
            st[name].fill_(SENTINEL)
        for name in ("root", "path", "plen", "depth_left", "flag"):
            st[name].fill_(int(SENTINEL))
    ex = dr.rollout_struct(ex_t, levels, gcb=False, node_base=0, epsilon=0.2, **kw)
    ro = dr.rollout_struct(ro_t, levels, gcb=False, node_base=900, epsilon=0.5, **kw)
    ct = dc.ctree_struct(t, c=P["c"], tree_node_base=0, device_index=0)
    return dict(t=t, ct=ct, ex_t=ex_t, ex=ex, ro_t=ro_t, ro=ro, levels=levels, put=put, kmax=kmax)


def fetch(buf):
    return {k: v.detach().cpu().numpy() for k, v in buf.items()}


def same_tables(got, i, T, fields):
    for name in fields:
        want, have = np.asarray(T[name]), np.asarray(got[name][i])
        assert have.dtype == (np.float64 if want.dtype.kind == "f" else np.int32), name
        assert have.tobytes() == want.astype(have.dtype).tobytes(), (name, have, want)


def same_row(st, i, row):
    """Row i of a downloaded ipp_rollout state against a new_state row (None: the row is dead and otherwise untouched)."""
    if row is None:
        assert int(st["live"][i]) == 0
        assert st["budget"][i] == SENTINEL and int(st["plen"][i]) == int(SENTINEL) and np.all(st["cur"][i] == SENTINEL)
        return
    assert int(st["live"][i]) == 1 and int(st["flag"][i]) == 0 and int(st["root"][i]) == row["root"]
    assert st["path"][i].tolist() == row["path"] and int(st["plen"][i]) == row["plen"] and int(st["depth_left"][i]) == row["depth_left"]
    assert np.array_equal(st["cur"][i], row["cur"]) and np.array_equal(st["charge_from"][i], row["charge_from"])
    assert np.float64(st["budget"][i]).tobytes() == np.float64(row["budget"]).tobytes()
    assert st["value"][i] == 0.0 and st["disc"][i] == 1.0


def copy_table(T):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in T.items()}


def descend_groups():
    """Launches of three cases that share their widening table and geometry."""
    out = []
    allc = cases.descend_cases()
    keys = {}
    for name, cs in allc.items():
        keys.setdefault(cs["P"]["thr"].tobytes(), []).append(name)
    for names in keys.values():
        out += [("small", tuple(ch)) for ch in chunks(names)]
    out.append(("wide", tuple(chunks(cases.widening_cases())[0])))
    return out


@pytest.mark.parametrize("kind, names", descend_groups(), ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_descend_equals_the_host_restatement(kind, names):
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc

    allc = cases.descend_cases() if kind == "small" else cases.widening_cases()
    cs = [allc[n] for n in names]
    P = cs[0]["P"]
    cap = len(cs[0]["T"]["parent"])
    assert (cap, P["horizon"]) == ((9, 3) if kind == "small" else (40, 3))
    s = launch_setup([c["T"] for c in cs], P, cap)
    assert s["kmax"] == (18 if kind == "small" else 98)
    s["put"](s["t"], "root_wp", np.array([c["wp"] for c in cs]))
    s["put"](s["t"], "root_budget", np.array([c["budget"] for c in cs]))
    s["put"](s["t"], "tie_u", np.array([c["tie"] for c in cs]))
    for st in (s["ex_t"], s["ro_t"]):
        st["live"].fill_(1)   # (a descent must leave every row it does not use dead)
    _ffi.check(_ffi.load().ipp_ctree_descend(C.byref(s["ct"]), C.byref(s["ex"]), C.byref(s["ro"]), None))
    got, ex, ro = fetch(s["t"]), fetch(s["ex_t"]), fetch(s["ro_t"])
    for i, c in enumerate(cs):
        T = copy_table(c["T"])
        k, row = dc.descend_host(T, 5 + i, c["wp"], c["budget"], c["tie"], P)
        same_tables(got, i, T, dc.NODE_FIELDS + dc.ROOT_FIELDS)
        same_row(ex, i, row if k == dc.EXPAND else None)
        same_row(ro, i, row if k == dc.ROLLOUT else None)
        if c["kind"] is None:
            assert int(got["err"][i]) != 0
        else:   # the outcome written down with the case
            assert int(got["err"][i]) == 0 and int(got["leaf_kind"][i]) == c["kind"]
            assert got["t_slot"][i][: int(got["t_len"][i])].tolist() == c["trace"]


@pytest.mark.parametrize("names", chunks(cases.attach_cases()), ids="-".join)
def test_attach_equals_the_host_restatement(names):
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc

    allc = cases.attach_cases()
    cs = [allc[n] for n in names]
    P = cs[0]["P"]
    s = launch_setup([c["T"] for c in cs], P, cases.CAP)
    s["put"](s["t"], "root_wp", np.array([c["T"]["action"][0] for c in cs]))
    e = s["ex_t"]
    s["put"](e, "live", np.array([c["ex"][0] for c in cs], dtype=np.int32))
    s["put"](e, "flag", np.array([c["ex"][1] for c in cs], dtype=np.int32))
    s["put"](e, "action", np.array([c["ex"][2] for c in cs]))
    s["put"](e, "new_id", np.array([c["ex"][3] for c in cs], dtype=np.int32))
    s["put"](e, "step_reward", np.array([c["ex"][4] for c in cs], dtype=np.float32))
    s["put"](e, "step_status", np.array([c["ex"][5] for c in cs], dtype=np.int32))
    _ffi.check(_ffi.load().ipp_ctree_attach(C.byref(s["ct"]), C.byref(s["ex"]), C.byref(s["ro"]), None))
    got, ro = fetch(s["t"]), fetch(s["ro_t"])
    for i, c in enumerate(cs):
        T = copy_table(c["T"])
        row = dc.attach_host(T, 5 + i, *c["ex"], P)
        same_tables(got, i, T, dc.NODE_FIELDS + dc.ROOT_FIELDS)
        same_row(ro, i, row)
        assert int(got["err"][i]) == c["err"] and int(got["leaf_kind"][i]) == c["kind"]


@pytest.mark.parametrize("names", chunks(cases.backup_cases()), ids="-".join)
def test_backup_equals_the_host_restatement(names):
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc

    allc = cases.backup_cases()
    cs = [allc[n] for n in names]
    P = cs[0]["P"]
    s = launch_setup([c["T"] for c in cs], P, cases.CAP)
    s["put"](s["t"], "root_wp", np.array([c["T"]["action"][0] for c in cs]))
    s["put"](s["ro_t"], "value", np.array([c["value"] for c in cs]))
    s["put"](s["ro_t"], "flag", np.array([c["flag"] for c in cs], dtype=np.int32))
    _ffi.check(_ffi.load().ipp_ctree_backup(C.byref(s["ct"]), C.byref(s["ro"]), None))
    got = fetch(s["t"])
    for i, c in enumerate(cs):
        T = copy_table(c["T"])
        dc.backup_host(T, c["value"], c["flag"], P)
        same_tables(got, i, T, dc.NODE_FIELDS + dc.ROOT_FIELDS)
        assert int(got["err"][i]) == c["err"] and got["visits"][i][:4].tolist() == c["visits"]
        assert got["value_sum"][i][:4].tobytes() == np.array(c["value_sum"], dtype=np.float64).tobytes()


@pytest.mark.parametrize("names", chunks(cases.best_cases()), ids="-".join)
def test_best_equals_the_host_restatement(names):
    import torch

    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc

    allc = cases.best_cases()
    cs = [allc[n] for n in names]
    s = launch_setup([c["T"] for c in cs], cases.params(), cases.CAP)
    s["put"](s["t"], "root_wp", np.array([c["wp"] for c in cs]))
    action = torch.full((R, 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    has = torch.full((R,), 9, dtype=torch.int32, device="cuda:0")
    _ffi.check(_ffi.load().ipp_ctree_best(C.byref(s["ct"]), action.data_ptr(), has.data_ptr(), None))
    a, h = action.cpu().numpy(), has.cpu().numpy()
    got = fetch(s["t"])
    for i, c in enumerate(cs):
        wa, wh = dc.best_host(c["T"], c["wp"])
        assert int(h[i]) == wh == c["has"] and np.array_equal(a[i], wa) and np.array_equal(a[i], c["action"])
        same_tables(got, i, c["T"], dc.NODE_FIELDS + dc.ROOT_FIELDS)   # a read-out: nothing is written


def test_calls_are_validated():
    import torch

    from ipp_rl_amd import _ffi

    cs = cases.best_cases()["no_child"]
    s = launch_setup([cs["T"]] * R, cases.params(), cases.CAP)
    lib = _ffi.load()
    s["ct"].horizon = 7
    with pytest.raises(_ffi.IppError, match="horizon"):
        _ffi.check(lib.ipp_ctree_descend(C.byref(s["ct"]), C.byref(s["ex"]), C.byref(s["ro"]), None))
    s["ct"].horizon = 3
    s["ro"].max_depth = 2
    with pytest.raises(_ffi.IppError, match="max_depth"):
        _ffi.check(lib.ipp_ctree_attach(C.byref(s["ct"]), C.byref(s["ex"]), C.byref(s["ro"]), None))
    s["ro"].max_depth = 3
    s["ct"].err = None
    with pytest.raises(_ffi.IppError, match="null buffer"):
        _ffi.check(lib.ipp_ctree_backup(C.byref(s["ct"]), C.byref(s["ro"]), None))
    assert torch.cuda.is_available()
