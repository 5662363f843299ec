"""
GPU tests of csrc/k_mcts.h at kernel level: ipp_mcts_select (k_mcts_select<1..4, 0>), ipp_mcts_backup (k_mcts_backup and
k_mcts_backup_serial) and ipp_mcts_policy (k_mcts_policy) on bare tables (tests/mcts_table_cases.py: SyntheticTables, no engine, no
search) against the per-root sequential fp64 restatements of the same file, which tests/test_mcts_tables_host.py pins to the
reference's compute_uct / normalize_q_values / get_policy, to the host drivers and, composed into a search, to VectorMCTS; the same
file proves on the CPU that each frozen case reaches the edge it is named for ("Tree-search tables on bare tables", has
the table).

Everything the kernels store is compared bit for bit: paths, leaves, pending entries, children, hash tables, counters, flags, device
paths, the NaN / inf pattern of the edge numerators, virtual visits, error flags, the request list (as a set: its order across roots
is an atomic counter's), costs and budgets (sqrt and division are correctly rounded, contraction is off), Q and the visit counts
after a backup -- from both backup kernels -- and the policy at temperature 1.  The policies at other temperatures are the only
inexact output: within 1e-15 absolute of the restatement (the device's pow; the bar of test_device_read_out_equals_the_host_read_out).
A failure names the case, root, descent and level of the first difference.
"""
import numpy as np
import pytest

from tests import mcts_table_cases as mc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

POW_ATOL = 1e-15
BACKUP_WRITES = ("t_qsa", "t_nsa", "n_ns", "counts")
REQUEST_LISTS = ("rq_root", "rq_parent", "rq_k", "rq_child", "rq_newdev", "rq_cost", "rq_prev", "rq_action", "ts_paths")


def untouched(got, st, names, label):
    for k in names:
        assert mc.same_bits(got[k], st[k]), (label, k, "moved")


# ---------------------------------------------------------------------------------------------------- backup
def _check_backup(name, form):
    st, W = mc.build_backup(name, form)
    want, _ = mc.backup_ref(st, W)
    got = mc.SyntheticTables(st).backup(W)
    for j in range(st["roots"]):  # the first recorded step whose edge differs, in the order the backup takes them
        for w in range(W):
            for stp in range(int(st["p_len"][w, j]) - 1, -1, -1):
                e = (int(st["p_node"][w, j, stp]), int(st["p_k"][w, j, stp]))
                same = mc.same_bits(got["t_qsa"][e], want["t_qsa"][e]) and mc.same_bits(got["t_nsa"][e], want["t_nsa"][e])
                assert same, (f"{name} ({form}): root {j}, descent {w}, step {stp}, edge {e}: (Q, count) got "
                              f"{float(got['t_qsa'][e])!r}, {float(got['t_nsa'][e])!r}, want {float(want['t_qsa'][e])!r}, {float(want['t_nsa'][e])!r}")
    for k in ("t_qsa", "t_nsa", "n_ns"):
        assert mc.same_bits(got[k], want[k]), (name, form, k)
    assert not got["counts"].any() and st["counts"].all(), (name, form, "pend_count / rq_count not cleared")
    untouched(got, st, [k for k in mc.ARRAYS if k not in BACKUP_WRITES], (name, form))
    return got


@pytest.mark.parametrize("name", list(mc.BACKUP_CASES))
def test_backup_kernels_equal_the_sequential_backup_and_each_other(name):
    wave, serial = _check_backup(name, "wave"), _check_backup(name, "serial")
    for k in ("t_qsa", "t_nsa", "n_ns"):
        assert mc.same_bits(wave[k], serial[k]), (name, k, "the two kernels differ")


# ---------------------------------------------------------------------------------------------------- read-out
@pytest.mark.parametrize("name", list(mc.READOUT_CASES))
def test_read_out(name):
    c = mc.build_readout(name)
    st, tie_u = c["st"], c["tie_u"]
    R, kmax, npr = st["roots"], st["kmax"], st["nodes_per_root"]
    tables = mc.SyntheticTables(st)
    K = st["n_k"][np.arange(R) * npr]
    padding = np.arange(kmax)[None, :] >= K[:, None]
    worst = 0.0
    for t, d, want_idx in mc.readout_modes(name):
        policy, idx, ok, info = mc.policy_ref(st, tie_u, t, d)
        got = tables.policy(tie_u, t, d, want_idx)
        label = (name, "temperature", t, "deploy_time", d)
        assert np.array_equal(got["ok"], ok), (label, got["ok"], ok)
        assert np.array_equal(got["valid_idx"], idx if want_idx else np.full_like(idx, -9)), label
        for j in range(R):
            if t == 1.0:
                assert mc.same_bits(got["policy"][j], policy[j]), (f"{label}: root {j}, first slot {int(np.argmax(got['policy'][j] != policy[j]))}: "
                                                                   f"got {got['policy'][j][:8]}, want {policy[j][:8]}; {info[j]}")
            else:
                err = float(np.abs(got["policy"][j] - policy[j]).max())
                worst = max(worst, err)
                assert err <= POW_ATOL, (label, "root", j, err, info[j])
        assert not got["policy"][padding].any(), (label, "padding")
        assert not got["policy"][ok == 0].any(), (label, "rows of bad roots")
        untouched(got, st, mc.ARRAYS, label)
    print(f"read-out {name}: largest |device - restatement| at temperatures != 1: {worst:.3g}")


# ---------------------------------------------------------------------------------------------------- select
def _check_select(name):
    c, want, requests, info = mc.build_select(name)
    st, W = c["st"], c["W"]
    got = mc.SyntheticTables(st).select(c["root_env"], c["prev0"], c["budget0"], c["depth0"], c["sim0"], W, c["seed"])
    for j in range(st["roots"]):
        for w in range(W):
            for level in range(max(int(want["p_len"][w, j]), min(int(got["p_len"][w, j]), st["max_depth"]), 0)):
                g = (int(got["p_node"][w, j, level]), int(got["p_k"][w, j, level]), float(got["p_cost"][w, j, level]))
                e = (int(want["p_node"][w, j, level]), int(want["p_k"][w, j, level]), float(want["p_cost"][w, j, level]))
                same = g[:2] == e[:2] and mc.same_bits(got["p_cost"][w, j, level], want["p_cost"][w, j, level])
                assert same, (f"{name}: root {j}, descent {w}, level {level}: (node, k, cost) got {g}, want {e}; "
                              f"{info[(j, w)][level] if level < len(info[(j, w)]) else None}")
            ends = (int(got["p_len"][w, j]), int(got["leaf"][w, j])), (int(want["p_len"][w, j]), int(want["leaf"][w, j]))
            assert ends[0] == ends[1], f"{name}: root {j}, descent {w}: (p_len, leaf) got {ends[0]}, want {ends[1]}"
    assert np.array_equal(got["counts"], want["counts"]), (name, "pend_count, rq_count", got["counts"], want["counts"])
    assert mc.requests_of(got) == mc.requests_ref(requests), (name, "request set")
    n = int(want["counts"][-1])
    for k in REQUEST_LISTS:  # nothing beyond the list's end
        assert mc.same_bits(got[k][n:], st[k][n:]), (name, k, "beyond the list")
    for k in mc.ARRAYS:  # every other buffer, written or not, as the sequential descents leave it
        if k not in REQUEST_LISTS:
            assert mc.same_bits(got[k], want[k]), (name, k, np.argwhere(mc.bits(got[k]) != mc.bits(want[k]))[:4].tolist())
    return c, want, got, info


@pytest.mark.parametrize("name", list(mc.SELECT_CASES))
def test_select(name):
    c, want, got, info = _check_select(name)
    st, W = c["st"], c["W"]
    # (what the comparison above covered, said once more where a whole-array comparison could hide it)
    assert np.array_equal(np.isnan(got["t_num"]), np.isnan(want["t_num"])) and np.array_equal(np.isinf(got["t_num"]), np.isinf(want["t_num"]))
    if W == 1:
        assert mc.same_bits(got["t_nsa"], st["t_nsa"]) and mc.same_bits(got["n_ns"], st["n_ns"])
    else:
        assert np.nansum(got["t_nsa"]) - np.nansum(st["t_nsa"]) == got["p_len"][:W].sum()
