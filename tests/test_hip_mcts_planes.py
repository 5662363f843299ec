"""
GPU tests of DeviceMCTS(feature_planes=True): every inference batch carries the planes of its leaves (mcts.py:178-204), built on
the device from the leaf's ancestry on its descent (ipp_mcts_plane_entries) and the roots' own histories (root_history).
  * the entries of the sampled leaves equal a host restatement read from the search's tables, and their planes equal planes from
    those host-built entries;
  * groups = 1 and groups = 2 (each group's own tables) give the same planes for the same leaves;
  * with uniform priors the trees and policies are bit-identical to feature_planes=False.
"""
import numpy as np
import pytest

from tests.test_hip_mcts import _search_setup

pytestmark = pytest.mark.gpu

DIM, R, SIMS, HORIZON, W = 40, 4, 6, 2, 2
PLANE_HP = dict(input_history_length=3, use_fov_input=False, use_action_costs_input=True)


def host(t):
    return t.detach().cpu().numpy()


def _root_history(eng, prev, H):
    from ipp_rl_amd.feature_planes import entry_tensor, make_entry, pack_entries

    # entry 0 = the root state, entry 1 = an older state of the same slot (its prior: rank 0)
    return entry_tensor(pack_entries([[make_entry(j, prev[j], 1.0), make_entry(j, [2.0, 2.0, 14.0], 1.0, rank=0)] for j in range(R)], H),
                        eng.device)


def _host_entries(batch, prev_all, bud_all, root_hist, H, b0):
    """The entries of every row of the batch, restated from the search's tables (include/ipp_engine.h: ipp_mcts_plane_entries)."""
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    s = batch["search"]
    b = {k: host(v) for k, v in s._buf.items() if k in ("counts", "pend_node", "pend_sim", "pend_prev", "pend_budget", "p_node", "p_k",
                                                       "p_cost", "p_len", "n_devpath", "t_idx")}
    Rg, D, Wg = s._tab_roots, s._tab_depth, s.sims_in_flight
    base, sim0 = batch["root_base"], batch["sim"]
    rows = []
    for j in range(Rg):
        for q in range(int(b["counts"][j])):
            g = j * Wg + q
            jj = base + j
            w = int(b["pend_sim"].reshape(-1)[g]) - sim0
            plen = int(b["p_len"].reshape(-1)[w * Rg + j])
            pn, pk, pc = (b[k].reshape(Wg, Rg, D)[w, j] for k in ("p_node", "p_k", "p_cost"))
            ents = [make_entry(jj, b["pend_prev"].reshape(-1, 3)[g], b["pend_budget"].reshape(-1)[g] / b0,
                               path=b["n_devpath"][int(b["pend_node"].reshape(-1)[g])])]
            for a in range(plen - 1, -1, -1):
                if len(ents) == H:
                    break
                budget = bud_all[jj]
                for e in range(a):
                    budget -= pc[e]
                pos = prev_all[jj] if a == 0 else s.actions_np[int(b["t_idx"][int(pn[a - 1]), int(pk[a - 1])])]
                ents.append(make_entry(jj, pos, budget / b0, path=b["n_devpath"][int(pn[a])]))
            if root_hist is not None:
                for e in root_hist[jj, 1:]:
                    if len(ents) < H:
                        ents.append(e)
            rows.append(ents)
    return pack_entries(rows, H)


def _run(groups, feature_planes, record):
    import torch

    from ipp_rl_amd.feature_planes import entry_records
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS

    eng, prev, hyper, meta = _search_setup(DIM, R, SIMS, HORIZON, eps=0.0, node_slack=16)
    assert eng.info.patch_layout == 1
    hyper = dict(hyper, **PLANE_HP)
    meta = dict(meta, altitude_spacing=3.0)  # (3 levels: 4800 actions, above DENSE_ACTIONS, so groups > 1 takes the grouped path)
    H = PLANE_HP["input_history_length"]
    budgets = np.full(R, 40.0)
    rh = _root_history(eng, prev, H) if feature_planes else None
    rh_host = entry_records(rh) if rh is not None else None
    checks = {"rows": 0, "host": 0}

    def infer(batch):
        value = 0.3 + 0.01 * (batch["K"].to(torch.float64) % 7)
        if feature_planes:
            planes = batch["planes"]
            spec = batch["search"].plane_spec
            assert tuple(planes.shape) == (len(batch["node"]), spec.channels, DIM * DIM, DIM * DIM)
            want = _host_entries(batch, prev, budgets, rh_host, H, float(meta["initial_budget"]))
            got = entry_records(batch["entries"])
            np.testing.assert_allclose(got["budget"], want["budget"], rtol=1e-15, atol=0)
            want["budget"] = got["budget"]
            assert got.tobytes() == want.tobytes()
            n = min(2, len(want))  # (planes of 40 x 40 are 10 MB: the first rows of every batch)
            ref = eng.feature_planes(want[:n], spec, mask_env=got["root_env"][:n, 0])
            assert torch.equal(torch.nan_to_num(planes[:n], nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
            checks["host"] += n
            proj = torch.nan_to_num(planes.double(), nan=-7.0).sum(dim=(2, 3))
            for i in range(len(want)):
                key = (int(want[i, 0]["root_env"]), int(batch["depth"][i]), tuple(host(batch["previous_action"][i]).tolist()),
                       float(batch["budget"][i]))
                record[key] = host(proj[i]).tobytes()
            checks["rows"] += len(want)
        return None, value

    s = DeviceMCTS(eng, hyper, meta, infer, sims_in_flight=W, tie_break="first", seed=3, groups=groups, feature_planes=feature_planes)
    out = s.get_policy(list(range(R)), prev, budgets, root_history=rh)
    assert (s._subs_used is not None) == (groups > 1)
    idx, nsa, q = s.root_statistics()
    eng.close()
    return out, idx.copy(), nsa.copy(), q.copy(), checks


def test_leaf_planes_groups_and_unchanged_trees():
    rec1, rec2 = {}, {}
    out0, idx0, nsa0, q0, _ = _run(1, False, {})
    out1, idx1, nsa1, q1, c1 = _run(1, True, rec1)
    out2, idx2, nsa2, q2, c2 = _run(2, True, rec2)
    assert c1["rows"] > R and c1["host"] > 0 and c2["host"] > 0
    # the planes of a leaf do not depend on how the roots were grouped
    assert rec1.keys() == rec2.keys() and all(rec1[k] == rec2[k] for k in rec1)
    # the planes are an extra input only: same trees and policies as without them
    for a, b in ((idx0, idx1), (nsa0, nsa1), (q0, q1), (idx0, idx2), (nsa0, nsa2), (q0, q2)):
        assert np.array_equal(a, b)
    assert [p[0] for p in out0] == [p[0] for p in out1] == [p[0] for p in out2]


def test_feature_planes_needs_infer_and_spec():
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS

    eng, prev, hyper, meta = _search_setup(DIM, R, SIMS, HORIZON, eps=0.0)
    with pytest.raises(ValueError):
        DeviceMCTS(eng, dict(hyper, **PLANE_HP), meta, None, feature_planes=True)
    with pytest.raises(ValueError):
        DeviceMCTS(eng, hyper, meta, lambda b: (None, 0.0), feature_planes=True)  # no input_history_length in hyper_params
    s = DeviceMCTS(eng, hyper, meta, lambda b: (None, 0.0))
    with pytest.raises(ValueError):
        s.get_policy(list(range(R)), prev, [40.0] * R, root_history=_root_history(eng, prev, 3))
    eng.close()
