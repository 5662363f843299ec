"""
GPU tests of the paths of the device tree search (csrc/k_mcts.h) that tests/test_hip_mcts.py leaves open:

  * the Dirichlet noise of the root priors, value by value against the fp64 restatement of the counter-based stream
    (tests/mcts_noise_ref.py; its own ties to the mathematics are in tests/test_mcts_noise_host.py) -- shapes below 1 (the boost
    branch of mc_gamma, what training runs after the first iterations), at 1 and above, rows of 162 and 338 entries, priors given by
    a network, and the second group of a grouped search (noise keyed on the root's number in the WHOLE search);
  * network priors, a discount below 1, budgets that decide the valid set (and leave leaves without any valid action) and tree nodes
    stored as patches (k_tree_patch writes the edge numerators itself), each against the NumPy driver VectorMCTS on the same device
    states with lowest-index tie-breaking: the same trees;
  * network priors in a grouped search against the search in one piece, bit for bit.

DESIGN.md ("Tree search: priors, noise, discount") holds the measured errors and the edits of the kernels each test was seen to catch.
"""
import numpy as np
import pytest

from tests.mcts_noise_ref import NOISE_CASES, NOISE_EPS, case_roots, noisy_priors_ref, prior_of
from tests.test_hip_mcts import _search_setup

pytestmark = pytest.mark.gpu
HORIZON = 4
NOISE_RTOL = 1e-12  # fp64 libm within a few ulp, gsum + rest: at most 339 summands in another order -> 1e-13, and a factor 10


def value_of_K(K):
    return 0.05 * float(int(K) % 7) + 0.3


def host_infer(priors):
    """The stub network for VectorMCTS: value from the size of the valid set; priors (if any) prior_of(action index) in the form
    VectorMCTS._vexpand expects -- dense over all actions when the request carries the mask, on valid_idx otherwise."""
    def infer(reqs):
        out = []
        for r in reqs:
            vi = np.asarray(r["valid_idx"])
            policy = None
            if priors:
                policy = prior_of(vi)
                if r["action_msk"] is not None:
                    policy = np.zeros(len(r["action_msk"]))
                    policy[vi] = prior_of(vi)
            out.append((policy, value_of_K(len(vi))))
        return out
    return infer


def device_infer(priors, asked=None):
    """The same network asked with tensors (DeviceMCTS): prior [n, kmax] on the valid sets, 0 on the -1 padding."""
    import torch

    def infer(batch):
        K = batch["K"].to(torch.float64)
        if asked is not None:
            asked.append((int(K.numel()), int((batch["K"] <= 0).sum())))
        vi = batch["valid_idx"].to(torch.int64)
        prior = None
        if priors:
            prior = torch.where(vi >= 0, 1.0 + torch.remainder(vi * 7919, 13).to(torch.float64), torch.zeros((), dtype=torch.float64, device=vi.device))
        return prior, 0.05 * torch.remainder(K, 7.0) + 0.3
    return infer


# ---------------------------------------------------------------------------------------------------- noise at the root
@pytest.mark.parametrize("case,alpha", [(name, alpha) for name, c in NOISE_CASES.items() for alpha in c["alphas"]])
def test_root_noise_equals_the_fp64_restatement(case, alpha):
    """After one search the root rows of t_Ps are the noisy priors of the first simulation: (1 - eps) prior + eps Dirichlet(alpha),
    normalised over all actions, every entry within 1e-12 (relative) of noisy_priors_ref at the root's number in the whole search.
    Only the root of the first simulation gets noise: an expanded node below a root holds the plain normalisation, bit for bit."""
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS

    c = NOISE_CASES[case]
    dim, R, sims = c["dim"], c["R"], 12
    eng, prev, hyper, meta = _search_setup(dim, R, sims, HORIZON, eps=NOISE_EPS, max_dist=c["max_dist"])
    hyper = dict(hyper, dirichlet_alpha=alpha)
    pos, valid = case_roots(dim, R, c["max_dist"])
    assert np.array_equal(pos, prev)  # (the keys whose acceptance margins the CPU test checked are the ones used here)
    A = 2 * dim * dim
    m = DeviceMCTS(eng, hyper, meta, device_infer(True) if c["given"] else None, sims_in_flight=4, tie_break="first", seed=c["seed"],
                   leaf_value=0.3, groups=c["groups"])
    assert m.num_actions == A
    m.get_policy(list(range(R)), prev, [60.0] * R)
    assert (m._subs_used is not None) == (c["groups"] > 1)
    ps, idx, Kd = m.t_Ps, m.t_idx, m.n_K
    worst = 0.0
    for j in range(R):
        K = len(valid[j])
        assert int(Kd[j]) == K and np.array_equal(idx[j, :K], valid[j]) and np.all(idx[j, K:] == -1)
        ref = noisy_priors_ref(c["seed"], j, K, A, alpha, NOISE_EPS, prior=prior_of(valid[j]) if c["given"] else None)
        worst = max(worst, float(np.max(np.abs(ps[j, :K] / ref - 1.0))))
        assert np.all(ps[j, K:] == 0)
    print(f"[{case}, alpha {alpha}] K {min(map(len, valid))}..{max(map(len, valid))} of kmax {ps.shape[1]}: largest relative error of a "
          f"noisy root prior {worst:.2e}")
    assert worst < NOISE_RTOL
    # ---- below the roots: no noise (the last group's tables, where the roots' numbers differ most from their numbers in the group)
    sub = m._subs_used[-1] if m._subs_used else m
    b, npr = sub._buf, sub.nodes_per_root
    flags, nk = b["n_flags"].cpu().numpy(), b["n_k"].cpu().numpy()
    below = [n for n in np.nonzero(flags & 1)[0] if n % npr != 0]
    assert len(below) >= R // c["groups"]  # (every root's second wave of simulations expanded a child)
    for n in below[:: max(1, len(below) // 8)]:
        K = int(nk[n])
        row, vi = b["t_ps"][int(n)].cpu().numpy(), b["t_idx"][int(n)].cpu().numpy().astype(np.int64)
        if c["given"]:
            p = prior_of(vi[:K])
            want = p / np.sum(p)
        else:
            want = np.full(K, (1.0 / A) / float(np.sum(np.full(K, 1.0 / A))))
        assert K > 0 and np.array_equal(row[:K], want) and np.all(row[K:] == 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------- against the host driver
PS_RTOL = 2.0 ** -49  # see _assert_same_trees


def _assert_same_trees(a, b, roots, exact_priors=False):
    """Root rows of VectorMCTS a and DeviceMCTS b: what test_device_search_builds_the_same_trees_as_the_host_driver asks, and the
    priors of the roots and of their expanded children.  Priors: the device divides by the total once; the host driver follows the
    reference's dense arithmetic (mcts.py:160-164, 224-225), which at the root of the first simulation normalises twice even with
    noise weight 0 and sums all A <= 3200 entries, zeros included -- the second total is 1 within (1 + log2 A) u <= 13 u of pairwise
    summation (u = 2^-53), one more rounding each for the two divisions: 16 u = 2^-49 relative.  exact_priors (small-integer priors
    from the network: every order gives the same total): below the roots, where both divide once, bit for bit."""
    idx_b, nsa_b, q_b = b.root_statistics()
    ps_b = b.t_Ps
    npr = b.nodes_per_root
    child_b, flags_b, nk_b = (b._buf[k].cpu().numpy() for k in ("t_child", "n_flags", "n_k"))
    worst, below = 0.0, 0
    for j in roots:
        rt = int(a.root_ids[j])
        K = int(a.n_K[rt]) if a.n_expanded[rt] else 0
        assert K == (int(b.n_K[j]) if b.n_expanded[j] else 0), j
        assert bool(a.n_expanded[rt]) == bool(b.n_expanded[j])
        assert np.array_equal(a.t_idx[rt, :K], idx_b[j, :K])
        assert np.array_equal(a.t_Nsa[rt, :K], nsa_b[j, :K]), (j, a.t_Nsa[rt, :K], nsa_b[j, :K])
        if K:
            assert np.max(np.abs(a.t_Qsa[rt, :K] - q_b[j, :K])) < 1e-6
            worst = max(worst, float(np.max(np.abs(ps_b[j, :K] / a.t_Ps[rt, :K] - 1.0))))
        for k in range(K):  # the root's children: the same nodes, the same valid sets and priors
            ca, cb = int(a.t_child[rt, k]), int(child_b[j * npr, k])
            assert (ca >= 0) == (cb >= 0)
            if ca < 0 or not a.n_expanded[ca]:
                assert cb < 0 or not (flags_b[cb] & 1)
                continue
            Kc = int(a.n_K[ca])
            assert (flags_b[cb] & 1) and int(nk_b[cb]) == Kc
            row_i, row_p = b._buf["t_idx"][cb].cpu().numpy(), b._buf["t_ps"][cb].cpu().numpy()
            assert np.array_equal(a.t_idx[ca, :Kc], row_i[:Kc]) and np.all(row_i[Kc:] == -1) and np.all(row_p[Kc:] == 0)
            if exact_priors:
                assert np.array_equal(a.t_Ps[ca, :Kc], row_p[:Kc]), (j, k, a.t_Ps[ca, :Kc], row_p[:Kc])
            worst = max(worst, float(np.max(np.abs(row_p[:Kc] / a.t_Ps[ca, :Kc] - 1.0))))
            below += 1
    print(f"priors of {len(roots)} roots and {below} children: largest relative difference device / host {worst:.2e}")
    assert worst < PS_RTOL and below >= len([j for j in roots if b.n_expanded[j]])
    assert a.stats["nodes"] == b.stats["nodes"] and a.stats["device_steps"] == b.stats["device_steps"]
    assert a.stats["inferences"] == b.stats["inferences"], (a.stats, b.stats)


# W = 16: more recorded steps than a wave has lanes (k_mcts_backup_serial); 40x40: tree nodes as patches, k_tree_patch writes t_num
@pytest.mark.parametrize("dim,gamma,priors,R,sims,W", [(20, 0.9, True, 16, 48, 4), (20, 0.9, True, 16, 48, 16), (40, 1.0, False, 8, 32, 4),
                                                       (40, 0.9, True, 8, 32, 4)])
def test_priors_and_discount_build_the_same_trees_as_the_host_driver(dim, gamma, priors, R, sims, W):
    """DeviceMCTS against VectorMCTS with priors from a 'network' (the prior != NULL branch of k_mcts_expand: wave sum of the row, then
    prior / total -- small integers, so that the total is exact in every order and equal trees are a fair demand) and a discount
    below 1 (val = reward + gamma value' in both backup kernels), on band-tile and on patch-layout engines."""
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS
    from ipp_rl_amd.planning.mcts_zero.vector_mcts import VectorMCTS

    eng, prev, hyper, meta = _search_setup(dim, R, sims, HORIZON, eps=0.0)
    hyper = dict(hyper, gamma=gamma)
    assert int(eng.info.patch_layout) == (1 if dim == 40 else 0)
    roots = list(range(R))
    rngs = lambda: [np.random.RandomState(7 + r) for r in roots]  # noqa: E731
    a = VectorMCTS(eng, hyper, meta, host_infer(priors), sims_in_flight=W, tie_break="first")
    a.get_policy(roots, prev, [60.0] * R, rngs=rngs())
    asked = []
    b = DeviceMCTS(eng, hyper, meta, device_infer(priors, asked), sims_in_flight=W, tie_break="first")
    b.get_policy(roots, prev, [60.0] * R, rngs=rngs())
    _assert_same_trees(a, b, roots, exact_priors=priors)
    assert b.stats["inferences"] == sum(n for n, _ in asked)
    if priors:  # (the priors are not uniform anywhere: the selection kernel saw unequal Ps)
        assert all(len(np.unique(b.t_Ps[j, :int(b.n_K[j])])) > 1 for j in roots)
    if gamma != 1.0:  # the parameter matters: the same search without discount has other root values
        q_b = b.t_Qsa.copy()
        c = DeviceMCTS(eng, dict(hyper, gamma=1.0), meta, device_infer(priors), sims_in_flight=W, tie_break="first")
        c.get_policy(roots, prev, [60.0] * R, rngs=rngs())
        diff = float(np.max(np.abs(q_b - c.t_Qsa)))
        print(f"largest change of a root Q from gamma {gamma} to 1: {diff:.3e}")
        assert diff > 1e-3
    eng.close()


@pytest.mark.parametrize("network", [True, False])
def test_budgets_that_decide_the_valid_sets(network):
    """Budgets from below the nearest action (3: no valid action at all, both drivers return None) over exactly the in-plane (4) and
    the altitude (6) neighbour distance (dist <= budget against <) up to 60 (max_valid_action_distance decides): the same valid
    sets and trees as the host driver, leaves without a valid action (mcts.py:201-202: value 0, stays a leaf, no inference) included.
    With a network asked with tensors, and with the stub (infer=None: constant leaf value, the inferences counted from the node flags)."""
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS
    from ipp_rl_amd.planning.mcts_zero.vector_mcts import VectorMCTS

    dim, R, sims, W = 20, 16, 48, 4
    eng, prev, hyper, meta = _search_setup(dim, R, sims, HORIZON, eps=0.0)
    hyper = dict(hyper, gamma=0.9)
    budgets = [3.0, 4.0, 6.0, 9.0, 14.0, 25.0, 40.0, 60.0] * 2
    prev = prev.copy()
    prev[:8], prev[8:] = prev[0], prev[8]  # every budget at the same position, twice (the search only needs a position, not the env's last)
    roots = list(range(R))
    rngs = lambda: [np.random.RandomState(7 + r) for r in roots]  # noqa: E731
    constant = lambda reqs: [(None, 0.3) for _ in reqs]  # noqa: E731
    a = VectorMCTS(eng, hyper, meta, host_infer(False) if network else constant, sims_in_flight=W, tie_break="first")
    out_a = a.get_policy(roots, prev, budgets, rngs=rngs())
    asked = []
    b = DeviceMCTS(eng, hyper, meta, device_infer(False, asked) if network else None, sims_in_flight=W, tie_break="first", leaf_value=0.3)
    # n_k is written when a node's valid set is computed: a recognisable filler tells "no valid action" from "never looked at"
    b._alloc(R, HORIZON + 1)
    b._buf["n_k"].fill_(-7)
    out_b = b.get_policy(roots, prev, budgets, rngs=rngs())
    _assert_same_trees(a, b, roots)
    for j in roots:
        assert (out_a[j] is None) == (out_b[j] is None) == (budgets[j] == 3.0), j
    nK = b.n_K
    print("K by budget:", {bud: (int(nK[i]), int(nK[i + 8])) for i, bud in enumerate(budgets[:8])})
    assert nK[0] == nK[8] == 0
    for half in (0, 8):
        assert 0 < nK[half + 1] < nK[half + 2] < nK[half + 7]  # budget 4 < budget 6 < budget 60 at one position
    # the network is not asked about leaves without a valid action
    if network:
        assert b.stats["inferences"] == sum(n for n, _ in asked) and all(z == 0 for _, z in asked)
    assert b.stats["inferences"] == b.stats["nodes"] == a.stats["inferences"] > 0  # (every leaf asked about was expanded, once)
    # leaves below the roots without a valid action were reached
    npr = b.nodes_per_root
    nk = b._buf["n_k"].cpu().numpy().reshape(R, npr)
    flags = b._buf["n_flags"].cpu().numpy().reshape(R, npr)
    cnt = b._buf["root_count"].cpu().numpy()
    assert all(np.all(nk[j, int(cnt[j]):] == -7) for j in roots) and all(cnt[j] < npr for j in roots)  # (the filler survived the search)
    dead = [(j, n) for j in roots for n in range(1, int(cnt[j])) if nk[j, n] == 0]
    print(f"{len(dead)} leaves below the roots without a valid action")
    assert dead and all(not (flags[j, n] & 1) for j, n in dead)
    eng.close()


def test_network_priors_in_a_grouped_search_equal_the_search_in_one_piece():
    """groups = 2 (the default) with a network that returns priors: _expand runs once per group on the group's stream and scatters the
    replies into the group's own slots.  Random ties, Dirichlet noise with shape 0.3: statistics, policies and the as_arrays outputs
    equal the search in one piece bit for bit."""
    from ipp_rl_amd.planning.mcts_zero.device_mcts import DeviceMCTS

    dim, R, sims, W = 50, 37, 32, 4
    eng, prev, hyper, meta = _search_setup(dim, R, sims, HORIZON, eps=NOISE_EPS, node_slack=16)
    hyper = dict(hyper, dirichlet_alpha=0.3)
    assert int(eng.info.patch_layout) == 1 and eng.max_batch >= R * W
    roots = list(range(R))
    res = []
    for g in (1, 2):
        asked = []
        s = DeviceMCTS(eng, hyper, meta, device_infer(True, asked), sims_in_flight=W, tie_break="random", seed=9, groups=g)
        assert s.num_actions > s.DENSE_ACTIONS
        out = s.get_policy(roots, prev, [60.0] * R)
        assert (s._subs_used is not None) == (g > 1)
        idx, nsa, q = s.root_statistics()
        ps = s.t_Ps.copy()
        stats = dict(s.stats)
        arr = s.get_policy(roots, prev, [60.0] * R, as_arrays=True)
        res.append((out, idx.copy(), nsa.copy(), q.copy(), ps, stats, {k: v.cpu().numpy() for k, v in arr.items()}, sum(n for n, _ in asked)))
    (out_a, idx_a, nsa_a, q_a, ps_a, st_a, arr_a, n_a), (out_b, idx_b, nsa_b, q_b, ps_b, st_b, arr_b, n_b) = res
    assert np.array_equal(idx_a, idx_b) and np.array_equal(nsa_a, nsa_b) and np.array_equal(q_a, q_b) and np.array_equal(ps_a, ps_b)
    assert st_a["nodes"] == st_b["nodes"] and st_a["device_steps"] == st_b["device_steps"] and st_a["inferences"] == st_b["inferences"]
    assert n_a == n_b
    for j in roots:
        assert out_a[j][0] == out_b[j][0] and np.array_equal(out_a[j][1], out_b[j][1])
        K = int((idx_a[j] >= 0).sum())
        assert len(np.unique(ps_a[j, :K])) > 1
    for k in arr_a:
        assert np.array_equal(arr_a[k], arr_b[k]), k
    eng.close()
