"""
CPU checks of the batched feature planes (ipp_feature_planes): the entry record and its packing, the channel layout of every
spec, rejected specs and arguments, and a NumPy restatement of generate_input_feature_planes (planning/common/features.py:83-151)
against the reference's outputs recorded in tests/golden/planes.npz (gen_plane_golden.py) at 1e-12.  The restatement is the
definition the device kernel is tested against in tests/test_hip_feature_planes.py.

The second half builds the fp64 states those device tests compare with: seeded walks replayed through the dense Kalman chain of
oracle/ipp_oracle.py (oracle_history), the requests made of them, and the mask threshold of each request (pick_threshold), whose
margin is checked here for every case so that no cell's mask can differ on the device.
"""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import ipp_oracle as orc
from tests.test_prior_kernels_host import prior_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planes.npz")
RES, DIM = 4.0, 10
TAN = math.tan(0.5 * math.radians(60.0))


# ----------------------------------------------------------------------------- NumPy restatement
def min_max_normalize(x):
    lo, hi = np.min(x), np.max(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / hi if lo == hi else (x - lo) / (hi - lo)


def footprint(pos, W, H, res=RES, tanx=TAN, tany=TAN):
    """sensors/cameras.py:49-75: (xl, xr, yu, yd)."""
    cx, cy = np.floor(2 * pos[2] * tanx / res), np.floor(2 * pos[2] * tany / res)
    gx, gy = np.floor(pos[0] / res), np.floor(pos[1] / res)
    rx, ry = np.floor(0.5 * cx), np.floor(0.5 * cy)
    return (int(np.clip(gx - rx, 0, W - 1)), int(np.clip(gx + rx, 0, W - 1)), int(np.clip(gy - ry, 0, H - 1)), int(np.clip(gy + ry, 0, H - 1)))


def fov_plane(pos, W, H):
    xl, xr, yu, yd = footprint(pos, W, H)
    sel = np.zeros(W * H, dtype=bool)
    for x in range(xl, xr):
        for y in range(yu, yd):
            sel[W * x + y] = True  # flatten_grid_index of (x, y): x_dim * x + y
    return np.outer(sel, sel).astype(np.float64)


def cost_plane(pos0, W, H, min_alt, uav=None, res=RES):
    n = W * H
    costs = np.zeros(n)
    for x in range(W):
        for y in range(H):
            d = np.array([x * res + 0.5 * res, y * res + 0.5 * res, min_alt]) - np.array([pos0[0], pos0[1], min_alt])
            dist = np.sqrt(np.sum(d * d))
            if uav is None:
                costs[W * x + y] = dist
            else:
                d_acc = min(dist * 0.5, uav["max_v"] ** 2 / (2 * uav["max_a"]))
                costs[W * x + y] = (dist - 2 * d_acc) / uav["max_v"] + 2 * np.sqrt(2 * d_acc / uav["max_a"])
    return min_max_normalize(np.repeat(costs[:, None], n, axis=1))


def state_plane(state, mean=None, thr=None, kf=None):
    s = np.array(state, dtype=np.float64, copy=True)
    if mean is not None:
        m = np.asarray(mean).ravel() + kf * np.diag(s) >= thr
        s[~m, :] = 0
        s[:, ~m] = 0
    return min_max_normalize(s)


def ref_planes(states, positions, budgets, H, W, Hg, *, fov, costs, mean=None, thr=None, kf=None, min_alt=8.0, max_alt=14.0, uav=None):
    """generate_input_feature_planes on copies: states / positions / budgets newest first (len <= H)."""
    n = W * Hg
    out = []
    for s, p, b in zip(states, positions, budgets):
        sp = state_plane(s, mean, thr, kf)
        if fov:
            out += [sp, fov_plane(p, W, Hg), b * np.ones((n, n))]
        else:
            out += [sp, p[0] / (W * RES) * np.ones((n, n)), p[1] / (W * RES) * np.ones((n, n)),
                    (p[2] - min_alt) / (max_alt - min_alt) * np.ones((n, n)), b * np.ones((n, n))]
    out += [np.zeros((n, n))] * ((3 if fov else 5) * (H - len(states)))
    if costs and not fov:
        out.append(cost_plane(positions[0], W, Hg, min_alt, uav))
    return np.array(out)


def golden_case(g, name):
    """The inputs of one recorded case (newest first) and its spec."""
    desc = bool(g[f"{name}_descent"])
    idx = g[f"{name}_idx"]
    S = g["descent_states"] if desc else g["states"]
    P = g["descent_positions"] if desc else g["positions"]
    B = g["descent_budgets"] if desc else g["budgets"]
    kw = dict(fov=bool(g[f"{name}_fov"]), costs=bool(g[f"{name}_costs"]))
    if g[f"{name}_adaptive"]:
        kw.update(mean=g["mean"].ravel(), thr=float(g[f"{name}_thr"]), kf=float(g[f"{name}_kf"]))
    return [S[i] for i in idx], [P[i] for i in idx], [B[i] for i in idx], kw


def case_names(g):
    return sorted(k[:-len("_idx")] for k in g.files if k.endswith("_idx"))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_matches_reference(golden):
    g = golden
    uav = {"max_v": float(g["max_v"]), "max_a": float(g["max_a"])}
    names = case_names(g)
    assert len(names) == 8 + 5 + 2
    for name in names:
        S, P, B, kw = golden_case(g, name)
        got = ref_planes(S, P, B, int(g["history"]), DIM, DIM, uav=uav, min_alt=float(g["min_altitude"]), max_alt=float(g["max_altitude"]), **kw)
        with np.errstate(invalid="ignore"):
            proj = got @ g["proj"]
        np.testing.assert_allclose(proj, g[f"{name}_proj"], rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
        if f"{name}_planes" in g.files:
            np.testing.assert_allclose(got.astype(np.float32), g[f"{name}_planes"], rtol=0, atol=0, equal_nan=True, err_msg=name)
    # the recorded cases cover what the device must reproduce: short histories, the empty mask, FoV sets
    assert np.isnan(g["nanmask_proj"][0]).all() and not np.isnan(g["nanmask_proj"][1:]).any()
    assert len(g["grow0_idx"]) == 1 and len(g["grow1_idx"]) == 2
    assert g["final_f1c0a1_proj"].shape[0] == 9 and g["final_f0c1a1_proj"].shape[0] == 16
    assert np.array_equal(g["final_f1c1a1_proj"], g["final_f1c0a1_proj"], equal_nan=True)  # FoV mode returns before the cost plane


# ----------------------------------------------------------------------------- spec, entries, channel layout
def test_channel_layout_of_every_spec():
    from ipp_rl_amd.feature_planes import PlaneSpec

    for H in (1, 3, 8):
        assert PlaneSpec(H, min_altitude=8, max_altitude=14).channels == 5 * H
        assert PlaneSpec(H, use_costs=True, min_altitude=8, max_altitude=14).channels == 5 * H + 1
        assert PlaneSpec(H, use_fov=True).channels == 3 * H
        assert PlaneSpec(H, use_fov=True, use_costs=True).channels == 3 * H  # FoV mode has no cost plane
    assert PlaneSpec(2, use_costs=True, min_altitude=8, max_altitude=14).channel_names() == [
        "state[0]", "x[0]", "y[0]", "z[0]", "budget[0]", "state[1]", "x[1]", "y[1]", "z[1]", "budget[1]", "cost"]
    assert PlaneSpec(1, use_fov=True).channel_names() == ["state[0]", "fov[0]", "budget[0]"]
    hp = {"input_history_length": 3, "use_fov_input": False, "use_action_costs_input": True}
    s = PlaneSpec.from_params(hp, {"min_altitude": 8, "max_altitude": 14})
    assert (s.history, s.use_fov, s.use_costs, s.min_altitude, s.max_altitude, s.channels) == (3, False, True, 8.0, 14.0, 16)
    s = PlaneSpec.from_params(dict(hp, use_fov_input=True), {"min_altitude": 8, "max_altitude": 14})
    assert s.use_fov and s.channels == 9


def test_entry_record_matches_the_c_struct():
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.feature_planes import ENTRY_DTYPE, ENTRY_WORDS, PlaneSpec

    assert ENTRY_DTYPE.itemsize == 72 and ENTRY_WORDS == 18
    assert [ENTRY_DTYPE.fields[k][1] for k in ("root_env", "rank", "path", "valid", "reserved", "position", "budget")] == [0, 4, 8, 32, 36, 40, 64]
    assert ctypes.sizeof(_ffi.IppPlaneSpec) == 6 * 4 + 2 * 8
    c = PlaneSpec(3, use_costs=True, adaptive=False, min_altitude=8, max_altitude=14).to_c()
    assert (c.history, c.use_fov, c.use_costs, c.adaptive, c.use_flight_time, c.min_altitude, c.max_altitude) == (3, 0, 1, 0, 1, 8.0, 14.0)
    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    import re

    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ipp_plane_spec \{(.*?)\} ipp_plane_spec;", txt, flags=re.S).group(1), flags=re.S)
    names = [n.strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert names == [f[0] for f in _ffi.IppPlaneSpec._fields_]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ipp_plane_entry \{(.*?)\} ipp_plane_entry;", txt, flags=re.S).group(1), flags=re.S)
    names = [re.sub(r"\[.*\]", "", n).strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert names == list(ENTRY_DTYPE.names)


def test_entry_packing():
    from ipp_rl_amd.feature_planes import ENTRY_WORDS, make_entry, pack_entries

    e = make_entry(7, [1.0, 2.0, 3.0], 0.25, rank=4, path=[3, 9, -1])
    assert (int(e["root_env"]), int(e["rank"]), int(e["valid"]), list(e["path"])) == (7, 4, 1, [3, 9, -1, -1, -1, -1])
    recs = pack_entries([[e], [e, make_entry(1, [0, 0, 8], 1.0)], []], history=3)
    assert recs.shape == (3, 3)
    assert list(recs["valid"].sum(axis=1)) == [1, 2, 0]
    assert (recs["path"][recs["valid"] == 0] == -1).all()
    words = recs.view(np.int32).reshape(3, 3, ENTRY_WORDS)
    assert words[0, 0, 0] == 7 and words[0, 0, 1] == 4 and words[0, 0, 8] == 1
    assert recs.view(np.float64).reshape(3, 3, 9)[0, 0, 5:9].tolist() == [1.0, 2.0, 3.0, 0.25]
    with pytest.raises(ValueError):
        pack_entries([[e] * 4], history=3)
    with pytest.raises(ValueError):
        make_entry(0, [0, 0, 8], 1.0, path=list(range(7)))


def test_bad_specs_raise():
    from ipp_rl_amd.feature_planes import PlaneSpec

    with pytest.raises(ValueError):
        PlaneSpec(0, use_fov=True)
    with pytest.raises(ValueError):
        PlaneSpec(65, use_fov=True)
    with pytest.raises(ValueError):
        PlaneSpec(3)  # position mode without altitudes
    with pytest.raises(ValueError):
        PlaneSpec(3, min_altitude=8, max_altitude=8)
    with pytest.raises(ValueError):
        PlaneSpec(3, min_altitude=float("nan"), max_altitude=14)


def test_c_entry_point_rejects_bad_calls_without_a_gpu():
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    spec = _ffi.IppPlaneSpec(history=3, use_fov=1)
    assert lib.ipp_feature_planes(None, ctypes.byref(spec), None, 1, None, None, None, None) == -1
    assert b"null" in lib.ipp_last_error()


def test_vec_env_feature_history_needs_budget_mode():
    from ipp_rl_amd.vec_env import VecIPPEnv

    with pytest.raises(ValueError):
        VecIPPEnv.check_feature_history(3, budget=None)
    with pytest.raises(ValueError):
        VecIPPEnv.check_feature_history(-1, budget=200.0)
    VecIPPEnv.check_feature_history(3, budget=200.0)
    VecIPPEnv.check_feature_history(0, budget=None)


# ----------------------------------------------------------------------------- fp64 states for the device comparisons
START = np.array([2.0, 2.0, 14.0])  # planning/missions.py:69
UAV = {"max_v": 2.0, "max_a": 2.0}
ALTS = (6.0, 8.0, 9.0, 12.0, 14.0)  # m = 1, 9, 9, 4, 9 measurements; rf = 2 above 10 m
# The 8-step walks take a seeded order of these: 7 x 9 + 4 columns, so the ranks pass 32 and 64 (the chunks of k_feature_planes'
# column loop) and end at 67, whatever the seed.  6 m (one measurement) is drawn in the tree and state-plane walks.
WALK_ALTS = (8.0, 8.0, 9.0, 9.0, 12.0, 14.0, 14.0, 14.0)
KF = 0.5
MARGIN = 1e-4  # the device diagonal and mean are within 1e-5 of fp64 and KF <= 1: a cell's score moves by < 2e-5
PREFIX_STEPS = (6, 3, 1)
BUDGETS = (0.9, 0.7, 0.45, 0.2, 0.05)
INF = float("inf")
# name: (dim, nu, seed).  The seeds were chosen on the CPU so that every request below has margin >= MARGIN and a mask that is
# neither empty nor full for every entry (test_reference_masks_are_nontrivial_with_margin).  The patch layout needs an even
# x_dim > 2 * window_rows + 13: 40 for the 10-row windows of nu = 1.5, 2.5 and inf, 42 for nu = 0.5 (14 rows).
HISTORY_CASES = {
    "exact10": (10, 1.5, 5), "exact11": (11, 1.5, 8), "exact": (20, 1.5, 2), "band": (20, 1.5, 2), "patch": (40, 1.5, 56),
    "exact11-nu0.5": (11, 0.5, 39), "exact11-nu2.5": (11, 2.5, 3), "exact11-nuinf": (11, INF, 8),
    "patch-nu0.5": (42, 0.5, 66), "patch-nu2.5": (40, 2.5, 11), "patch-nuinf": (40, INF, 4),
}
TREE_CASES = {"band": (20, 1.5, 1), "patch": (40, 1.5, 1)}
TREE_ENV_STEPS, TREE_CHAIN, TREE_FORK = 3, 6, 2  # nodes 0 .. 5 in a chain below the env, node 6 a second child of node 1
# ipp_state_plane (tests/test_hip_features.py): name: (dim, nu); the walk of that test (seed 21, waypoints over the whole grid)
PLANE_CASES = {"factor-0": (20, 1.5), "patch40": (40, 1.5), "factor-0-nu2.5": (20, 2.5)}


def pick_threshold(scores):
    """(thr, margin) for the reference's mean + kf * diag(P) of every entry of a request: the midpoint and half the width of the
    widest gap between consecutive sorted values inside the middle half of their range [min + (max - min) / 4, max - (max - min)
    / 4].  (Of the range, not of the rank order: after a few steps on a 40 x 40 grid three quarters of the cells still hold the
    prior variance and the initial mean, so the values between the quartiles are one point and have no gap.)"""
    v = np.sort(np.concatenate([np.ravel(x) for x in scores]))
    q = 0.25 * (v[-1] - v[0])
    w = v[(v >= v[0] + q) & (v <= v[-1] - q)]
    assert w.size >= 2, "fewer than two scores inside the middle half"
    gaps = np.diff(w)
    k = int(np.argmax(gaps))
    return float(0.5 * (w[k] + w[k + 1])), float(0.5 * gaps[k])


def oracle_history(dim, nu, white, actions, eps, tree=()):
    """Replays `actions` (with the ground truth of `white` and the measurement noise `eps`, the first m of every row) through
    the dense fp64 chain from the prior of `nu` and keeps P after every step: P[k] / ranks[k] = the state and the number of
    factor columns after k steps.  tree: (node id, parent id or None = the final env state, action) in creation order, chained
    with predict_step; nodes[id] = that node's P, fov[id] = its footprint."""
    cfg = orc.OracleConfig(x_dim=dim, y_dim=dim)
    st = orc.env_reset(cfg, white)
    if nu != 1.5:
        st.P = prior_matrix(nu, dim)
    P, ranks = [st.P], [0]
    for a, e in zip(actions, eps):
        m = orc.num_measurements(orc.project_fov(cfg, a), orc.resolution_factor(a))
        orc.env_step(cfg, st, a, e[:m])
        P.append(st.P)
        ranks.append(ranks[-1] + m)
    nodes, fov = {}, {}
    for nid, parent, a in tree:
        nodes[nid] = orc.predict_step(cfg, st.P if parent is None else nodes[parent], START, a)[1]
        fov[nid] = orc.project_fov(cfg, a)
    return SimpleNamespace(cfg=cfg, st=st, P=P, ranks=ranks, nodes=nodes, fov=fov)


def seeded_walk(dim, seed, steps=len(WALK_ALTS), alts=None, spread=None):
    """White noise, waypoints over cell centres within `spread` cells of the grid's centre (no footprint is clipped there),
    altitudes (a seeded order of WALK_ALTS, or draws from `alts`), measurement noise and an fp32 mean for the mask.  That mean
    is uniform in [0, 4): wider than KF times the prior variance (0.91), so that the scores of observed and of unobserved cells
    overlap in the middle of the range and a threshold there splits every entry, the bare prior included."""
    rs = np.random.RandomState(seed)
    white = rs.normal(size=(dim, dim))
    spread = min(4, dim // 2 - 3) if spread is None else spread
    cells = dim // 2 + rs.randint(-spread, spread + 1, size=(steps, 2))
    alt = rs.permutation(WALK_ALTS)[:steps] if alts is None else rs.choice(alts, size=steps)
    actions = np.column_stack([RES * cells[:, 0] + 0.5 * RES, RES * cells[:, 1] + 0.5 * RES, alt])
    eps = rs.normal(size=(steps, 9))
    mask_mean = rs.uniform(0, 4, size=dim * dim).astype(np.float32)
    return SimpleNamespace(white=white, actions=actions, eps=eps, mask_mean=mask_mean)


def history_case(name):
    """Section-2 request of one case: (walk, history, request); the request's entries newest first -- the current state, the
    prefixes at the ranks recorded before steps 6, 3 and 1, and rank 0 (the bare prior)."""
    dim, nu, seed = HISTORY_CASES[name]
    w = seeded_walk(dim, seed)
    h = oracle_history(dim, nu, w.white, w.actions, w.eps)
    T = len(w.actions)
    idx = [T] + list(PREFIX_STEPS) + [0]
    req = SimpleNamespace(states=[h.P[k] for k in idx], ranks=[-1] + [h.ranks[k] for k in idx[1:]], paths=[None] * len(idx),
                          positions=[w.actions[k - 1] if k else START for k in idx], budgets=list(BUDGETS))
    return w, h, req


def tree_case(name):
    """Section-3 request: 3 env steps, a chain of 6 nodes and a sibling of node 2; entries: the paths of depth 6 and 3, the
    sibling, depth 1, the root."""
    dim, nu, seed = TREE_CASES[name]
    w = seeded_walk(dim, seed, steps=TREE_ENV_STEPS + TREE_CHAIN + 1, alts=ALTS, spread=3)
    env_a, tree_a = w.actions[:TREE_ENV_STEPS], w.actions[TREE_ENV_STEPS:]
    tree = [(d, d - 1 if d else None, tree_a[d]) for d in range(TREE_CHAIN)] + [(TREE_CHAIN, TREE_FORK - 1, tree_a[TREE_CHAIN])]
    h = oracle_history(dim, nu, w.white, env_a, w.eps[:TREE_ENV_STEPS], tree)
    paths = [list(range(6)), [0, 1, 2], [0, 1, TREE_CHAIN], [0], []]
    req = SimpleNamespace(states=[h.nodes[p[-1]] if p else h.st.P for p in paths], ranks=[-1] * len(paths), paths=paths,
                          positions=[tree_a[p[-1]] if p else env_a[-1] for p in paths], budgets=list(BUDGETS))
    w.tree = tree
    return w, h, req


def plane_walk(dim, seed=21, steps=6):
    """The walk of test_state_plane_of_engine_slots_vs_oracle: waypoints over the whole grid, altitudes 5 .. 14 m."""
    rs = np.random.RandomState(seed)
    white = rs.normal(size=(dim, dim))
    actions, eps = [], []
    for _ in range(steps):
        actions.append(np.array([4.0 * rs.randint(0, dim) + 2.0, 4.0 * rs.randint(0, dim) + 2.0, float(rs.randint(5, 15))]))
        eps.append(rs.normal(size=9))
    return SimpleNamespace(white=white, actions=np.array(actions), eps=np.array(eps), other_mean=rs.uniform(0, 1, size=(dim, dim)))


def dense_edge_case(seed=5, n=110, slots=2):
    """Covariances for the largest plane k_feature_planes keeps in LDS (110 cells: 48 400 + 112 + 16 736 = 65 248 of 65 536
    bytes), exact in fp32, and an fp32 mean."""
    rs = np.random.RandomState(seed)
    mats = []
    for _ in range(slots):
        A = rs.normal(size=(n, n))
        mats.append((A @ A.T / n).astype(np.float32).astype(np.float64))
    return mats, rs.uniform(0, 1, size=n).astype(np.float32)


def request_scores(states, mean):
    return [np.asarray(mean, dtype=np.float64).ravel() + KF * np.diag(P) for P in states]


def check_margin(states, mean, what):
    """pick_threshold of a request, with the two conditions that make the device comparison total."""
    scores = request_scores(states, mean)
    thr, margin = pick_threshold(scores)
    assert margin >= MARGIN, f"{what}: margin {margin:.3g}"
    for k, sc in enumerate(scores):
        assert 0 < int((sc >= thr).sum()) < sc.size, f"{what}: entry {k} has a trivial mask"
    return thr, margin


@pytest.mark.parametrize("name", list(HISTORY_CASES))
def test_reference_masks_are_nontrivial_with_margin(name):
    w, h, req = history_case(name)
    assert h.ranks[-1] == 67 and min(h.ranks[1:]) < 32 < max(h.ranks[:-1]) < 64 < h.ranks[-1]
    assert 0 < min(req.ranks[1:4]) < 32 < max(req.ranks[1:4]) < 64 and req.ranks[4] == 0
    m1 = check_margin(req.states, w.mask_mean, f"{name} mask_mean")[1]
    m2 = check_margin(req.states, h.st.mean, f"{name} mask_env")[1]
    print(f"{name}: margins {m1:.3g} (mask_mean) {m2:.3g} (mask_env)")
    dim, nu, _ = HISTORY_CASES[name]
    if nu != 1.5:  # the rank-0 entry is the prior of this nu, and no other kind's plane is within the tolerance of it
        assert np.array_equal(req.states[-1], prior_matrix(nu, dim))
        assert np.max(np.abs(state_plane(req.states[-1]) - state_plane(prior_matrix(1.5, dim)))) > 1e-2


@pytest.mark.parametrize("name", list(TREE_CASES))
def test_reference_tree_masks_are_nontrivial_with_margin(name):
    w, h, req = tree_case(name)
    check_margin(req.states, w.mask_mean, f"{name} tree mask_mean")
    check_margin(req.states, h.st.mean, f"{name} tree mask_env")
    # plane_diag looks a cell up in the deepest node of the path that holds it: two nodes of the deepest path share cells
    def cells(f):
        return {(x, y) for x in range(f[0], f[1] + 1) for y in range(f[2], f[3] + 1)}
    assert any(cells(h.fov[a]) & cells(h.fov[b]) for a in range(TREE_CHAIN) for b in range(a))
    alts = set(w.actions[TREE_ENV_STEPS:, 2])
    assert 6.0 in alts and alts & {12.0, 14.0} and alts & {8.0, 9.0}  # m = 1, rf = 2 and rf = 1 among the tree's steps


@pytest.mark.parametrize("name", list(PLANE_CASES))
def test_reference_state_plane_masks_are_nontrivial_with_margin(name):
    dim, nu = PLANE_CASES[name]
    w = plane_walk(dim)
    h = oracle_history(dim, nu, w.white, w.actions, w.eps)
    check_margin([h.st.P], h.st.mean, f"{name} own mean")
    check_margin([h.st.P], w.other_mean, f"{name} other mean")


def test_reference_dense_edge_masks_are_nontrivial_with_margin():
    mats, mean = dense_edge_case()
    check_margin(mats, mean, "dense 10 x 11")


def test_pick_threshold():
    thr, margin = pick_threshold([np.array([0.0, 0.3, 0.35, 0.6, 1.0]), np.array([0.3, 0.7])])
    assert (thr, margin) == pytest.approx((0.475, 0.125), abs=1e-15)  # [0.25, 0.75] holds 0.3, 0.3, 0.35, 0.6, 0.7
