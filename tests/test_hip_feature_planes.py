"""
GPU tests of the batched NN input feature planes (ipp_feature_planes, IPPEngine.feature_planes, VecIPPEnv(feature_history=H)):
  * the reference's planes (tests/golden/planes.npz) from fixture states written into a dense engine, every spec;
  * factor engines (exact, band-tile window, patch): current-state entries equal ipp_state_plane, prefix entries (rank r_{t-k})
    equal the plane of a snapshot forked at step t-k;
  * tree paths equal the plane of an env slot stepped through the same actions;
  * VecIPPEnv budget-mode histories equal planes from entries rebuilt out of host bookkeeping, across done-resets, parts = 1 and 2;
  * factor, patch and tree states against fp64 directly: the dense Kalman chain of oracle/ipp_oracle.py replayed next to the device
    (tests/test_feature_planes_host.py: oracle_history, pick_threshold), current, prefix, rank-0 and tree-path entries, every prior
    kind, position mode with the cost plane and FoV mode, mask_mean and mask_env, interval_factor = 0.5;
  * edges: the largest plane kept in LDS (110 cells), the flat branch (lo == hi), refused specs on a non-square grid.
"""
import numpy as np
import pytest

from tests.test_feature_planes_host import (DIM, HISTORY_CASES, KF, START, TREE_CASES, UAV, case_names, check_margin, dense_edge_case,
                                            golden_case, history_case, ref_planes, request_scores, tree_case)

pytestmark = pytest.mark.gpu

GOLDEN = "tests/golden/planes.npz"


def host(t):
    return t.detach().cpu().numpy()


def _spec(fov, costs, adaptive, H=3):
    from ipp_rl_amd.feature_planes import PlaneSpec

    return PlaneSpec(H, use_fov=bool(fov), use_costs=bool(costs), adaptive=bool(adaptive), use_flight_time=True,
                     min_altitude=0.0 if fov else 8.0, max_altitude=0.0 if fov else 14.0)


def test_dense_fixture_states_match_reference():
    import os

    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), GOLDEN))
    S, D = g["states"], g["descent_states"]
    eng = IPPEngine(EngineConfig(x_dim=DIM, y_dim=DIM), capacity=len(S) + len(D), state="dense", device="cuda:0")
    eng.set_uav(float(g["max_v"]), float(g["max_a"]))
    for k, st in enumerate(list(S) + list(D)):
        eng.write_cov(k, st)
    uav = {"max_v": float(g["max_v"]), "max_a": float(g["max_a"])}
    mean = g["mean"].ravel().astype(np.float32)
    H = int(g["history"])
    seen_nan = False
    for name in case_names(g):
        Sx, Px, Bx, kw = golden_case(g, name)
        off = len(S) if g[f"{name}_descent"] else 0
        recs = pack_entries([[make_entry(off + int(i), p, b) for i, p, b in zip(g[f"{name}_idx"], Px, Bx)]], H)
        spec = _spec(g[f"{name}_fov"], g[f"{name}_costs"], g[f"{name}_adaptive"], H)
        eng.set_adaptive(float(g[f"{name}_thr"]), float(g[f"{name}_kf"]))
        got = host(eng.feature_planes(recs, spec, mask_mean=mean[None]))[0].astype(np.float64)
        want = ref_planes(Sx, Px, Bx, H, DIM, DIM, uav=uav, **kw)
        assert got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, equal_nan=True, err_msg=name)
        if f"{name}_planes" in g.files:
            np.testing.assert_allclose(got, g[f"{name}_planes"], rtol=0, atol=1e-5, equal_nan=True, err_msg=name)
        seen_nan |= bool(np.isnan(got).any())
    assert seen_nan
    eng.close()


# 10 x 10: the plane stays in LDS between the passes; 11 x 11 and up: densified again (the 64 KB of LDS include the static tiles)
ENGINES = [("exact10", 10, 0, False), ("exact11", 11, 0, False), ("exact", 20, 0, False), ("band", 20, 12, False),
           ("patch", 40, -1, True)]


def _factor_engine(dim, window_rows, fixed, capacity, node_capacity=0, nu=1.5):
    from ipp_rl_amd import EngineConfig, IPPEngine

    eng = IPPEngine(EngineConfig(x_dim=dim, y_dim=dim, nu=nu), capacity=capacity, state="factor", rank_cap=96, window_rows=window_rows,
                    fixed_prior=fixed, score_scratch=True, node_capacity=node_capacity, max_batch=64, device="cuda:0")
    return eng


def _actions(rs, dim, n):
    c = np.clip(dim // 2 + rs.randint(-4, 5, size=(n, 2)), 0, dim - 1)
    return np.stack([4.0 * c[:, 0] + 2.0, 4.0 * c[:, 1] + 2.0, rs.choice([8.0, 9.0, 14.0], size=n)], axis=1)


@pytest.mark.parametrize("layout,dim,window_rows,fixed", ENGINES)
def test_factor_current_and_prefix_entries(layout, dim, window_rows, fixed):
    import torch

    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    K = 4
    B = 2  # slots 0, 1 step; slots 2 .. 2 + 2K - 1 hold the snapshots of steps 0 .. K - 1
    eng = _factor_engine(dim, window_rows, fixed, B + B * K)
    assert int(eng.info.patch_layout) == (1 if layout == "patch" else 0)
    eng.set_adaptive(0.45, 0.05)
    rs = np.random.RandomState(3)
    eng.reset(env_ids=list(range(B)), white_noise=rs.normal(size=(B, dim, dim)))
    prev = np.tile([2.0, 2.0, 14.0], (B, 1))
    ranks = []
    for t in range(K):
        eng.fork(list(range(B)), [B + B * t + b for b in range(B)])
        ranks.append(host(eng.ranks())[:B].copy())
        a = _actions(rs, dim, B)
        eng.step(a, prev, env_ids=list(range(B)), meas_noise=rs.normal(size=(B, 9)))
        prev = a
    torch.cuda.synchronize()
    mean = host(eng.read_mean(0)).astype(np.float32)
    spec = _spec(0, 0, 1, H=K + 1)
    hist = [[make_entry(b, prev[b], 1.0)] + [make_entry(b, [4.0, 4.0, 8.0], 0.5, rank=int(ranks[t][b])) for t in range(K - 1, -1, -1)]
            for b in range(B)]
    got = host(eng.feature_planes(pack_entries(hist, K + 1), spec, mask_mean=np.tile(mean, (B, 1))))
    for b in range(B):
        want = host(eng.state_plane(b, mean_for_mask=mean))
        np.testing.assert_allclose(got[b, 0], want, rtol=0, atol=1e-6, err_msg=f"{layout} current {b}")
        for j, t in enumerate(range(K - 1, -1, -1)):
            want = host(eng.state_plane(B + B * t + b, mean_for_mask=mean))
            np.testing.assert_allclose(got[b, 5 * (j + 1)], want, rtol=0, atol=1e-6, err_msg=f"{layout} prefix t={t} env {b}")
            assert np.all(got[b, 5 * (j + 1) + 4] == np.float32(0.5))
    # bad entries are loud: a rank above the slot's and a slot outside the engine give NaN planes, never another state
    bad = pack_entries([[make_entry(0, prev[0], 1.0, rank=int(ranks[-1][0]) + 10_000)], [make_entry(10_000, prev[0], 1.0)]], 1)
    out = host(eng.feature_planes(bad, _spec(0, 0, 1, H=1), mask_mean=np.tile(mean, (2, 1))))
    assert np.isnan(out).all()
    eng.close()


@pytest.mark.parametrize("dim,window_rows,fixed", [(20, 12, False), (40, -1, True)])
def test_tree_path_entries_equal_stepped_slot(dim, window_rows, fixed):
    import torch

    from ipp_rl_amd.feature_planes import TREE_DEPTH, make_entry, pack_entries

    eng = _factor_engine(dim, window_rows, fixed, capacity=3, node_capacity=16)
    eng.set_adaptive(0.45, 0.05)  # (interval_factor > 0: the mask reads each node's own diagonal)
    rs = np.random.RandomState(7)
    eng.reset(env_ids=[0], white_noise=rs.normal(size=(1, dim, dim)))
    prev = np.array([2.0, 2.0, 14.0])
    for _ in range(3):
        a = _actions(rs, dim, 1)[0]
        eng.step(a[None], prev[None], env_ids=[0], meas_noise=rs.normal(size=(1, 9)))
        prev = a
    eng.fork([0, 0], [1, 2])
    acts = _actions(rs, dim, 3)
    path, p = [], prev
    for d in range(3):  # nodes 0, 1, 2: a chain below env 0; slot 1 takes all three steps, slot 2 the first two
        eng.tree_step([0], [path + [-1] * (TREE_DEPTH - len(path))], acts[d][None], p[None], new_ids=[d])
        eng.step(acts[d][None], p[None], env_ids=[1], cov_only=True)
        if d < 2:
            eng.step(acts[d][None], p[None], env_ids=[2], cov_only=True)
        path.append(d)
        p = acts[d]
    torch.cuda.synchronize()
    mean = host(eng.read_mean(0)).astype(np.float32)
    recs = pack_entries([[make_entry(0, acts[2], 0.3, path=[0, 1, 2]), make_entry(0, acts[1], 0.6, path=[0, 1]), make_entry(0, prev, 1.0)]], 3)
    got = host(eng.feature_planes(recs, _spec(0, 1, 1), mask_mean=mean[None]))[0]
    for ch, slot in ((0, 1), (5, 2)):  # (tree nodes from the tree-step kernels, the slots from the env-step kernels)
        want = host(eng.state_plane(slot, mean_for_mask=mean))
        err = float(np.max(np.abs(got[ch] - want)))
        print(f"tree entry {ch // 5} vs stepped slot {slot} ({dim} x {dim}): max |diff| = {err:.3g}")
        np.testing.assert_allclose(got[ch], want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[10], host(eng.state_plane(0, mean_for_mask=mean)), rtol=0, atol=1e-6)
    eng.close()


@pytest.mark.parametrize("parts", [1, 2])
def test_vec_env_history_matches_host_bookkeeping(parts):
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.feature_planes import entry_records, make_entry, pack_entries
    from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions

    cfg = EngineConfig(x_dim=50, y_dim=50)
    B, H, B0 = 4096, 3, 60.0
    env = VecIPPEnv(cfg, B, episode_steps=40, window_rows=-1, seed=13, budget=B0, shuffle_budget=True, parts=parts, feature_history=H)
    env.reset()
    sample = np.array([1, 1000, 2048, B - 1])  # (a 50 x 50 plane is 10 MB: a few envs of every phase / part)
    hist = {int(e): [] for e in sample}  # host bookkeeping: (rank, prev, budget / B0) of the pre-step states of the current episode
    spec = _spec(1, 0, 1, H)
    resets = 0
    for t in range(14):
        torch.cuda.synchronize()
        rk, pv, bd, ep = host(env.engine.ranks())[:B], host(env.prev), host(env.budget), host(env.episode)
        want = pack_entries([[make_entry(e, pv[e], bd[e] / B0)] +
                             [make_entry(e, p, b, rank=r) for r, p, b in hist[int(e)][::-1][:H - 1]] for e in sample], H)
        got = entry_records(env.history_entries(sample))
        # (budget / B0: torch's device fp64 division may differ from NumPy's in the last bit)
        np.testing.assert_allclose(got["budget"], want["budget"], rtol=1e-15, atol=0, err_msg=f"step {t}")
        want["budget"] = got["budget"]
        diff = [(int(e), k, got[i, k], want[i, k]) for i, e in enumerate(sample) for k in range(H)
                if got[i, k].tobytes() != want[i, k].tobytes()]
        assert not diff, f"step {t}: {diff[:3]}"
        planes = env.feature_planes(spec, env_ids=sample)
        ref = env.engine.feature_planes(want, spec, mask_env=sample)
        assert torch.equal(torch.nan_to_num(planes, nan=-7.0), torch.nan_to_num(ref, nan=-7.0)), f"step {t}"
        for i, e in enumerate(sample):
            n_valid = 1 + min(len(hist[int(e)]), H - 1)
            assert not bool(planes[i, 3 * n_valid:].any())  # older entries of a reset history are zero planes
            assert bool(torch.isfinite(planes[i, :3 * n_valid]).all())
        del planes, ref
        for e in sample:
            hist[int(e)].append((int(rk[e]), pv[e].copy(), float(bd[e] / B0)))
        env.step(cell_centre_actions(cfg, t, 0, B, B, [8.0, 14.0]))
        torch.cuda.synchronize()
        ep2 = host(env.episode)
        for e in sample:
            if ep2[e] != ep[e]:
                hist[int(e)] = []
                resets += 1
    assert resets > 0  # envs finished at different steps inside the run
    env.close()


# ----------------------------------------------------------------------------- factor, patch and tree states against fp64
STATE_TOL = 1e-5       # the project's parity bar
ROUND_TOL = 2.0 ** -23  # fp64 arithmetic rounded once to fp32 on values in [0, 1] (2^-25), with room for the last bit of a sqrt


def _compare(got, want, per, H, tag):
    """One request's planes against ref_planes, by plane type; returns the largest state-plane error."""
    assert got.shape == want.shape, tag
    worst = 0.0
    for ch in range(want.shape[0]):
        if ch == per * H:  # the cost plane
            err = float(np.max(np.abs(got[ch] - want[ch])))
            assert err <= ROUND_TOL, f"{tag}: cost plane off by {err:.3g}"
        elif ch % per == 0:
            err = float(np.max(np.abs(got[ch] - want[ch])))
            worst = max(worst, err)
            assert err <= STATE_TOL, f"{tag}: state plane of entry {ch // per} off by {err:.3g}"
        else:  # position / FoV / budget planes: np.float32 of the fp64 value
            assert np.array_equal(got[ch], want[ch].astype(np.float32)), f"{tag}: plane {ch}"
    return worst


def _request_vs_fp64(eng, req, dim, mask_mean, oracle_mean, tag):
    """Position mode with the cost plane and FoV mode, each with mask_mean and with mask_env (slot 0's device mean; the reference
    takes the oracle's), interval_factor = KF and the threshold picked for the request.  Returns the largest state-plane error."""
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    H = len(req.states)
    recs = pack_entries([[make_entry(0, p, b, rank=r, path=path) for p, b, r, path in zip(req.positions, req.budgets, req.ranks, req.paths)]], H)
    worst = 0.0
    for label, mean, kw in (("mask_mean", mask_mean, dict(mask_mean=mask_mean[None])), ("mask_env", oracle_mean, dict(mask_env=[0]))):
        thr, _ = check_margin(req.states, mean, f"{tag} {label}")
        eng.set_adaptive(thr, KF)
        for fov in (0, 1):
            got = host(eng.feature_planes(recs, _spec(fov, 1 - fov, 1, H), **kw))[0]
            want = ref_planes(req.states, req.positions, req.budgets, H, dim, dim, fov=bool(fov), costs=not fov, mean=mean, thr=thr, kf=KF,
                              uav=UAV)
            worst = max(worst, _compare(got, want, 3 if fov else 5, H, f"{tag} {label} fov={fov}"))
            del got, want
    return worst


def _replay(eng, w, h, steps):
    """`steps` env steps of walk `w` on slot 0; the ranks before every step and after the last equal the oracle's, and the slot's mean
    and diagonal are within the parity bar of fp64 (what check_margin's margin presumes)."""
    eng.reset(env_ids=[0], white_noise=w.white[None])
    prev, ranks = START, []
    for a, eps in zip(w.actions[:steps], w.eps[:steps]):
        ranks.append(int(host(eng.ranks())[0]))
        _, status = eng.step(a[None], prev[None], env_ids=[0], meas_noise=eps[None])
        assert int(status[0]) == 0
        prev = a
    ranks.append(int(host(eng.ranks())[0]))
    assert ranks == h.ranks
    assert np.max(np.abs(host(eng.read_mean(0)).ravel() - h.st.mean.ravel())) < STATE_TOL
    assert np.max(np.abs(host(eng.read_diag(0)).ravel() - np.diag(h.st.P))) < STATE_TOL
    return ranks


def _history_vs_fp64(name, window_rows, fixed, patch):
    dim, nu, _ = HISTORY_CASES[name]
    w, h, req = history_case(name)
    eng = _factor_engine(dim, window_rows, fixed, capacity=1, nu=nu)
    assert int(eng.info.patch_layout) == patch
    ranks = _replay(eng, w, h, len(w.actions))
    for edge in (32, 64):  # the chunks of the kernel's column loop: states on both sides of either edge, none on it
        assert min(ranks) < edge < max(ranks) and edge not in ranks
    assert [r for r in req.ranks[1:]] == [ranks[6], ranks[3], ranks[1], 0]
    worst = _request_vs_fp64(eng, req, dim, w.mask_mean, h.st.mean.ravel(), name)
    print(f"{name} ({dim} x {dim}, nu = {nu}): ranks {ranks}, largest state-plane error {worst:.3g}")
    eng.close()


@pytest.mark.parametrize("layout,dim,window_rows,fixed", ENGINES)
def test_history_entries_match_fp64(layout, dim, window_rows, fixed):
    """Current state, column prefixes and the bare prior of a slot stepped 8 times, against the dense fp64 chain."""
    assert HISTORY_CASES[layout][0] == dim
    _history_vs_fp64(layout, window_rows, fixed, 1 if layout == "patch" else 0)


@pytest.mark.parametrize("tag", ["nu0.5", "nu2.5", "nuinf"])
@pytest.mark.parametrize("layout,window_rows,fixed", [("exact11", 0, False), ("patch", -1, True)])
def test_history_entries_match_fp64_every_prior(layout, window_rows, fixed, tag):
    """The same with the priors of nu = 0.5, 2.5 and inf: the oracle starts from the closed form of that nu, and the rank-0
    entry is that prior's normalised masked plane.  The patch grid is 40 x 40 where the kind's window allows it (nu = 2.5, inf),
    else the smallest that has the patch layout (42 x 42 for the 14 rows of nu = 0.5: a 40 x 40 engine falls back to band tiles)."""
    name = f"{layout}-{tag}"
    dim, nu, _ = HISTORY_CASES[name]
    if layout == "patch" and dim != 40:
        small = _factor_engine(40, window_rows, fixed, capacity=1, nu=nu)
        assert int(small.info.patch_layout) == 0
        small.close()
    _history_vs_fp64(name, window_rows, fixed, 1 if layout == "patch" else 0)


@pytest.mark.parametrize("name,window_rows,fixed", [("band", 12, False), ("patch", -1, True)])
def test_tree_paths_match_fp64(name, window_rows, fixed):
    """Paths of depth 6 (every s.off / s.ids slot), 3 and 1, a sibling branching at depth 2 and the root, each node's covariance
    from predict_step.  The footprints of the path's nodes overlap (asserted on the CPU), so the mask's diagonal must come from
    the deepest node that holds a cell."""
    from ipp_rl_amd.feature_planes import TREE_DEPTH

    dim, nu, _ = TREE_CASES[name]
    w, h, req = tree_case(name)
    eng = _factor_engine(dim, window_rows, fixed, capacity=1, node_capacity=16, nu=nu)
    assert int(eng.info.patch_layout) == (1 if name == "patch" else 0)
    _replay(eng, w, h, len(h.P) - 1)
    paths = {None: []}
    for nid, parent, a in w.tree:
        path = paths[parent]
        _, status = eng.tree_step([0], [path + [-1] * (TREE_DEPTH - len(path))], a[None], START[None], new_ids=[nid])
        assert int(status[0]) == 0
        paths[nid] = path + [nid]
    assert [paths[p[-1]] if p else [] for p in req.paths] == req.paths and len(req.paths[0]) == TREE_DEPTH
    worst = _request_vs_fp64(eng, req, dim, w.mask_mean, h.st.mean.ravel(), f"tree {name}")
    print(f"tree {name} ({dim} x {dim}): largest state-plane error {worst:.3g}")
    eng.close()


# ----------------------------------------------------------------------------- edges
@pytest.mark.parametrize("W,Hg", [(10, 11), (11, 10)])
def test_largest_cached_plane_and_refused_specs(W, Hg):
    """110 cells: the largest plane that stays in LDS between the passes (65 248 of 65 536 bytes), on a dense engine written with
    write_cov.  The grid is not square, so position mode without costs; FoV and cost specs are refused before any launch.
    There is no factor-engine twin of this case: reset(white_noise=...) refuses a non-square grid (the device GRF needs a
    square one), which is asserted here."""
    import torch

    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd._ffi import IppError
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    mats, mean = dense_edge_case()
    N, H = W * Hg, 3
    eng = IPPEngine(EngineConfig(x_dim=W, y_dim=Hg), capacity=len(mats), state="dense", device="cuda:0")
    for k, P in enumerate(mats):
        eng.write_cov(k, P)
    thr, _ = check_margin(mats, mean, "dense edge")
    eng.set_adaptive(thr, KF)
    positions, budgets = [np.array([14.0, 22.0, 9.0]), np.array([26.0, 6.0, 12.0])], [0.8, 0.3]
    recs = pack_entries([[make_entry(k, positions[k], budgets[k]) for k in range(len(mats))]], H)  # (one padding entry)
    got = host(eng.feature_planes(recs, _spec(0, 0, 1, H), mask_mean=mean[None]))[0]
    want = ref_planes(mats, positions, budgets, H, W, Hg, fov=False, costs=False, mean=mean, thr=thr, kf=KF)
    assert got.shape == want.shape == (5 * H, N, N)
    for ch in range(5 * H):
        if ch % 5 == 0:  # the device holds these fp32 matrices exactly and normalises in fp64: one rounding
            assert np.max(np.abs(got[ch] - want[ch])) <= ROUND_TOL, ch
        else:
            assert np.array_equal(got[ch], want[ch].astype(np.float32)), ch
    assert 0.0 < want[0].max() and not want[10:].any()
    for fov, costs in ((1, 0), (0, 1)):
        spec = _spec(fov, costs, 1, H)
        out = torch.full((1, spec.channels, N, N), -7.0, dtype=torch.float32, device="cuda:0")
        with pytest.raises(IppError, match=rf"ipp engine error -1: FoV and cost planes need a square grid \(cell x_dim \* x \+ y\), got {W} x {Hg}"):
            eng.feature_planes(recs, spec, mask_mean=mean[None], out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())  # nothing was launched
    eng.close()
    fac = IPPEngine(EngineConfig(x_dim=W, y_dim=Hg), capacity=1, state="factor", rank_cap=96, score_scratch=True, device="cuda:0")
    with pytest.raises(IppError, match="device GRF needs a square grid"):
        fac.reset(env_ids=[0], white_noise=np.zeros((1, Hg, W)))
    fac.close()


@pytest.mark.parametrize("layout,window_rows,fixed", [("exact10", 0, False), ("band", 12, False)])
def test_flat_planes_of_an_empty_mask(layout, window_rows, fixed):
    """lo == hi on a factor engine: a threshold above every score empties the mask, the plane is 0 / 0 = NaN exactly where the
    reference's is, with the plane kept in LDS (10 x 10) and densified twice (20 x 20)."""
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    dim, nu, _ = HISTORY_CASES[layout]
    w, h, req = history_case(layout)
    eng = _factor_engine(dim, window_rows, fixed, capacity=1, nu=nu)
    _replay(eng, w, h, len(w.actions))
    H = len(req.states)
    thr = max(float(s.max()) for s in request_scores(req.states, w.mask_mean)) + 1.0
    eng.set_adaptive(thr, KF)
    recs = pack_entries([[make_entry(0, p, b, rank=r) for p, b, r in zip(req.positions, req.budgets, req.ranks)]], H)
    got = host(eng.feature_planes(recs, _spec(0, 1, 1, H), mask_mean=w.mask_mean[None]))[0]
    want = ref_planes(req.states, req.positions, req.budgets, H, dim, dim, fov=False, costs=True, mean=w.mask_mean, thr=thr, kf=KF, uav=UAV)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want[0::5][:H]).all() and not np.isnan(want[1]).any()
    keep = ~np.isnan(want)
    assert np.max(np.abs(got[keep] - want[keep])) <= ROUND_TOL
    eng.close()


def test_flat_plane_of_a_constant_matrix():
    """lo == hi without a mask: a dense slot that holds one value everywhere gives x / hi = 1."""
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.feature_planes import make_entry, pack_entries

    eng = IPPEngine(EngineConfig(x_dim=DIM, y_dim=DIM), capacity=1, state="dense", device="cuda:0")
    N = DIM * DIM
    P = np.full((N, N), np.float64(np.float32(0.37)))
    eng.write_cov(0, P)
    pos = np.array([18.0, 22.0, 9.0])
    got = host(eng.feature_planes(pack_entries([[make_entry(0, pos, 0.6)]], 1), _spec(0, 0, 0, 1)))[0]
    want = ref_planes([P], [pos], [0.6], 1, DIM, DIM, fov=False, costs=False)
    assert np.array_equal(want[0], np.ones((N, N))) and np.array_equal(got[0], np.ones((N, N), dtype=np.float32))
    assert np.array_equal(got, want.astype(np.float32))
    eng.close()
