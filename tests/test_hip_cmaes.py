"""
GPU tests of the batched CMA-ES planner: the strategy kernels on bare buffers (ipp_cma_init / _ask / _tell, csrc/k_cmaes.h), the
trajectory objective (ipp_cma_plan / _objective around fork + covariance-only steps) and VecCmaesPolicy (planning/vec_cmaes.py),
against the fp64 NumPy restatements of planning/vec_cmaes.py (tests/test_cmaes_host.py pins those), the values recorded from the
reference's simulate_trajectory (tests/golden/cmaes.npz) and the fp64 oracle's prediction steps.

The eigenbasis of a covariance with (nearly) equal eigenvalues is not unique -- C = I after ipp_cma_init, and N - mu - 1 equal
eigenvalues after the first update -- and the candidates B (D (.) z) depend on it.  So the arithmetic of a tell is compared with the
host's from the SAME (B, D), the device's, and the device's eigendecomposition is checked by its invariants.
"""
import numpy as np
import pytest

from oracle import ipp_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = 1e-5  # the per-reward bar of tests/test_hip_vec_greedy.py
UAV = {"max_v": 2.0, "max_a": 2.0}
NMAX = 48
SCALE = np.tile([2.0, 2.0, 0.5], NMAX // 3)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def random_states(rs, dims):
    """Per env a generic strategy state: a random SPD C of condition number < 10 with B, D from its eigh."""
    out = []
    for N in dims:
        if N == 0:
            out.append(None)
            continue
        Q, _ = np.linalg.qr(rs.normal(size=(N, N)))
        C = Q @ np.diag(rs.uniform(1.0, 9.0, N)) @ Q.T
        C = 0.5 * (C + C.T)
        assert np.linalg.cond(C) < 10
        w, V = np.linalg.eigh(C)
        out.append(dict(m=rs.uniform(5, 30, N), sigma=float(rs.uniform(0.5, 2.0)), C=C, B=V, D=np.sqrt(w), p_sigma=0.3 * rs.normal(size=N),
                        p_c=0.3 * rs.normal(size=N), generation=int(rs.randint(0, 6)), best_x=np.zeros(N), best_f=np.inf, status=0))
    return out


def upload(torch, dev, states, dims, nmax=NMAX):
    from ipp_rl_amd.planning.vec_cmaes import CmaState

    n = len(dims)
    st = CmaState(torch, dev, n, nmax)
    st.init(torch.as_tensor(np.asarray(dims, dtype=np.int32), device=dev), torch.zeros((n, nmax), dtype=torch.float64, device=dev))

    def put(view, arr):
        view.copy_(torch.as_tensor(np.asarray(arr), dtype=view.dtype, device=dev))

    for e, s in enumerate(states):
        if s is None:
            continue
        N = s["m"].size
        put(st.m[e, :N], s["m"]); put(st.D[e, :N], s["D"]); put(st.p_sigma[e, :N], s["p_sigma"]); put(st.p_c[e, :N], s["p_c"])
        put(st.C[e, :N, :N], s["C"]); put(st.B[e, :N, :N], s["B"])
        st.sigma[e] = s["sigma"]
        st.generation[e] = s["generation"]
    return st


def device_state(st, e, N):
    return dict(m=host(st.m[e, :N]), sigma=float(st.sigma[e]), C=host(st.C[e, :N, :N]), B=host(st.B[e, :N, :N]), D=host(st.D[e, :N]),
                p_sigma=host(st.p_sigma[e, :N]), p_c=host(st.p_c[e, :N]), generation=int(st.generation[e]), best_x=host(st.best_x[e, :N]),
                best_f=float(st.best_f[e]), status=int(st.status[e]))


def close(got, want, rel):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got) - want))) <= rel * max(float(np.max(np.abs(want))), 1e-300)


def eig_quality(B, D, C):
    N = len(D)
    return (float(np.max(np.abs(B.T @ B - np.eye(N)))), float(np.max(np.abs(B @ np.diag(D * D) @ B.T - C)) / np.max(np.abs(C))))


@pytest.fixture(scope="module")
def small_engine():
    from ipp_rl_amd import EngineConfig, IPPEngine

    eng = IPPEngine(EngineConfig(x_dim=10, y_dim=10), capacity=2, state="factor", rank_cap=32, max_batch=8)
    yield eng
    eng.close()


@pytest.mark.parametrize("dims,lam", [((0, 3, 9, 30, 48), 12), ((0, 3, 9, 30, 48), 4), ((0, 3, 9, 30, 48), 13), ((48,) * 5, 64)])
def test_ask_and_tell_on_bare_buffers(small_engine, dims, lam):
    """One generation against the host functions fed the device's own normals; X, m, sigma, p_sigma, p_c, C within 1e-11 max|expected|
    (two orders above Nmax lam 2^-53 = 3.4e-13, the reordering error of the longest sum).  The eigendecomposition by its invariants,
    bounded by 100 x what numpy.linalg.eigh leaves on the same matrices.  Measured on an MI355X, worst over the four cases:
    |B^T B - I| 1.18e-14 (eigh on the same matrices: 1.3e-15 .. 2.4e-15), |B D^2 B^T - C| / |C| 1.68e-14 (eigh: 0.9e-15 .. 1.9e-15),
    both at N = 48; at N = 3 and 9 the two routines are level (2e-15 and below)."""
    import torch
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning.vec_cmaes import cma_ask_host, cma_tell_host

    eng = small_engine
    dev = eng.device
    n = len(dims)
    rs = np.random.RandomState(100 + lam)
    states = random_states(rs, dims)
    st = upload(torch, dev, states, dims)
    before = st.buf.clone()
    scale = torch.as_tensor(SCALE, dtype=torch.float64, device=dev)
    Z = torch.zeros((n, lam, NMAX), dtype=torch.float32, device=dev)
    eng.normal_rows(Z.view(n, lam * NMAX), lam * NMAX, 77, _ffi.IPP_CMA_STREAM + lam, row_offset=1000)
    assert float(Z.abs().max()) > 1 and abs(float(Z.mean())) < 0.1
    X = torch.full((n, lam, NMAX), 7.0, dtype=torch.float64, device=dev)
    st.ask(Z, scale, X)
    Zh, Xh = host(Z), host(X)
    targets = [rs.uniform(5, 30, N) for N in dims]
    f = torch.zeros((n, lam), dtype=torch.float64, device=dev)
    for e, N in enumerate(dims):
        if N == 0:
            assert np.all(Xh[e] == 7.0)
            continue
        want = cma_ask_host(states[e], Zh[e], SCALE)
        assert close(Xh[e, :, :N], want, 1e-11), (e, N)
        assert np.all(Xh[e, :, N:] == 0.0)
        f[e] = ((X[e, :, :N] - torch.as_tensor(targets[e], device=dev)) ** 2).sum(dim=1)
    fh = host(f)
    st.tell(Z, X, f, scale)
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0, 0.0]
    for e, N in enumerate(dims):
        if N == 0:
            assert torch.equal(st.buf[e], before[e])  # untouched
            continue
        want = cma_tell_host(states[e], Zh[e], Xh[e], fh[e], SCALE)
        got = device_state(st, e, N)
        assert got["status"] == 0 and want["status"] == 0 and got["generation"] == want["generation"] == states[e]["generation"] + 1
        for name in ("m", "p_sigma", "p_c", "C"):
            assert close(got[name], want[name], 1e-11), (e, N, name)
        assert abs(got["sigma"] - want["sigma"]) <= 1e-11 * want["sigma"]
        k = int(np.argmin(fh[e]))
        assert got["best_f"] == fh[e, k] and np.array_equal(got["best_x"], Xh[e, k, :N])
        assert np.array_equal(got["C"], got["C"].T)
        d_orth, d_rec = eig_quality(got["B"], got["D"], got["C"])
        w, V = np.linalg.eigh(got["C"])
        h_orth, h_rec = eig_quality(V, np.sqrt(w), got["C"])
        print(f"[lam {lam}] N = {N}: |B^T B - I| {d_orth:.2e} (eigh {h_orth:.2e}), |B D^2 B^T - C| / |C| {d_rec:.2e} (eigh {h_rec:.2e})")
        assert d_orth <= 100 * h_orth and d_rec <= 100 * h_rec, (e, N)
        assert close(np.sort(got["D"] ** 2), w, 1e-12)
        worst = [max(a, b) for a, b in zip(worst, (d_orth, h_orth, d_rec, h_rec))]
    print(f"[lam {lam}] worst: orthogonality {worst[0]:.2e} (eigh {worst[1]:.2e}), reconstruction {worst[2]:.2e} (eigh {worst[3]:.2e})")
    # ties: every fitness 100 except two equal minima -- the lower index ranks first, then the 100s in index order
    st = upload(torch, dev, states, dims)
    ft = np.full((n, lam), 100.0)
    ft[:, [lam - 1, 1]] = -2.5
    st.tell(Z, X, torch.as_tensor(ft, device=dev), scale)
    torch.cuda.synchronize()
    for e, N in enumerate(dims):
        if N == 0:
            continue
        want = cma_tell_host(states[e], Zh[e], Xh[e], ft[e], SCALE)
        got = device_state(st, e, N)
        assert close(got["m"], want["m"], 1e-11) and close(got["C"], want["C"], 1e-11), (e, N)
        assert got["best_f"] == -2.5 and np.array_equal(got["best_x"], Xh[e, 1, :N])


def test_eight_generations_replayed(small_engine):
    """ask -> tell with f = |x - x*|^2 computed on the device; the host replays the tells from the recorded Z and f (sampling basis: the
    device's B, D of that generation, checked against the host's C).  m, sigma, C within 1e-9 relative while cond(C) < 10."""
    import torch
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning.vec_cmaes import CmaState, cma_state_host, cma_tell_host

    eng = small_engine
    dev = eng.device
    dims, lam, G = (9, 30, 48, 0), 12, 8
    n = len(dims)
    rs = np.random.RandomState(8)
    m0 = np.zeros((n, NMAX))
    targets = []
    for e, N in enumerate(dims):
        m0[e, :N] = rs.uniform(5, 30, N)
        targets.append(m0[e, :N] + rs.uniform(-2, 2, N))
    st = CmaState(torch, dev, n, NMAX)
    st.init(torch.as_tensor(np.asarray(dims, dtype=np.int32), device=dev), torch.as_tensor(m0, device=dev))
    scale = torch.as_tensor(SCALE, dtype=torch.float64, device=dev)
    tgt = torch.zeros((n, NMAX), dtype=torch.float64, device=dev)
    msk = torch.zeros((n, NMAX), dtype=torch.float64, device=dev)
    for e, N in enumerate(dims):
        tgt[e, :N] = torch.as_tensor(targets[e], device=dev)
        msk[e, :N] = 1.0
    rec = []
    Z = torch.zeros((n, lam, NMAX), dtype=torch.float32, device=dev)
    X = torch.zeros((n, lam, NMAX), dtype=torch.float64, device=dev)
    for g in range(G):
        eng.normal_rows(Z.view(n, lam * NMAX), lam * NMAX, 5, _ffi.IPP_CMA_STREAM + g)
        st.ask(Z, scale, X)
        f = (((X - tgt[:, None, :]) ** 2) * msk[:, None, :]).sum(dim=2)
        basis = (st.B.clone(), st.D.clone())
        st.tell(Z, X, f, scale)
        rec.append((Z.clone(), X.clone(), f.clone(), basis, st.m.clone(), st.sigma.clone(), st.C.clone()))
    torch.cuda.synchronize()
    assert host(st.status).tolist() == [0, 0, 0, 0] and host(st.generation).tolist() == [G, G, G, 0]
    for e, N in enumerate(dims):
        if N == 0:
            continue
        hs = cma_state_host(m0[e, :N])
        best_f, best_x = np.inf, None
        for g, (Zg, Xg, fg, (Bg, Dg), mg, sg, Cg) in enumerate(rec):
            B, D = host(Bg[e, :N, :N]), host(Dg[e, :N])
            assert eig_quality(B, D, hs["C"])[1] < 1e-11, (e, g)  # the device's basis decomposes the host's C
            hs = cma_tell_host(dict(hs, B=B, D=D), host(Zg[e]), host(Xg[e]), host(fg[e]), SCALE)
            assert hs["status"] == 0 and np.linalg.cond(hs["C"]) < 10, (e, g)
            assert close(host(mg[e, :N]), hs["m"], 1e-9) and close(host(Cg[e, :N, :N]), hs["C"], 1e-9), (e, g)
            assert abs(float(sg[e]) - hs["sigma"]) <= 1e-9 * hs["sigma"], (e, g)
            fh = host(fg[e])
            k = int(np.argmin(fh))
            if fh[k] < best_f:
                best_f, best_x = fh[k], host(Xg[e, k, :N])
        assert float(st.best_f[e]) == best_f and np.array_equal(host(st.best_x[e, :N]), best_x)
        assert hs["best_f"] == best_f


def test_breakdown_is_flagged_and_contained(small_engine):
    """A C that cannot become positive definite (an input check, no fault): status 1, m / B / D as they were, later calls no-ops,
    the neighbours of the launch unaffected."""
    import torch
    from ipp_rl_amd.planning.vec_cmaes import cma_ask_host, cma_tell_host

    dev = small_engine.device
    dims, lam, nmax = (9, 9, 9), 6, 9
    rs = np.random.RandomState(4)
    states = random_states(rs, dims)
    bad = states[1]
    bad["C"] = np.diag([1.0, 1.0, 1.0, 1.0, -50.0, 1.0, 1.0, 1.0, 1.0])
    bad["B"], bad["D"] = np.eye(9), np.ones(9)
    st = upload(torch, dev, states, dims, nmax=nmax)
    scale = torch.as_tensor(SCALE[:nmax], dtype=torch.float64, device=dev)
    Z = torch.as_tensor(rs.normal(size=(3, lam, nmax)), dtype=torch.float32, device=dev)
    X = torch.full((3, lam, nmax), 7.0, dtype=torch.float64, device=dev)
    st.ask(Z, scale, X)
    f = torch.as_tensor(rs.uniform(0, 1, size=(3, lam)), device=dev)
    st.tell(Z, X, f, scale)
    torch.cuda.synchronize()
    assert host(st.status).tolist() == [0, 1, 0]
    got = device_state(st, 1, 9)
    assert np.array_equal(got["m"], bad["m"]) and np.array_equal(got["B"], bad["B"]) and np.array_equal(got["D"], bad["D"])
    assert got["generation"] == bad["generation"]
    Zh, Xh, fh = host(Z), host(X), host(f)
    for e in (0, 2):
        want = cma_tell_host(states[e], Zh[e], Xh[e], fh[e], SCALE[:nmax])
        g = device_state(st, e, 9)
        assert close(g["m"], want["m"], 1e-11) and close(g["C"], want["C"], 1e-11) and abs(g["sigma"] - want["sigma"]) <= 1e-11 * want["sigma"]
    frozen = st.buf[1].clone()
    X2 = torch.full((3, lam, nmax), 7.0, dtype=torch.float64, device=dev)
    st.ask(Z, scale, X2)
    st.tell(Z, X2, f, scale)
    torch.cuda.synchronize()
    assert bool((X2[1] == 7.0).all()) and not bool((X2[0] == 7.0).any())
    assert torch.equal(st.buf[1], frozen)
    assert host(st.generation).tolist() == [states[0]["generation"] + 2, bad["generation"], states[2]["generation"] + 2]


def objective_tolerance(plan):
    """|f - reference| allowed by the per-reward bar TOL: sum over the live steps of TOL (cost_t + 1) / path."""
    if plan["live"] <= 0:
        return 0.0
    return float(np.sum(TOL * (plan["costs"][: plan["live"]] + 1.0)) / plan["path"])


@pytest.mark.parametrize("dim", [10, 20])
def test_objective_on_the_device_matches_the_reference(golden, dim):
    import torch
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.planning.vec_cmaes import TrajectoryBatch, trajectory_plan_host

    g = golden("cmaes")
    wps = g[f"waypoints_{dim}"]
    K, H = len(wps), wps.shape[1]
    amin, amax, _ = g["alts"]
    cfg = EngineConfig(x_dim=dim, y_dim=dim)
    eng = IPPEngine(cfg, capacity=1 + K, state="factor", rank_cap=64, max_batch=1 + K)
    eng.set_uav(UAV["max_v"], UAV["max_a"])
    eng.reset()
    dev = eng.device
    batch = TrajectoryBatch(torch, dev, 1, K, 3 * H, H)
    X = torch.as_tensor(wps.reshape(1, K, 3 * H), dtype=torch.float64, device=dev).contiguous()
    dims = torch.as_tensor([3 * H], dtype=torch.int32, device=dev)
    prev = torch.as_tensor(g["prev"][None], dtype=torch.float64, device=dev)
    src = torch.zeros(K, dtype=torch.int32, device=dev)
    slots = torch.arange(1, K + 1, dtype=torch.int32, device=dev)
    exact = 0
    for adaptive in (1, 0):
        for b, budget in enumerate(g["budgets"]):
            left = torch.as_tensor([budget], dtype=torch.float64, device=dev)
            batch.plan(dims, X, prev, left, cfg, amin, amax, True)
            batch.evaluate(eng, src, slots, bool(adaptive), True)
            f = host(batch.objective())[0]
            live, cost, path = host(batch.live), host(batch.cost), host(batch.path)
            want = g[f"objective_{dim}_a{adaptive}"][b]
            for k in range(K):
                plan = trajectory_plan_host(wps[k], g["prev"], budget, dim, dim, 4.0, amin, amax, UAV)
                assert int(live[k]) == plan["live"], (adaptive, budget, k)
                if plan["live"] >= 0:
                    assert np.max(np.abs(cost[:, k] - plan["costs"])) < 1e-12 and abs(path[k] - plan["path"]) < 1e-12
                tol = objective_tolerance(plan)
                print(f"{dim}x{dim} adaptive {adaptive} budget {budget} trajectory {k}: f {f[k]:.9f} reference {want[k]:.9f} tolerance {tol:.1e}")
                if want[k] == 100 or want[k] == 0:
                    assert f[k] == want[k], (adaptive, budget, k)
                    exact += 1
                else:
                    assert abs(f[k] - want[k]) <= tol, (adaptive, budget, k, f[k], want[k])
    assert exact >= 8
    eng.close()


def oracle_utility(oc, P, mean, cfg, prev, waypoints, budget, dim, amin, amax, adaptive):
    """-simulate_trajectory on the fp64 oracle's prediction steps, and the tolerance the per-reward bar gives it."""
    from ipp_rl_amd.planning.vec_cmaes import trajectory_objective_host, trajectory_plan_host

    plan = trajectory_plan_host(waypoints, prev, budget, dim, dim, cfg.resolution, amin, amax, UAV)
    rewards, p = [], np.asarray(prev, dtype=np.float64)
    info = {"mean": mean, "value_threshold": cfg.value_threshold, "interval_factor": cfg.interval_factor} if adaptive else None
    for t in range(max(plan["live"], 0)):
        r, P, _, _ = orc.predict_step(oc, P, p, waypoints[t], UAV, info)
        rewards.append(r)
        p = waypoints[t]
    return -trajectory_objective_host(plan, rewards), objective_tolerance(plan)


def build_planner(n, lam, horizon, max_iter, offset=0, total=None, seed=31):
    """n planned envs (global ids offset ..) followed by n * lam scratch slots on a 10x10 grid, two executed measurements each."""
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning import VecCmaesPolicy
    from ipp_rl_amd.vec_env import VecIPPEnv

    dim = 10
    cfg = EngineConfig(x_dim=dim, y_dim=dim)
    total = n if total is None else total
    rs = np.random.RandomState(seed)
    white = rs.normal(size=(total, dim, dim))
    acts = np.stack([np.stack([4.0 * rs.randint(0, dim, total) + 2.0, 4.0 * rs.randint(0, dim, total) + 2.0,
                               np.array([8.0, 14.0])[rs.randint(0, 2, total)]], axis=1) for _ in range(2)])
    eps = rs.normal(size=(2, total, 9))
    slots = n * (1 + lam)
    env = VecIPPEnv(cfg, slots, episode_steps=10, seed=seed, env_id_offset=offset, max_batch=max(slots, n * 200))
    pad = lambda a: np.concatenate([a[offset: offset + n], np.repeat(a[offset: offset + 1], n * lam, axis=0)])  # noqa: E731
    env.reset(white_noise=pad(white))
    for t in range(2):
        env.step(pad(acts[t]), meas_noise=pad(eps[t]), auto_reset=False)
    policy = VecCmaesPolicy(env, 8, 14, 6, horizon=horizon, max_iter=max_iter, popsize=lam, seed=seed)
    return env, policy, (white, acts, eps)


def nan_equal(torch, a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def test_planner_end_to_end():
    """10x10 grid, 6 envs with their own ground truths, measurements and start budgets (one pays for fewer than `horizon` waypoints, one
    for none), horizon 3, popsize 6, 4 generations."""
    import torch

    n, lam, H, dim = 6, 6, 3, 10
    env, policy, (white, acts, eps) = build_planner(n, lam, H, 4)
    cfg = env.cfg
    eng = env.engine
    budgets = np.array([60.0, 45.0, 60.0, 30.0, 7.0, 2.0])
    ids, scratch = np.arange(n), n + np.arange(n * lam)
    before = (eng.ranks().clone()[:n], torch.stack([eng.read_diag(b) for b in range(n)]).clone(),
              torch.stack([eng.read_mean(b) for b in range(n)]).clone())
    trace = []
    ways, valid, info = policy.plan(ids, scratch, budgets, trace=trace)
    torch.cuda.synchronize()
    after = (eng.ranks()[:n], torch.stack([eng.read_diag(b) for b in range(n)]), torch.stack([eng.read_mean(b) for b in range(n)]))
    for x, y in zip(before, after):
        assert torch.equal(x, y)  # no env slot outside scratch_ids changed
    assert len(trace) == 4 and tuple(trace[0][1].shape) == (n, lam, 3 * H)
    w, v, greedy = host(ways), host(valid).astype(bool), host(info["greedy"])
    ug, uc, chose, status, dims = (host(info[k]) for k in ("utility_greedy", "utility_cma", "chose_cma", "status", "dims"))
    print("valid waypoints", v.sum(axis=1), "utility greedy", ug, "cma", uc, "chose", chose, "status", status)
    assert v[:4].all() and 0 < v[4].sum() < H and not v[5].any()
    assert np.array_equal(dims, 3 * v.sum(axis=1))
    assert np.all(np.isnan(w[~v])) and np.all(np.isfinite(w[v]))
    ok = (status == 0) & (dims > 0)
    assert ok[:5].all()
    assert np.array_equal(chose[ok].astype(bool), uc[ok] >= ug[ok])  # greedy wins only when strictly larger
    assert not chose[5]
    # the env without a greedy waypoint was never stepped: every action of its candidates in every generation's launch is NaN
    # (its populations' slots hold the env's own state, forked and left alone)
    for s in scratch[5 * lam: 6 * lam]:
        assert int(eng.ranks()[s]) == int(eng.ranks()[5]) and torch.equal(eng.read_diag(int(s)), eng.read_diag(5))
    # the returned trajectory is no worse than greedy's on the fp64 oracle
    oc = orc.OracleConfig(x_dim=dim, y_dim=dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b)
    for b in range(5):
        st = orc.env_reset(oc, white[b])
        prev = np.array([2.0, 2.0, 14.0])
        for t in range(2):
            m = orc.num_measurements(orc.project_fov(oc, acts[t, b]), orc.resolution_factor(acts[t, b]))
            orc.env_step(oc, st, acts[t, b], eps[t, b, :m])
            prev = acts[t, b]
        assert np.array_equal(host(env.prev[b]), prev)
        W = int(v[b].sum())
        u_ret, tol_r = oracle_utility(oc, st.P, st.mean, cfg, prev, w[b, :W], budgets[b], dim, 8, 14, env.adaptive)
        u_gre, tol_g = oracle_utility(oc, st.P, st.mean, cfg, prev, greedy[b, :W], budgets[b], dim, 8, 14, env.adaptive)
        print(f"env {b}: oracle utility returned {u_ret:.6f} greedy {u_gre:.6f} (device: cma {uc[b]:.6f} greedy {ug[b]:.6f})")
        assert u_ret >= u_gre - (tol_r + tol_g), (b, u_ret, u_gre)
        assert abs(ug[b] - u_gre) <= tol_g and abs((uc[b] if chose[b] else ug[b]) - u_ret) <= tol_r
    # refusals
    with pytest.raises(ValueError, match="max_batch"):
        policy.plan(np.zeros(400, dtype=np.int32), np.zeros(400 * lam, dtype=np.int32), np.ones(400))
    from ipp_rl_amd.planning import VecCmaesPolicy
    with pytest.raises(ValueError, match="horizon"):
        VecCmaesPolicy(env, 8, 14, 6, horizon=17)
    for bad in (3, 65):
        with pytest.raises(ValueError, match="popsize"):
            VecCmaesPolicy(env, 8, 14, 6, horizon=3, popsize=bad)
    env.close()


def test_plans_are_deterministic_and_do_not_depend_on_sharding():
    import torch

    lam, H, G = 4, 3, 3
    budgets = np.array([50.0, 40.0, 30.0, 9.0])
    plans = []
    for _ in range(2):
        env, policy, _ = build_planner(4, lam, H, G)
        ways, valid, info = policy.plan(np.arange(4), 4 + np.arange(4 * lam), budgets)
        torch.cuda.synchronize()
        plans.append((ways.clone(), valid.clone(), info["utility_cma"].clone(), info["chose_cma"].clone()))
        env.close()
    for a, b in zip(*plans):
        assert nan_equal(torch, a.double(), b.double())
    assert bool(plans[0][1][:3].all())
    env, policy, _ = build_planner(2, lam, H, G, offset=2, total=4)
    ways, valid, info = policy.plan(np.arange(2), 2 + np.arange(2 * lam), budgets[2:])
    torch.cuda.synchronize()
    assert nan_equal(torch, ways, plans[0][0][2:]) and torch.equal(valid, plans[0][1][2:])
    assert nan_equal(torch, info["utility_cma"], plans[0][2][2:]) and torch.equal(info["chose_cma"], plans[0][3][2:])
    env.close()


def test_act_and_run_follow_the_greedy_policys_conventions():
    """Budget-mode env on a patch-layout engine: the planned envs fly the first waypoint of their plan, the scratch slots behind them hold
    their position with has_action False and a budget of 0 (VecGreedyPolicy.act's convention for an env without an action)."""
    import torch
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning import VecCmaesPolicy
    from ipp_rl_amd.vec_env import VecIPPEnv

    P, lam = 2, 4
    env = VecIPPEnv(EngineConfig(x_dim=50, y_dim=50), P * (1 + lam), window_rows=-1, episode_steps=40, budget=60.0, seed=17)
    assert int(env.engine.info.patch_layout) == 1
    env.reset()
    policy = VecCmaesPolicy(env, 8, 14, 6, horizon=2, max_iter=2, popsize=lam)
    assert policy.planned_envs == P
    prev = env.prev.clone()
    actions, has = policy.act()
    ways, valid, info = policy.last
    torch.cuda.synchronize()
    assert host(has).astype(bool).tolist() == [True] * P + [False] * (P * lam)
    assert torch.equal(actions[:P], ways[:, 0]) and torch.equal(actions[P:], prev[P:]) and bool(valid.all())
    assert float(env.budget[P:].abs().sum()) == 0 and bool((env.budget[:P] == 60.0).all())
    assert host(info["status"]).tolist() == [0, 0] and policy.replans == 1
    policy.run(2)
    torch.cuda.synchronize()
    assert policy.replans == 3 and bool((env.budget[:P] < 60.0).all()) and bool(torch.isfinite(env.prev).all())
    with pytest.raises(ValueError, match="scratch"):
        VecCmaesPolicy(env, 8, 14, 6, horizon=2, max_iter=2, popsize=lam, planned_envs=3).act()
    env.close()
