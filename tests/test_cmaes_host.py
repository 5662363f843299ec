"""
CPU-only checks of the CMA-ES planner's host restatements (ipp_rl_amd/planning/vec_cmaes.py), the oracle of tests/test_hip_cmaes.py:
  * the strategy constants against the closed forms of Hansen's tutorial,
  * 150 generations of ask / tell minimise a 9-dimensional sphere (a wrong sign or a missing term does not),
  * the ranking is stable (an infeasible population of all 100 ranks as 0 .. lam - 1),
  * the trajectory objective reproduces every recorded value of the reference's simulate_trajectory (tests/golden/cmaes.npz),
  * the new C-ABI symbols are declared in the header and bound in _ffi.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UAV = {"max_v": 2.0, "max_a": 2.0}


@pytest.mark.parametrize("N,lam", [(3, 4), (9, 13), (30, 12), (48, 64)])
def test_constants_follow_the_closed_forms(N, lam):
    from ipp_rl_amd.planning.vec_cmaes import cma_constants

    k = cma_constants(N, lam)
    mu = lam // 2
    assert k["mu"] == mu and len(k["weights"]) == mu
    raw = np.array([np.log((lam + 1) / 2) - np.log(i) for i in range(1, mu + 1)])
    w = raw / raw.sum()
    assert np.allclose(k["weights"], w, rtol=1e-15, atol=0)
    assert abs(k["weights"].sum() - 1.0) < 1e-15 and np.all(np.diff(k["weights"]) < 0) and np.all(k["weights"] > 0)
    mu_eff = 1.0 / np.sum(w ** 2)
    want = dict(mu_eff=mu_eff, c_sigma=(mu_eff + 2) / (N + mu_eff + 5),
                d_sigma=1 + 2 * max(0.0, np.sqrt((mu_eff - 1) / (N + 1)) - 1) + (mu_eff + 2) / (N + mu_eff + 5),
                c_c=(4 + mu_eff / N) / (N + 4 + 2 * mu_eff / N), c_1=2 / ((N + 1.3) ** 2 + mu_eff),
                chi_N=np.sqrt(N) * (1 - 1 / (4 * N) + 1 / (21 * N ** 2)))
    want["c_mu"] = min(1 - want["c_1"], 2 * (mu_eff - 2 + 1 / mu_eff) / ((N + 2) ** 2 + mu_eff))
    for name, v in want.items():
        assert abs(k[name] - v) <= 1e-14 * abs(v), name
    assert 1.0 - k["c_1"] - k["c_mu"] > 0
    assert 1 <= k["mu_eff"] <= mu and 0 < k["c_sigma"] < 1 and 0 < k["c_c"] <= 1


def test_sphere_converges():
    from ipp_rl_amd.planning.vec_cmaes import cma_ask_host, cma_state_host, cma_tell_host

    N, lam = 9, 12
    rs = np.random.RandomState(5)
    target = rs.uniform(-3, 3, N)
    scale = np.tile([2.0, 2.0, 0.5], 3)
    st = cma_state_host(target + rs.uniform(-2, 2, N))
    for g in range(150):
        Z = rs.normal(size=(lam, N))
        X = cma_ask_host(st, Z, scale)
        f = np.sum((X - target) ** 2, axis=1)
        st = cma_tell_host(st, Z, X, f, scale)
        assert st["status"] == 0 and st["generation"] == g + 1
        assert np.max(np.abs(st["B"] @ np.diag(st["D"] ** 2) @ st["B"].T - st["C"])) < 1e-12 * np.max(np.abs(st["C"]))
    assert np.sum((st["m"] - target) ** 2) < 1e-6
    assert st["best_f"] < 1e-6 and np.sum((st["best_x"] - target) ** 2) == st["best_f"]


def test_ranking_is_stable_and_breakdown_is_flagged():
    from ipp_rl_amd.planning.vec_cmaes import cma_ask_host, cma_state_host, cma_tell_host, stable_ranking

    assert np.array_equal(stable_ranking(np.full(12, 100.0)), np.arange(12))
    f = np.full(8, 100.0)
    f[[6, 2]] = -1.5
    f[4] = np.nan
    assert np.array_equal(stable_ranking(f), [2, 6, 0, 1, 3, 5, 7, 4])
    # an all-100 population recombines its first mu candidates
    rs = np.random.RandomState(1)
    st = cma_state_host(np.zeros(6))
    Z = rs.normal(size=(8, 6))
    scale = np.ones(6)
    X = cma_ask_host(st, Z, scale)
    new = cma_tell_host(st, Z, X, np.full(8, 100.0), scale)
    from ipp_rl_amd.planning.vec_cmaes import cma_constants
    assert np.allclose(new["m"], cma_constants(6, 8)["weights"] @ Z[:4], rtol=0, atol=1e-15)
    assert new["best_f"] == 100.0 and np.array_equal(new["best_x"], X[0])
    # a covariance that cannot become positive definite: status 1, m / B / D kept, later tells do nothing
    bad = dict(st, C=np.diag([1.0, 1.0, -50.0, 1.0, 1.0, 1.0]))
    out = cma_tell_host(bad, Z, X, np.arange(8.0), scale)
    assert out["status"] == 1 and out["generation"] == 0
    assert np.array_equal(out["m"], st["m"]) and np.array_equal(out["B"], st["B"]) and np.array_equal(out["D"], st["D"])
    assert cma_tell_host(out, Z, X, np.arange(8.0), scale) is out


def test_objective_reproduces_the_reference(golden):
    from ipp_rl_amd.planning.vec_cmaes import trajectory_objective_host, trajectory_plan_host

    g = golden("cmaes")
    prev, (amin, amax, _) = g["prev"], g["alts"]
    seen = {"hundred": 0, "zero": 0, "zero_cost_live": 0, "partial": 0}
    for dim in (10, 20):
        wps = g[f"waypoints_{dim}"]
        for adaptive in (1, 0):
            want, rewards = g[f"objective_{dim}_a{adaptive}"], g[f"rewards_{dim}_a{adaptive}"]
            for b, budget in enumerate(g["budgets"]):
                for k in range(len(wps)):
                    plan = trajectory_plan_host(wps[k], prev, budget, dim, dim, 4.0, amin, amax, UAV)
                    live = int(np.sum(~np.isnan(rewards[b, k])))
                    assert max(plan["live"], 0) == live, (dim, adaptive, budget, k)
                    if plan["live"] >= 0:
                        assert np.max(np.abs(plan["costs"] - g[f"costs_{dim}"][k])) < 1e-12
                    f = trajectory_objective_host(plan, rewards[b, k])
                    assert abs(f - want[b, k]) < 1e-12, (dim, adaptive, budget, k, f, want[b, k])
                    if want[b, k] == 100:
                        assert f == 100
                        seen["hundred"] += 1
                    if want[b, k] == 0:
                        assert f == 0 and plan["live"] == 0
                        seen["zero"] += 1
                    if plan["live"] > 0 and np.any(plan["costs"][: plan["live"]] == 0):
                        seen["zero_cost_live"] += 1
                    if 0 < plan["live"] < 3:
                        seen["partial"] += 1
    assert all(v > 0 for v in seen.values()), seen
    # the far edge is legal, a hair beyond it is not (actions.py:102-106)
    far = trajectory_plan_host([[40.0, 10.0, 9.0]], prev, 200, 10, 10, 4.0, amin, amax, UAV)
    assert far["live"] == 1
    assert trajectory_plan_host([[10.0, np.nextafter(40.0, 41.0), 9.0]], prev, 200, 10, 10, 4.0, amin, amax, UAV)["live"] == -1
    assert trajectory_plan_host([[10.0, 10.0, np.nan]], prev, 200, 10, 10, 4.0, amin, amax, UAV)["live"] == -1
    # waypoint[0] is tested against y_dim and waypoint[1] against x_dim, as the reference writes it
    assert trajectory_plan_host([[50.0, 10.0, 9.0]], prev, 200, 10, 20, 4.0, amin, amax, UAV)["live"] == 1
    assert trajectory_plan_host([[10.0, 50.0, 9.0]], prev, 200, 10, 20, 4.0, amin, amax, UAV)["live"] == -1
    # a live step of a status other than ok / Cholesky fallback makes the trajectory infeasible
    assert trajectory_objective_host(far, [1.0], statuses=[1]) < 0 and trajectory_objective_host(far, [1.0], statuses=[4]) == 100


def test_symbols_are_declared_and_bound():
    from ipp_rl_amd import _ffi

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    names = ["ipp_cma_state_bytes", "ipp_cma_init", "ipp_cma_ask", "ipp_cma_plan", "ipp_cma_objective", "ipp_cma_tell"]
    for n in names:
        assert re.search(rf"^int {n}\(", txt, flags=re.M), n
        assert n in _ffi.PROTOTYPES
    m = re.search(r"#define\s+IPP_CMA_STREAM\s+\((\d+)ull << (\d+)\)", txt)
    assert m and int(m.group(1)) << int(m.group(2)) == _ffi.IPP_CMA_STREAM
    bases = [1 << 40, 2 << 40, _ffi.IPP_BUDGET_STREAM, _ffi.IPP_SP_ACTION_STREAM, _ffi.IPP_SP_INIT_STREAM, _ffi.IPP_SP_TIE_STREAM,
             _ffi.IPP_SP_ARGMAX_STREAM, _ffi.IPP_REPLAY_STREAM]
    assert all(_ffi.IPP_CMA_STREAM >= b + (1 << 40) for b in bases)  # disjoint from every other stream's 2^40 subsequences
    assert _ffi.ABI_VERSION == 17 and re.search(r"#define\s+IPP_ABI_VERSION\s+17\b", txt)
    for macro, val in (("IPP_CMA_MAX_DIM", _ffi.IPP_CMA_MAX_DIM), ("IPP_CMA_MAX_LAMBDA", _ffi.IPP_CMA_MAX_LAMBDA)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", txt).group(1)) == val
    lib = _ffi.load()
    import ctypes

    nbytes = ctypes.c_uint64(0)
    assert lib.ipp_cma_state_bytes(48, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * (2 * 48 * 48 + 5 * 48 + 5)
    assert lib.ipp_cma_state_bytes(49, ctypes.byref(nbytes)) != 0 and b"nmax" in lib.ipp_last_error()
    # argument checks come before any device call
    assert lib.ipp_cma_ask(None, 1, 9, 12, None, None, None, 0, None) != 0 and b"null" in lib.ipp_last_error()
    p = ctypes.c_void_p(0x1000)
    assert lib.ipp_cma_ask(p, 1, 9, 3, p, p, p, 0, None) != 0 and b"lam" in lib.ipp_last_error()
    assert lib.ipp_cma_tell(p, 1, 9, 65, p, p, p, p, 0, None) != 0 and b"lam" in lib.ipp_last_error()
    assert lib.ipp_cma_init(p, -1, 9, p, p, 0, None) != 0 and b"n < 0" in lib.ipp_last_error()
    assert lib.ipp_cma_plan(p, p, p, p, 1, 12, 9, 4, 40.0, 40.0, 8.0, 14.0, 1, 2.0, 2.0, p, p, p, p, p, 0, None) != 0 and \
        b"horizon" in lib.ipp_last_error()
    assert lib.ipp_cma_objective(p, p, p, p, p, -1, 3, p, 0, None) != 0 and b"candidates" in lib.ipp_last_error()
    assert lib.ipp_cma_tell(p, 0, 9, 12, p, p, p, p, 0, None) == 0  # nothing to do
