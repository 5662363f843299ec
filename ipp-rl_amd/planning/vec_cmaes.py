"""
CMA-ES trajectory planner for a whole batch of envs (the batched counterpart of the reference's planning/ipp_masha.py IPPMashaMission):
the greedy look-ahead of `horizon` waypoints (VecGreedyPolicy.search) is refined jointly, in continuous (x, y, z), by one
(mu/mu_w, lambda)-CMA-ES per env; the objective is simulate_trajectory (ipp_masha.py:102-140), the chained covariance-only prediction
steps along the trajectory; the better of {greedy, refined} is returned (:204-217).

The strategy (csrc/k_cmaes.h: ask, tell with a Jacobi eigendecomposition, one wavefront per env, every env with its own dimension), the
trajectory bookkeeping (bounds, costs, live steps) and the objective run on the device; a generation is: normals, ask, plan, fork, `horizon`
covariance-only step launches for the populations of ALL envs, objective, tell -- queued on the stream with no host read.

The reference's `cma` package is replaced by Hansen's published algorithm ("The CMA Evolution Strategy: A Tutorial", default parameters,
positive weights); INTEGRATION.md lists the divergences.  The host restatements below (fp64 NumPy, no GPU) are the oracle of the tests.
"""
import ctypes as C
from typing import Dict, Optional

import numpy as np

from .. import _ffi
from .common.actions import action_costs

NMAX = _ffi.IPP_CMA_MAX_DIM
LAMBDA_MIN, LAMBDA_MAX = 4, _ffi.IPP_CMA_MAX_LAMBDA
INFEASIBLE = 100.0  # simulate_trajectory's value of a trajectory it does not simulate (ipp_masha.py:106, :115)


# ----------------------------------------------------------------------------------------------- host restatements
def cma_constants(N: int, lam: int) -> Dict:
    """The strategy parameters of dimension N and population lam (tutorial, default parameters, positive weights only)."""
    mu = lam // 2
    w = np.log((lam + 1) / 2.0) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    w = w / w.sum()
    mu_eff = 1.0 / np.sum(w * w)
    c_sigma = (mu_eff + 2.0) / (N + mu_eff + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, np.sqrt((mu_eff - 1.0) / (N + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mu_eff / N) / (N + 4.0 + 2.0 * mu_eff / N)
    c_1 = 2.0 / ((N + 1.3) ** 2 + mu_eff)
    c_mu = min(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((N + 2.0) ** 2 + mu_eff))
    chi_N = np.sqrt(N) * (1.0 - 1.0 / (4.0 * N) + 1.0 / (21.0 * N * N))
    return dict(mu=mu, weights=w, mu_eff=mu_eff, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi_N=chi_N)


def cma_state_host(m0) -> Dict:
    """The start state of a search from m0 (sigma = 1, C = I): what ipp_cma_init writes."""
    m0 = np.array(m0, dtype=np.float64)
    N = m0.size
    return dict(m=m0, sigma=1.0, C=np.eye(N), B=np.eye(N), D=np.ones(N), p_sigma=np.zeros(N), p_c=np.zeros(N), generation=0,
                best_x=m0.copy(), best_f=np.inf, status=0)


def stable_ranking(f) -> np.ndarray:
    """Indices of f in ascending order, ties to the lower index, NaN as +inf."""
    f = np.asarray(f, dtype=np.float64)
    return np.argsort(np.where(np.isnan(f), np.inf, f), kind="stable")


def cma_ask_host(state: Dict, Z, scale) -> np.ndarray:
    """X [lam, N] = m + sigma s (.) (B (D (.) z_k)) for the normals Z [lam, >= N]."""
    N = state["m"].size
    Z = np.asarray(Z, dtype=np.float64)[:, :N]
    s = np.asarray(scale, dtype=np.float64)[:N]
    Y = (Z * state["D"][None, :]) @ state["B"].T
    return state["m"][None, :] + state["sigma"] * s[None, :] * Y


def cma_tell_host(state: Dict, Z, X, f, scale) -> Dict:
    """One update from the fitness f [lam] of the candidates X = cma_ask_host(state, Z, scale); returns the new state (the old one is
    not written).  B, D of the new state come from numpy.linalg.eigh.  Breakdown (an eigenvalue not finite and positive, sigma not
    finite): status 1, m, B and D kept; a state whose status is not 0 is returned as it is."""
    if state["status"] != 0:
        return state
    N = state["m"].size
    f = np.asarray(f, dtype=np.float64)
    lam = f.size
    k = cma_constants(N, lam)
    Z = np.asarray(Z, dtype=np.float64)[:, :N]
    X = np.asarray(X, dtype=np.float64)[:, :N]
    s = np.asarray(scale, dtype=np.float64)[:N]
    order = stable_ranking(f)
    new = dict(state)
    fs = np.where(np.isnan(f), np.inf, f)
    if fs[order[0]] < state["best_f"]:
        new["best_x"], new["best_f"] = X[order[0]].copy(), float(fs[order[0]])
    B, D, w = state["B"], state["D"], k["weights"]
    Y = (Z[order[: k["mu"]]] * D[None, :]) @ B.T
    y_w = w @ Y
    m = state["m"] + state["sigma"] * s * y_w
    p_sigma = (1.0 - k["c_sigma"]) * state["p_sigma"] + np.sqrt(k["c_sigma"] * (2.0 - k["c_sigma"]) * k["mu_eff"]) * (B @ ((B.T @ y_w) / D))
    norm = np.linalg.norm(p_sigma)
    h_sigma = float(norm / np.sqrt(1.0 - (1.0 - k["c_sigma"]) ** (2.0 * (state["generation"] + 1))) < (1.4 + 2.0 / (N + 1.0)) * k["chi_N"])
    p_c = (1.0 - k["c_c"]) * state["p_c"] + h_sigma * np.sqrt(k["c_c"] * (2.0 - k["c_c"]) * k["mu_eff"]) * y_w
    Cm = ((1.0 - k["c_1"] - k["c_mu"]) * state["C"] +
          k["c_1"] * (np.outer(p_c, p_c) + (1.0 - h_sigma) * k["c_c"] * (2.0 - k["c_c"]) * state["C"]) +
          k["c_mu"] * (Y.T * w[None, :]) @ Y)
    Cm = 0.5 * (Cm + Cm.T)
    with np.errstate(over="ignore", invalid="ignore"):
        sigma = state["sigma"] * np.exp((k["c_sigma"] / k["d_sigma"]) * (norm / k["chi_N"] - 1.0))
    new.update(C=Cm, p_sigma=p_sigma, p_c=p_c, sigma=float(sigma))
    try:
        eig, vec = np.linalg.eigh(Cm)
    except np.linalg.LinAlgError:
        eig, vec = np.full(N, np.nan), B
    if not (np.all(np.isfinite(eig)) and np.all(eig > 0) and np.isfinite(sigma)):
        new["status"] = 1
        return new
    new.update(m=m, B=vec, D=np.sqrt(eig), generation=state["generation"] + 1)
    return new


def trajectory_plan_host(waypoints, prev, budget: float, x_dim: int, y_dim: int, resolution: float, min_altitude: float,
                         max_altitude: float, uav: Optional[Dict] = None) -> Dict:
    """simulate_trajectory's bookkeeping (ipp_masha.py:102-125) for waypoints [W, 3] flown from `prev` with `budget` left:
    costs [W], path (their sum), live (steps before the first unaffordable one; -1 out of bounds, -2 path cost <= 0)."""
    wps = np.asarray(waypoints, dtype=np.float64).reshape(-1, 3)
    prev = np.asarray(prev, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = ((0 <= wps[:, 1]) & (wps[:, 1] <= x_dim * resolution) & (0 <= wps[:, 0]) & (wps[:, 0] <= y_dim * resolution) &
                  (min_altitude <= wps[:, 2]) & (wps[:, 2] <= max_altitude))  # out_of_bounds, actions.py:102-106
    if not bool(inside.all()):
        return dict(costs=np.zeros(len(wps)), path=0.0, live=-1)
    costs = np.empty(len(wps))
    p = prev
    for t, w in enumerate(wps):
        costs[t] = action_costs(w, p, uav)
        p = w
    path = 0.0
    for c in costs:
        path += c
    if path <= 0:
        return dict(costs=costs, path=float(path), live=-2)
    live, left = 0, float(budget)
    for c in costs:
        if c > left:
            break
        left -= c
        live += 1
    return dict(costs=costs, path=float(path), live=live)


def trajectory_objective_host(plan: Dict, rewards, statuses=None) -> float:
    """simulate_trajectory's value (ipp_masha.py:104-106, :114-115, :135-140) from the per-step rewards of the live steps."""
    if plan["live"] < 0:
        return INFEASIBLE
    total = 0.0
    for t in range(plan["live"]):
        if statuses is not None and int(statuses[t]) not in (0, 1):
            return INFEASIBLE
        total += float(rewards[t]) * (plan["costs"][t] + 1.0)
    return -total / plan["path"]


def coordinate_scales(sigma0, min_altitude: float, max_altitude: float, horizon: int) -> np.ndarray:
    """CMA_stds of calculate_parameter_bounds_and_scales (ipp_masha.py:151-156), [3 * horizon]."""
    return np.tile(np.array([sigma0[0], sigma0[1], min(sigma0[2], (max_altitude - min_altitude) / 2.0)], dtype=np.float64), int(horizon))


# ----------------------------------------------------------------------------------------------- the device calls
class CmaState:
    """n envs' strategy states in one device buffer (the layout of include/ipp_engine.h "Batched CMA-ES"), with named views."""

    def __init__(self, torch, device, n: int, nmax: int):
        if not 1 <= nmax <= NMAX:
            raise ValueError(f"nmax must lie in [1, {NMAX}]")
        nbytes = C.c_uint64(0)
        _ffi.check(_ffi.load().ipp_cma_state_bytes(int(nmax), C.byref(nbytes)))
        self.torch, self.device, self.n, self.nmax, self.words = torch, torch.device(device), int(n), int(nmax), int(nbytes.value) // 8
        self.buf = torch.zeros((self.n, self.words), dtype=torch.float64, device=self.device)
        self._ints = self.buf.view(torch.int64)
        NM = self.nmax
        o = 0
        self._off = {}
        for name, size in (("m", NM), ("sigma", 1), ("C", NM * NM), ("B", NM * NM), ("D", NM), ("p_sigma", NM), ("p_c", NM), ("best_x", NM),
                           ("best_f", 1), ("generation", 1), ("status", 1), ("dims", 1)):
            self._off[name] = (o, size)
            o += size
        assert o == self.words

    def __getattr__(self, name):
        off = self.__dict__.get("_off", {})
        if name not in off:
            raise AttributeError(name)
        o, size = off[name]
        src = self._ints if name in ("generation", "status", "dims") else self.buf
        v = src[:, o: o + size]
        if name in ("C", "B"):
            return v.view(self.n, self.nmax, self.nmax)
        return v[:, 0] if size == 1 else v

    @property
    def device_index(self) -> int:
        return self.device.index or 0

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def init(self, dims, m0):
        """ipp_cma_init: dims int32 [n], m0 float64 [n, nmax] device tensors."""
        _ffi.check(_ffi.load().ipp_cma_init(self.buf.data_ptr(), self.n, self.nmax, dims.data_ptr(), m0.data_ptr(), self.device_index,
                                            self._stream()))

    def ask(self, Z, scale, X):
        """ipp_cma_ask: Z float32 [n, lam, nmax], scale float64 [nmax], X float64 [n, lam, nmax] (out)."""
        _ffi.check(_ffi.load().ipp_cma_ask(self.buf.data_ptr(), self.n, self.nmax, int(Z.shape[1]), Z.data_ptr(), scale.data_ptr(), X.data_ptr(),
                                           self.device_index, self._stream()))

    def tell(self, Z, X, f, scale):
        """ipp_cma_tell: f float64 [n, lam]."""
        _ffi.check(_ffi.load().ipp_cma_tell(self.buf.data_ptr(), self.n, self.nmax, int(Z.shape[1]), Z.data_ptr(), X.data_ptr(), f.data_ptr(),
                                            scale.data_ptr(), self.device_index, self._stream()))


class TrajectoryBatch:
    """The buffers of one evaluation pass: n envs x per_env candidates x horizon steps (ipp_cma_plan / ipp_cma_objective)."""

    def __init__(self, torch, device, n: int, per_env: int, nmax: int, horizon: int):
        self.torch, self.device = torch, torch.device(device)
        self.n, self.per_env, self.nmax, self.horizon = int(n), int(per_env), int(nmax), int(horizon)
        nc = self.n * self.per_env
        f64 = dict(dtype=torch.float64, device=self.device)
        self.action = torch.zeros((self.horizon, nc, 3), **f64)
        self.prev_action = torch.zeros((self.horizon, nc, 3), **f64)
        self.cost = torch.zeros((self.horizon, nc), **f64)
        self.path = torch.zeros(nc, **f64)
        self.live = torch.zeros(nc, dtype=torch.int32, device=self.device)
        self.reward = torch.zeros((self.horizon, nc), dtype=torch.float32, device=self.device)
        self.status = torch.zeros((self.horizon, nc), dtype=torch.int32, device=self.device)
        self.f = torch.zeros((self.n, self.per_env), **f64)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def plan(self, dims, X, prev, budget, cfg, min_altitude: float, max_altitude: float, use_flight_time: bool):
        """dims int32 [n], X float64 [n, per_env, nmax], prev float64 [n, 3], budget float64 [n]: device tensors."""
        _ffi.check(_ffi.load().ipp_cma_plan(
            dims.data_ptr(), X.data_ptr(), prev.data_ptr(), budget.data_ptr(), self.n, self.per_env, self.nmax, self.horizon,
            float(cfg.y_dim * cfg.resolution), float(cfg.x_dim * cfg.resolution), float(min_altitude), float(max_altitude),
            1 if use_flight_time else 0, float(cfg.max_v), float(cfg.max_a), self.action.data_ptr(), self.prev_action.data_ptr(),
            self.cost.data_ptr(), self.path.data_ptr(), self.live.data_ptr(), self.device.index or 0, self._stream()))

    def evaluate(self, engine, src_ids, slot_ids, adaptive: bool, use_flight_time: bool):
        """Fork src_ids -> slot_ids (int32 [n * per_env] device tensors) and run the `horizon` covariance-only step launches there."""
        engine.fork(src_ids, slot_ids)
        for t in range(self.horizon):
            engine.step(self.action[t], self.prev_action[t], env_ids=slot_ids, cov_only=True, adaptive=adaptive, use_flight_time=use_flight_time,
                        reward_out=self.reward[t], status_out=self.status[t])

    def objective(self):
        _ffi.check(_ffi.load().ipp_cma_objective(self.reward.data_ptr(), self.status.data_ptr(), self.cost.data_ptr(), self.path.data_ptr(),
                                                 self.live.data_ptr(), self.n * self.per_env, self.horizon, self.f.data_ptr(),
                                                 self.device.index or 0, self._stream()))
        return self.f


# ----------------------------------------------------------------------------------------------- the device policy
class VecCmaesPolicy:
    def __init__(self, env, min_altitude: float, max_altitude: float, altitude_spacing: float, horizon: int = 10,
                 sigma0=(2.0, 2.0, 0.5), max_iter: int = 32, popsize: int = 12, seed: Optional[int] = None, planned_envs: Optional[int] = None):
        """env: a VecIPPEnv (a patch-layout engine for the one-launch greedy look-ahead; on other engines the look-ahead scores its
        candidates through predict-only step launches).  horizon, sigma0, max_iter, popsize: episode_horizon, cmaes_sigma0,
        cmaes_max_iter, cmaes_population_size of IPPMashaMission.  seed: key of the normals (default: the env's seed).
        planned_envs (act / run only): the envs 0 .. planned_envs - 1 are planned for, the slots behind them are the populations'
        scratch -- num_envs >= planned_envs * (1 + popsize); default num_envs // (1 + popsize)."""
        from .vec_greedy import VecGreedyPolicy

        if 3 * int(horizon) > NMAX or int(horizon) < 1:
            raise ValueError(f"horizon must lie in [1, {NMAX // 3}] (3 * horizon <= {NMAX} coordinates)")
        if not LAMBDA_MIN <= int(popsize) <= LAMBDA_MAX:
            raise ValueError(f"popsize must lie in [{LAMBDA_MIN}, {LAMBDA_MAX}]")
        if int(max_iter) < 0:
            raise ValueError("max_iter must not be negative")
        if len(sigma0) != 3 or not all(float(s) > 0 for s in sigma0):
            raise ValueError("sigma0: three positive standard deviations (x, y, z)")
        self.greedy = VecGreedyPolicy(env, min_altitude, max_altitude, altitude_spacing)
        self.env, self.cfg = env, env.cfg
        self.min_altitude, self.max_altitude = float(min_altitude), float(max_altitude)
        self.horizon, self.max_iter, self.popsize = int(horizon), int(max_iter), int(popsize)
        self.nmax = 3 * self.horizon
        self.seed = int(env.seed if seed is None else seed)
        self.replans = 0
        self.scale = env.torch.as_tensor(coordinate_scales(sigma0, self.min_altitude, self.max_altitude, self.horizon), dtype=env.torch.float64,
                                         device=env.device)
        self.planned_envs = int(env.num_envs // (1 + self.popsize) if planned_envs is None else planned_envs)
        self.last = None

    # -- the greedy look-ahead on engines without the one-launch scoring: candidates through predict-only steps (GreedyPlanner.score's
    #    shared_pass=False route), the rest as VecGreedyPolicy.search
    def _search_by_steps(self, ids, sids, budget):
        env, torch, g = self.env, self.env.torch, self.greedy
        eng = env.engine
        eng.fork(ids, sids)
        prev = env.prev[ids.long()].clone()
        left = budget.clone()
        alive = torch.ones(ids.numel(), dtype=torch.bool, device=env.device)
        ways, valids = [], []
        cfg = self.cfg
        for _ in range(self.horizon):
            cands = g.candidates(prev)
            n, k = cands.shape[:2]
            flat, pv, rep = cands.reshape(-1, 3), prev.repeat_interleave(k, dim=0), sids.repeat_interleave(k)
            reward = torch.empty(n * k, dtype=torch.float32, device=env.device)
            for i in range(0, n * k, int(eng.max_batch)):
                j = min(n * k, i + int(eng.max_batch))
                eng.step(flat[i:j], pv[i:j], env_ids=rep[i:j], cov_only=True, predict_only=True, adaptive=env.adaptive,
                         use_flight_time=env.use_flight_time, reward_out=reward[i:j])
            dist = torch.linalg.vector_norm(flat - pv, dim=-1)
            cost = dist
            if env.use_flight_time:
                ramp = torch.clamp(0.5 * dist, max=cfg.max_v ** 2 / (2 * cfg.max_a))
                cost = (dist - 2 * ramp) / cfg.max_v + 2 * torch.sqrt(2 * ramp / cfg.max_a)
            chosen, idx, has = g._pick(cands, reward.reshape(n, k), cost.reshape(n, k), left)
            alive = alive & has
            nan = torch.full_like(chosen, float("nan"))
            step_to = torch.where(alive[:, None], chosen, nan)
            eng.step(step_to, prev, env_ids=sids, cov_only=True, adaptive=env.adaptive, use_flight_time=env.use_flight_time)
            spent = cost.reshape(n, k)[torch.arange(n, device=env.device), idx]
            left = torch.where(alive, left - spent, left)
            prev = torch.where(alive[:, None], chosen, prev)
            ways.append(step_to)
            valids.append(alive)
        return torch.stack(ways, dim=1), torch.stack(valids, dim=1)

    def plan(self, env_ids, scratch_ids, budget, trace: Optional[list] = None):
        """One replan (IPPMashaMission.replan, ipp_masha.py:180-219) for the envs `env_ids` from env.prev and the remaining budgets
        `budget` [n].  scratch_ids: len(env_ids) * popsize spare slots of the engine (the populations are evaluated there; the envs
        themselves are not written).  Returns (waypoints [n, horizon, 3] with NaN rows past an env's last waypoint, valid [n, horizon],
        info) -- greedy's waypoints where its utility is strictly larger (:214), where the search broke down or where greedy found
        nothing; info: utility_greedy, utility_cma, chose_cma, status, dims (device tensors).  Nothing is read back to the host.
        trace: a list that receives per generation the device tensors (Z, X, f, m, sigma, C)."""
        env, torch = self.env, self.env.torch
        eng, dev = env.engine, env.device
        def as_ids(x):
            if isinstance(x, torch.Tensor):
                return x.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            return torch.as_tensor(np.asarray(x), dtype=torch.int32, device=dev).reshape(-1)

        ids, sids = as_ids(env_ids), as_ids(scratch_ids)
        n, lam, H, NM = int(ids.numel()), self.popsize, self.horizon, self.nmax
        if int(sids.numel()) != n * lam:
            raise ValueError(f"scratch_ids: {n} envs x popsize {lam} = {n * lam} slots needed, {int(sids.numel())} given")
        if n * lam > int(eng.max_batch):
            raise ValueError(f"{n} envs x popsize {lam} exceed the engine's max_batch {int(eng.max_batch)}")
        left = budget.to(device=dev, dtype=torch.float64).clone() if isinstance(budget, torch.Tensor) else \
            torch.as_tensor(np.asarray(budget, dtype=np.float64), dtype=torch.float64, device=dev)
        if int(left.numel()) != n:
            raise ValueError("budget needs one entry per env")
        if int(eng.info.patch_layout) == 1:
            ways, valid = self.greedy.search(ids, sids[:n], left, H)
        else:
            ways, valid = self._search_by_steps(ids, sids[:n], left)
        dims = (3 * valid.sum(dim=1)).to(torch.int32)
        greedy_x = torch.where(valid[:, :, None], ways, torch.zeros_like(ways)).reshape(n, NM).contiguous()
        prev = env.prev[ids.long()].clone()
        state = CmaState(torch, dev, n, NM)
        state.init(dims, greedy_x)
        Z = torch.zeros((n, lam, NM), dtype=torch.float32, device=dev)
        X = torch.zeros((n, lam, NM), dtype=torch.float64, device=dev)
        pop = TrajectoryBatch(torch, dev, n, lam, NM, H)
        src = ids.repeat_interleave(lam)
        replan = self.replans
        self.replans += 1
        for g in range(self.max_iter):
            eng.normal_rows(Z.view(n, lam * NM), lam * NM, self.seed, _ffi.IPP_CMA_STREAM + replan * self.max_iter + g, row_ids=ids,
                            row_offset=env.env_id_offset)
            state.ask(Z, self.scale, X)
            pop.plan(dims, X, prev, left, self.cfg, self.min_altitude, self.max_altitude, env.use_flight_time)
            pop.evaluate(eng, src, sids, env.adaptive, env.use_flight_time)
            f = pop.objective()
            state.tell(Z, X, f, self.scale)
            if trace is not None:
                trace.append((Z.clone(), X.clone(), f.clone(), state.m.clone(), state.sigma.clone(), state.C.clone()))
        # greedy against the best-ever candidate, both evaluated once more (ipp_masha.py:204, :211)
        pair = TrajectoryBatch(torch, dev, n, 2, NM, H)
        both = torch.stack([greedy_x, state.best_x], dim=1).contiguous()
        pair.plan(dims, both, prev, left, self.cfg, self.min_altitude, self.max_altitude, env.use_flight_time)
        pair.evaluate(eng, ids.repeat_interleave(2), sids[: 2 * n], env.adaptive, env.use_flight_time)
        f2 = pair.objective()
        utility_greedy, utility_cma = -f2[:, 0], -f2[:, 1]
        status = state.status.to(torch.int32)
        chose = (status == 0) & (dims > 0) & ~(utility_greedy > utility_cma)  # (:214: greedy only when strictly better)
        best = torch.where(chose[:, None], state.best_x, greedy_x).reshape(n, H, 3)
        waypoints = torch.where(valid[:, :, None], best, torch.full_like(best, float("nan")))
        info = dict(utility_greedy=utility_greedy, utility_cma=utility_cma, chose_cma=chose, status=status, dims=dims, greedy=ways)
        self._keep = (state, pop, pair, Z, X, both, src)
        return waypoints, valid, info

    def act(self):
        """One decision per planned env (the reference's adaptive execution, ipp_masha.py:234-235: replan, fly the first waypoint):
        ([B, 3] waypoints, has_action [B]) with VecGreedyPolicy.act's conventions -- an env without an affordable waypoint, and every
        scratch slot, keeps its waypoint, and in budget mode its budget is set to 0."""
        env, torch = self.env, self.env.torch
        P, lam = self.planned_envs, self.popsize
        if P < 1 or P * (1 + lam) > env.num_envs:
            raise ValueError(f"act(): {P} planned envs need {P * lam} scratch slots behind them; the env has {env.num_envs} slots")
        budget_mode = getattr(env, "budget_mode", False)
        left = env.budget[:P] if budget_mode else torch.full((P,), float("inf"), dtype=torch.float64, device=env.device)
        ways, valid, info = self.plan(np.arange(P), P + np.arange(P * lam), left)
        has = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
        has[:P] = valid[:, 0]
        actions = env.prev.clone()
        actions[:P] = torch.where(valid[:, :1], ways[:, 0], env.prev[:P])
        if budget_mode:
            env.budget.mul_(has.to(env.budget.dtype))
        self.last = (ways, valid, info)
        return actions, has

    def run(self, steps: int):
        """`steps` times act() then env.step(actions)."""
        for _ in range(int(steps)):
            actions, _ = self.act()
            self.env.step(actions)
        return self.env.reward
