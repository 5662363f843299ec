"""
The four baseline missions for a whole batch of envs (the batched counterparts of the reference's
planning/baselines/{lawn_mower,conical_spiral,random_discrete,random_continuous}_mission.py): one decision per env and call on the
device (ipp_baseline_act, csrc/k_baselines.h), on a budget-mode VecIPPEnv.  The reference plans a whole mission up front
(create_waypoints) and then flies it (execute); here the two budget tests are one rule per decision on the env's own ledger, so a
mission runs through episode ends and device-side resets with nothing read from the device: an env whose episode index changed starts
its table again at row 0.

The waypoint tables of the lawnmower and the spiral are built once on the host (lawnmower_table, spiral_table: create_waypoints at
budget = +inf, quirks kept); the random kinds draw from the caller's uniforms (parity runs, tests) or from Philox
(vec_env.philox_uniform, subsequence IPP_BASELINE_STREAM + the env's decision counter).

The host restatements below (fp64 NumPy, no GPU) are the oracle of the tests; INTEGRATION.md "Baselines and comparison curves" lists the
divergences from the reference.
"""
import ctypes as C
from typing import Optional

import numpy as np

from .. import _ffi
from .common.actions import _trapezoid_time

INIT_ACTION = np.array([2.0, 2.0, 14.0])  # planning/missions.py:69
TRIALS = _ffi.IPP_BASELINE_TRIALS


# ----------------------------------------------------------------------------------------------- host restatements
def _distance(a, b):
    """Euclidean distance, the three squares summed in order and every operation rounded on its own (what the kernels compute)."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def mission_cost(a, b, use_flight_time: bool, max_v: float, max_a: float):
    """action_costs (planning/common/actions.py:8-12): the flight time with UAV limits, else the distance."""
    d = _distance(a, b)
    return _trapezoid_time(d, float(max_v), float(max_a)) if use_flight_time else d


def altitude_linspace(min_altitude: float, max_altitude: float, altitude_spacing: float) -> np.ndarray:
    """The baselines' altitude levels (lawn_mower_mission.py:87-91, actions.py:74)."""
    return np.linspace(min_altitude, max_altitude, int((max_altitude - min_altitude) / altitude_spacing) + 1)


def lawnmower_table(x_dim: int, y_dim: int, resolution: float, dist_to_boundaries: float = 10, min_altitude: float = 5,
                    max_altitude: float = 30, step_size: float = 5, altitude_spacing: float = 5) -> np.ndarray:
    """[K, 3] float64: LawnMowerMission.create_waypoints (lawn_mower_mission.py:66-114) at budget = +inf.  Quirks kept: a waypoint is
    [y_coord, x_coord, altitude] truncated by dtype=int, and the x of odd rows is mirrored with x_dim * resolution - x."""
    lo = dist_to_boundaries
    hi_x = x_dim * resolution - dist_to_boundaries
    xs = np.linspace(lo, hi_x, int((hi_x - lo) / step_size) + 1)
    hi_y = y_dim * resolution - dist_to_boundaries
    ys = np.linspace(lo, hi_y, int((hi_y - lo) / step_size) + 1)
    rows = []
    for altitude in altitude_linspace(min_altitude, max_altitude, altitude_spacing):
        for j, y in enumerate(ys):
            for x in xs:
                if j % 2 == 1:
                    x = x_dim * resolution - x
                rows.append(np.array([y, x, altitude], dtype=int))
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def spiral_table(x_dim: int, y_dim: int, resolution: float, dist_to_boundaries: float = 10, min_altitude: float = 5,
                 max_altitude: float = 30, num_waypoints: int = 200, slope_factor: float = 10) -> np.ndarray:
    """[num_waypoints, 3] float64: ConicalSpiralMission.create_waypoints (conical_spiral_mission.py:67-97) before its budget cut.
    Quirks kept: x is centred with y_dim and y with x_dim, and the altitudes are flipped (the spiral starts at max_altitude)."""
    t_max = 0.5 * np.minimum(x_dim * resolution, y_dim * resolution) - dist_to_boundaries
    c = (max_altitude - min_altitude) / t_max ** 2
    t = np.linspace(0, t_max, num_waypoints)
    x = t * np.cos(slope_factor * t) + 0.5 * y_dim * resolution
    y = t * np.sin(slope_factor * t) + 0.5 * x_dim * resolution
    z = np.flip(c * np.square(t) + min_altitude)
    return np.ascontiguousarray(np.transpose(np.array([x, y, z])), dtype=np.float64)


def table_next(kind: str, table: np.ndarray, cursor: int, prev, budget: float, step_size: float, use_flight_time: bool, max_v: float,
               max_a: float):
    """(has, waypoint) of one table decision: the lawnmower's `budget >= step_size and budget > cost` (lawn_mower_mission.py:93-100,130) or the
    spiral's `cursor == 0 or budget - cost >= 0` (conical_spiral_mission.py:100-106)."""
    prev = np.asarray(prev, dtype=np.float64)
    if not (0 <= cursor < len(table)):
        return False, prev
    c = float(mission_cost(table[cursor], prev, use_flight_time, max_v, max_a))
    has = (budget >= step_size and budget > c) if kind == "lawnmower" else (cursor == 0 or budget - c >= 0)
    return bool(has), (table[cursor] if has else prev)


def discrete_actions(x_dim: int, y_dim: int, resolution: float, levels) -> np.ndarray:
    """actions_np of RandomDiscreteMission (enumerate_actions + action_dict_to_np_array, actions.py:73-99) on a square grid: row
    h N + x_dim xc + yc is (resolution xc + resolution / 2, resolution yc + resolution / 2, levels[h]) -- the reference flattens (x cell, y cell)."""
    if x_dim != y_dim:
        raise ValueError("enumerate_actions' index x_dim * xc + yc is one-to-one on square grids only")
    levels = np.asarray(levels, dtype=np.float64)
    c = np.arange(x_dim * y_dim)
    xc, yc = c // x_dim, c % x_dim
    out = np.empty((len(levels), x_dim * y_dim, 3))
    out[..., 0] = (xc * float(resolution) + 0.5 * resolution)[None, :]
    out[..., 1] = (yc * float(resolution) + 0.5 * resolution)[None, :]
    out[..., 2] = levels[:, None]
    return out.reshape(-1, 3)


def discrete_mask(actions: np.ndarray, prev, budget: float, adaptive: bool, max_v: float, max_a: float) -> np.ndarray:
    """get_next_actions_mask (random_discrete_mission.py:73-79)."""
    d = _distance(actions, np.asarray(prev, dtype=np.float64))
    if not adaptive:
        return (d > 0) & (d <= budget) & (d < 11.5)
    t = _trapezoid_time(d, float(max_v), float(max_a))
    return (t > 0) & (t <= budget)


def random_discrete_next(actions: np.ndarray, prev, budget: float, u: float, adaptive: bool, max_v: float, max_a: float):
    """One draw of RandomDiscreteMission.create_waypoints (:93-100) at the uniform u: (count, rank, action index, waypoint, has).  rank =
    min(floor(u count), count - 1) among the valid actions in index order (np.random.choice(count) replaced by the uniform)."""
    msk = discrete_mask(actions, prev, budget, adaptive, max_v, max_a)
    count = int(msk.sum())
    if count == 0:
        return 0, -1, -1, np.asarray(prev, dtype=np.float64), False
    k = min(int(np.floor(u * count)), count - 1)
    idx = int(np.nonzero(msk)[0][k])
    return count, k, idx, actions[idx], True


def continuous_box(x_dim: int, y_dim: int, resolution: float, dist_to_boundaries: float, min_altitude: float, max_altitude: float):
    """(low, high) of RandomContinuousMission.create_waypoints (random_continuous_mission.py:68-83): the FIRST coordinate's upper bound
    comes from x_dim and is called y there, the second from y_dim -- the reference's swap, kept."""
    low = np.array([dist_to_boundaries, dist_to_boundaries, min_altitude], dtype=np.float64)
    high = np.array([x_dim * resolution - dist_to_boundaries, y_dim * resolution - dist_to_boundaries, max_altitude], dtype=np.float64)
    return low, high


def random_continuous_next(prev, budget: float, u, low, high, use_flight_time: bool, max_v: float, max_a: float):
    """One outer iteration of RandomContinuousMission.create_waypoints (:79-97) with the uniforms u [101, 3]: (trial, action, has, chosen).
    The first trial with budget - cost >= 0 wins, else the 101st: `chosen`; has = budget >= 0 and budget > cost(chosen) (the `while` of
    :79 and execute's break, :118); action = chosen when has, else prev."""
    u = np.asarray(u, dtype=np.float64).reshape(TRIALS, 3)
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    prev = np.asarray(prev, dtype=np.float64)
    way = low + (high - low) * u
    cost = mission_cost(way, prev, use_flight_time, max_v, max_a)
    ok = np.nonzero(budget - cost >= 0)[0]
    t = int(ok[0]) if len(ok) else TRIALS - 1
    has = bool(budget >= 0 and budget > cost[t])
    return t, (way[t] if has else prev), has, way[t]


def baseline_uniform(seed: int, global_env_id, decision, trial=0, component=0) -> np.ndarray:
    """The device's Philox uniform of (env, decision, trial, component): vec_env.philox_uniform(512 id + 4 trial + component,
    IPP_BASELINE_STREAM + decision, seed)."""
    from ..vec_env import philox_uniform

    counter = np.asarray(global_env_id, dtype=np.int64) * 512 + 4 * np.asarray(trial, dtype=np.int64) + np.asarray(component, dtype=np.int64)
    return philox_uniform(counter, _ffi.IPP_BASELINE_STREAM + np.asarray(decision, dtype=np.int64), seed)


def curve_resample_host(xs, ys, max_x: float, grid: int) -> np.ndarray:
    """[grid, V]: np.interp of every column of ys [T, V] onto np.linspace(0, max_x, grid) (experiments.py:228-229)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    axis = np.linspace(0, max_x, int(grid))
    return np.stack([np.interp(axis, xs, ys[:, v]) for v in range(ys.shape[1])], axis=1)


def curve_reduce_host(per_env):
    """(mean [G, V], sd [G, V]) over the envs of per_env [B, G, V]; sd with ddof = 1, 0 for a single env."""
    per_env = np.asarray(per_env, dtype=np.float64)
    mean = per_env.mean(axis=0)
    sd = per_env.std(axis=0, ddof=1) if per_env.shape[0] > 1 else np.zeros_like(mean)
    return mean, sd


def curve_axis(max_x_all: float, budget: float):
    """(max_x, G) of experiments.py:227-228: max_x = min(max_x_all, budget), G = int(ceil(max_x)) (at least one grid point here)."""
    max_x = min(float(max_x_all), float(budget))
    return max_x, max(1, int(np.ceil(max_x)))


# ----------------------------------------------------------------------------------------------- the device policies
class _VecBaseline:
    KIND = None
    UNIFORM_SHAPE = None  # per decision and env

    def __init__(self, env, uniforms=None):
        if not getattr(env, "budget_mode", False) or not hasattr(env, "prev"):
            raise TypeError("env must be a budget-mode VecIPPEnv (VecIPPEnv(budget=...))")
        torch = env.torch
        self.env, self.cfg, self.torch = env, env.cfg, torch
        B, dev = env.num_envs, env.device
        self.cursor = torch.zeros(B, dtype=torch.int32, device=dev)
        self.seen_episode = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.decision = torch.zeros(B, dtype=torch.int64, device=dev)
        self.start_budget = torch.zeros(B, dtype=torch.float64, device=dev)
        self.action = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        self.has = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.uniforms = None
        if uniforms is not None:
            if self.UNIFORM_SHAPE is None:
                raise ValueError("this baseline draws nothing")
            u = uniforms if isinstance(uniforms, torch.Tensor) else torch.as_tensor(np.asarray(uniforms, dtype=np.float64))
            u = u.to(device=dev, dtype=torch.float64).contiguous()
            if tuple(u.shape[1:]) != (B,) + self.UNIFORM_SHAPE:
                raise ValueError(f"uniforms: shape [decisions, {B}{''.join(', %d' % s for s in self.UNIFORM_SHAPE)}] expected, got {tuple(u.shape)}")
            self.uniforms = u
        self.calls = 0
        d = _ffi.IppBaseline()
        d.n, d.kind, d.device = B, self.KIND, dev.index or 0
        d.use_flight_time = 1 if env.use_flight_time else 0
        d.max_v, d.max_a = float(self.cfg.max_v), float(self.cfg.max_a)
        d.resolution = float(self.cfg.resolution)
        d.seed, d.row_offset = int(env.seed) & (2 ** 64 - 1), int(env.env_id_offset)
        d.prev, d.budget, d.episode = env.prev.data_ptr(), env.budget.data_ptr(), env.episode.data_ptr()
        d.cursor, d.seen_episode, d.decision = self.cursor.data_ptr(), self.seen_episode.data_ptr(), self.decision.data_ptr()
        d.start_budget, d.action, d.has = self.start_budget.data_ptr(), self.action.data_ptr(), self.has.data_ptr()
        self._desc = d

    def _dev64(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=self.env.device)

    def act(self):
        """One decision per env: ([B, 3] waypoints, has_action [B]); the waypoints are the policy's own buffer, overwritten by the next
        call.  An env without an action keeps its waypoint and its budget is set to 0, so that the next budget step ends its episode."""
        d = self._desc
        if self.uniforms is not None:
            if self.calls >= int(self.uniforms.shape[0]):
                raise ValueError(f"uniforms for {int(self.uniforms.shape[0])} decisions only")
            d.uniforms = self.uniforms[self.calls].data_ptr()
        stream = C.c_void_p(self.torch.cuda.current_stream(self.env.device).cuda_stream)
        _ffi.check(_ffi.load().ipp_baseline_act(C.byref(d), stream))
        self.calls += 1
        return self.action, self.has.bool()

    def run(self, steps: int, trace: Optional[list] = None, log=None, auto_reset: Optional[bool] = None):
        """`steps` times act() then env.step(actions).  trace: a list that receives per step the device tensors (budget before,
        waypoints before, actions, has_action, reward, done after the step).  log: a MissionLog that receives every executed step (and
        the step-0 point before the first one).  auto_reset: the env's reset inside the step launch; by default on without a log and
        OFF with one -- such a reset replaces the map before the step's metrics are taken, so the last point of every episode would
        carry the fresh map's metrics -- and asking for both is refused."""
        env = self.env
        if auto_reset is None:
            auto_reset = log is None
        elif auto_reset and log is not None:
            raise ValueError("run(log=...) steps without the in-launch reset: auto_reset=True would log a reset map's metrics")
        if log is not None and not log.started:
            log.record(first=True)
        for _ in range(int(steps)):
            keep = trace is not None or log is not None
            prev_before = env.prev.clone() if keep else None
            before = env.budget.clone() if trace is not None else None
            actions, has = self.act()
            env.step(actions, auto_reset=auto_reset)
            if log is not None:
                log.record(prev_before, actions, has)
            if trace is not None:
                trace.append((before, prev_before, actions.clone(), has.clone(), env.reward.clone(), env.done.clone()))
        return env.reward


class _VecTablePolicy(_VecBaseline):
    def _install(self, table: np.ndarray):
        self.table_host = table
        self.table = self._dev64(table)
        self._desc.table, self._desc.table_len = self.table.data_ptr(), int(table.shape[0])


class VecLawnmowerPolicy(_VecTablePolicy):
    """LawnMowerMission for a batch: the rows of lawnmower_table while budget >= step_size and budget > cost(next, current)."""
    KIND = _ffi.IPP_BASELINE_LAWNMOWER

    def __init__(self, env, dist_to_boundaries: float = 10, min_altitude: float = 5, max_altitude: float = 30, step_size: float = 5,
                 altitude_spacing: float = 5):
        super().__init__(env)
        if not (step_size > 0 and altitude_spacing > 0 and max_altitude >= min_altitude):
            raise ValueError("need step_size > 0, altitude_spacing > 0 and max_altitude >= min_altitude")
        self.step_size = float(step_size)
        self._desc.step_size = self.step_size
        self._install(lawnmower_table(self.cfg.x_dim, self.cfg.y_dim, self.cfg.resolution, dist_to_boundaries, min_altitude, max_altitude,
                                      step_size, altitude_spacing))


class VecSpiralPolicy(_VecTablePolicy):
    """ConicalSpiralMission for a batch: the rows of spiral_table; the first is flown whatever it costs, a later one while
    budget - cost(next, current) >= 0."""
    KIND = _ffi.IPP_BASELINE_SPIRAL

    def __init__(self, env, dist_to_boundaries: float = 10, min_altitude: float = 5, max_altitude: float = 30, num_waypoints: int = 200,
                 slope_factor: float = 10):
        super().__init__(env)
        if int(num_waypoints) < 2:
            raise ValueError("num_waypoints < 2")
        self._install(spiral_table(self.cfg.x_dim, self.cfg.y_dim, self.cfg.resolution, dist_to_boundaries, min_altitude, max_altitude,
                                   int(num_waypoints), slope_factor))


class VecRandomDiscretePolicy(_VecBaseline):
    """RandomDiscreteMission for a batch: a uniform draw among the cell-centre actions get_next_actions_mask admits.  uniforms:
    [decisions, B] in [0, 1), or None for Philox.  dist_to_boundaries is accepted and unused, as in the reference."""
    KIND = _ffi.IPP_BASELINE_RANDOM_DISCRETE
    UNIFORM_SHAPE = ()

    def __init__(self, env, dist_to_boundaries: float = 10, min_altitude: float = 5, max_altitude: float = 30, altitude_spacing: float = 5,
                 adaptive: bool = False, uniforms=None):
        super().__init__(env, uniforms)
        if self.cfg.x_dim != self.cfg.y_dim:
            raise ValueError("random discrete baseline: square grids only (enumerate_actions' index)")
        if not (altitude_spacing > 0 and max_altitude >= min_altitude):
            raise ValueError("need altitude_spacing > 0 and max_altitude >= min_altitude")
        self.adaptive = bool(adaptive)
        self.levels_host = altitude_linspace(min_altitude, max_altitude, altitude_spacing)
        self.levels = self._dev64(self.levels_host)
        d = self._desc
        d.grid_w, d.grid_h, d.n_levels, d.adaptive = self.cfg.x_dim, self.cfg.y_dim, len(self.levels_host), 1 if adaptive else 0
        d.levels = self.levels.data_ptr()


class VecRandomContinuousPolicy(_VecBaseline):
    """RandomContinuousMission for a batch: up to 101 uniform trial waypoints in the reference's box, the first affordable one.
    uniforms: [decisions, B, 101, 3] in [0, 1), or None for Philox."""
    KIND = _ffi.IPP_BASELINE_RANDOM_CONTINUOUS
    UNIFORM_SHAPE = (TRIALS, 3)

    def __init__(self, env, dist_to_boundaries: float = 10, min_altitude: float = 5, max_altitude: float = 30, uniforms=None):
        super().__init__(env, uniforms)
        self.low, self.high = continuous_box(self.cfg.x_dim, self.cfg.y_dim, self.cfg.resolution, dist_to_boundaries, min_altitude,
                                             max_altitude)
        if not np.all(self.high >= self.low):
            raise ValueError("dist_to_boundaries / altitudes leave an empty box")
        for c in range(3):
            self._desc.low[c], self._desc.high[c] = float(self.low[c]), float(self.high[c])
