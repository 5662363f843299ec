"""
Greedy one-step planner for a whole batch of envs (the batched counterpart of planning/greedy.py; the reference's
planning/common/optimization.py:33-104 greedy_search and planning/greedy_mission.py loop, per env of a VecIPPEnv).

Every env's candidates are scored by ONE ipp_score_actions_envs call (csrc/k_score_batch.h; the library runs the predict-only step
launches for all n x k candidates itself).  Candidate construction, the budget filter of get_actions (planning/common/actions.py:63), the first-maximiser rule
(optimization.py:92-97) and the step run on the device; nothing in the loop reads the device from the host.

The host restatements below (candidate order, radius table, budget filter, first maximiser) run without a GPU.
"""
from typing import Optional

import numpy as np


# ----------------------------------------------------------------------------------------------- host restatements
def altitude_levels(min_altitude: float, max_altitude: float, altitude_spacing: float) -> np.ndarray:
    n = int((max_altitude - min_altitude) / altitude_spacing) + 1  # actions.py:54-55
    return min_altitude + altitude_spacing * np.arange(n)


def candidate_table(x_dim: int, y_dim: int, resolution: float, min_altitude: float, max_altitude: float,
                    altitude_spacing: float) -> np.ndarray:
    """[y_dim * x_dim * levels, 3] cell-centre waypoints in the order of get_actions (actions.py:56-62): row, column, level."""
    heights = altitude_levels(min_altitude, max_altitude, altitude_spacing)
    xs = resolution * np.arange(x_dim) + 0.5 * resolution
    ys = resolution * np.arange(y_dim) + 0.5 * resolution
    out = np.empty((y_dim, x_dim, len(heights), 3))
    out[..., 0] = xs[None, :, None]
    out[..., 1] = ys[:, None, None]
    out[..., 2] = heights[None, None, :]
    return out.reshape(-1, 3)


def radius_offsets(resolution: float, radius: float) -> np.ndarray:
    """[n_off, 2] (drow, dcol) of every cell that can hold a waypoint closer than `radius` to a point of the centre cell, row-major:
    the square of half-width ceil(radius / resolution) cells (the exact distance test runs per candidate)."""
    c = int(np.ceil(radius / resolution))
    d = np.arange(-c, c + 1)
    return np.stack(np.meshgrid(d, d, indexing="ij"), axis=-1).reshape(-1, 2)


def radius_candidates(position, x_dim: int, y_dim: int, resolution: float, min_altitude: float, max_altitude: float,
                      altitude_spacing: float, radius: float) -> np.ndarray:
    """[n_off * levels, 3] candidates around `position` in get_actions order; rows outside the grid or not closer than `radius`
    (3-D distance, planning/mcts_mission.py:169-173) are NaN."""
    position = np.asarray(position, dtype=np.float64)
    heights = altitude_levels(min_altitude, max_altitude, altitude_spacing)
    off = radius_offsets(resolution, radius)
    row = int(np.floor(position[1] / resolution)) + off[:, 0]
    col = int(np.floor(position[0] / resolution)) + off[:, 1]
    out = np.empty((len(off), len(heights), 3))
    out[..., 0] = (resolution * col + 0.5 * resolution)[:, None]
    out[..., 1] = (resolution * row + 0.5 * resolution)[:, None]
    out[..., 2] = heights[None, :]
    inside = (row >= 0) & (row < y_dim) & (col >= 0) & (col < x_dim)
    dist = np.linalg.norm(out - position, axis=-1)
    out[~(inside[:, None] & (dist < radius))] = np.nan
    return out.reshape(-1, 3)


def budget_filter(cost: np.ndarray, budget) -> np.ndarray:
    """get_actions' reachability test (actions.py:63): 0 < cost <= remaining budget (NaN costs fail both)."""
    cost = np.asarray(cost, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (cost > 0) & (cost <= np.asarray(budget, dtype=np.float64)[..., None])


def first_maximiser(reward: np.ndarray, valid: np.ndarray):
    """(index [n], has_action [n]): per row the FIRST valid candidate with the largest reward (optimization.py:92-97: a later
    candidate replaces the best only when strictly better; a NaN reward never does).  Rows without a valid candidate: index 0."""
    reward = np.asarray(reward, dtype=np.float64)
    ok = np.asarray(valid, dtype=bool) & ~np.isnan(reward)
    score = np.where(ok, reward, -np.inf)
    has = ok.any(axis=-1)
    best = score.max(axis=-1, keepdims=True)
    k = score.shape[-1]
    idx = np.where(ok & (score == best), np.arange(k), k).min(axis=-1)
    return np.where(has, idx, 0), has


# ----------------------------------------------------------------------------------------------- the device policy
class VecGreedyPolicy:
    def __init__(self, env, min_altitude: float, max_altitude: float, altitude_spacing: float, radius: Optional[float] = None):
        """env: a VecIPPEnv on a patch-layout engine.  radius: only waypoints closer than `radius` metres to the env's current
        waypoint (the reference's max_greedy_radius), built per env on the device from a fixed offset table around its cell."""
        if not (altitude_spacing > 0) or not (max_altitude >= min_altitude):
            raise ValueError("altitude levels: need altitude_spacing > 0 and max_altitude >= min_altitude")
        if radius is not None and not (radius > 0):
            raise ValueError("radius must be positive")
        if not hasattr(env, "score_actions") or not hasattr(env, "prev"):
            raise TypeError("env must be a VecIPPEnv")
        self.env = env
        self.cfg = env.cfg
        self.min_altitude, self.max_altitude, self.altitude_spacing = float(min_altitude), float(max_altitude), float(altitude_spacing)
        self.radius = None if radius is None else float(radius)
        self.heights = altitude_levels(self.min_altitude, self.max_altitude, self.altitude_spacing)
        self.last = None  # (reward, cost, status, index, has_action) of the last act()
        self._table = None
        self._off = None

    @property
    def num_candidates(self) -> int:
        cells = self.cfg.x_dim * self.cfg.y_dim if self.radius is None else len(radius_offsets(self.cfg.resolution, self.radius))
        return cells * len(self.heights)

    def candidates(self, prev):
        """[n, k, 3] device candidates for the waypoints prev [n, 3] (NaN rows = no candidate)."""
        torch = self.env.torch
        dev = self.env.device
        cfg = self.cfg
        n = int(prev.shape[0])
        if self.radius is None:
            if self._table is None:
                self._table = torch.as_tensor(candidate_table(cfg.x_dim, cfg.y_dim, cfg.resolution, self.min_altitude, self.max_altitude,
                                                              self.altitude_spacing), dtype=torch.float64, device=dev)
            return self._table.unsqueeze(0).expand(n, -1, -1).contiguous()
        if self._off is None:
            off = radius_offsets(cfg.resolution, self.radius)
            self._off = (torch.as_tensor(off[:, 0], dtype=torch.float64, device=dev), torch.as_tensor(off[:, 1], dtype=torch.float64, device=dev),
                         torch.as_tensor(self.heights, dtype=torch.float64, device=dev))
        drow, dcol, heights = self._off
        res = float(cfg.resolution)
        row = torch.floor(prev[:, 1] / res)[:, None] + drow[None, :]
        col = torch.floor(prev[:, 0] / res)[:, None] + dcol[None, :]
        L = heights.numel()
        out = torch.empty((n, drow.numel(), L, 3), dtype=torch.float64, device=dev)
        out[..., 0] = (res * col + 0.5 * res)[:, :, None]
        out[..., 1] = (res * row + 0.5 * res)[:, :, None]
        out[..., 2] = heights[None, None, :]
        inside = (row >= 0) & (row < cfg.y_dim) & (col >= 0) & (col < cfg.x_dim)
        dist = torch.linalg.vector_norm(out - prev[:, None, None, :], dim=-1)
        keep = inside[:, :, None] & (dist < self.radius)
        out = torch.where(keep[..., None], out, torch.full_like(out, float("nan")))
        return out.reshape(n, -1, 3)

    def _pick(self, cands, reward, cost, budget):
        """First maximiser among the candidates with 0 < cost <= budget, on the device."""
        torch = self.env.torch
        valid = (cost > 0) & ~torch.isnan(reward)
        if budget is not None:
            valid &= cost <= budget[:, None]
        score = torch.where(valid, reward.to(torch.float64), torch.full_like(cost, float("-inf")))
        has = valid.any(dim=1)
        best = score.max(dim=1, keepdim=True).values
        k = score.shape[1]
        ar = torch.arange(k, device=score.device)
        idx = torch.where(valid & (score == best), ar[None, :], torch.full_like(ar, k)[None, :]).min(dim=1).values
        idx = torch.where(has, idx, torch.zeros_like(idx))
        chosen = cands[torch.arange(cands.shape[0], device=cands.device), idx]
        return chosen, idx, has

    def act(self):
        """One greedy decision per env: ([B, 3] waypoints, has_action [B]).  An env without a reachable candidate keeps its waypoint
        and its budget is set to 0, so that the next budget step ends its episode."""
        env, torch = self.env, self.env.torch
        prev = env.prev
        cands = self.candidates(prev)
        reward, status, cost = env.score_actions(cands, want_cost=True)
        budget = env.budget if getattr(env, "budget_mode", False) else None
        chosen, idx, has = self._pick(cands, reward, cost, budget)
        actions = torch.where(has[:, None], chosen, prev)
        if budget is not None:
            budget.mul_(has.to(budget.dtype))
        self.last = (reward, cost, status, idx, has)
        return actions, has

    def run(self, steps: int, trace: Optional[list] = None):
        """`steps` times act() then env.step(actions).  trace: a list that receives per step the device tensors
        (budget before, reward, cost, index, has_action, actions, done after the step)."""
        env = self.env
        for _ in range(int(steps)):
            before = env.budget.clone() if (trace is not None and getattr(env, "budget_mode", False)) else None
            actions, has = self.act()
            env.step(actions)
            if trace is not None:
                reward, cost, status, idx, _ = self.last
                done = env.done.clone() if getattr(env, "budget_mode", False) else None
                trace.append((before, reward, cost, idx.clone(), has.clone(), actions.clone(), done))
        return env.reward

    def search(self, env_ids, scratch_ids, budget, horizon: int):
        """greedy_search with a look-ahead of `horizon` waypoints for the envs `env_ids` (optimization.py:33-104): their states are
        forked to the slots `scratch_ids`, every level scores from the look-ahead state and commits the winner there as a
        covariance-only step (the adaptive mask keeps the env's mean).  budget: [n] remaining budgets.  Returns
        (waypoints [n, horizon, 3], valid [n, horizon]); the envs themselves are not written."""
        env, torch = self.env, self.env.torch
        eng = env.engine
        def dev(x, dtype):  # (device tensors pass through: a caller that holds them does not read them back)
            if isinstance(x, torch.Tensor):
                return x.to(device=env.device, dtype=dtype)
            return torch.as_tensor(np.asarray(x), dtype=dtype, device=env.device)

        ids, sids = dev(env_ids, torch.int32), dev(scratch_ids, torch.int32)
        eng.fork(ids, sids)
        prev = env.prev[ids.long()].clone()
        left = dev(budget, torch.float64).clone()
        alive = torch.ones(ids.numel(), dtype=torch.bool, device=env.device)
        ways, valids = [], []
        for _ in range(int(horizon)):
            cands = self.candidates(prev)
            reward, status, cost = eng.score_actions_envs(cands, prev, env_ids=sids, adaptive=env.adaptive,
                                                          use_flight_time=env.use_flight_time, want_cost=True)
            chosen, idx, has = self._pick(cands, reward, cost, left)
            alive = alive & has
            step_to = torch.where(alive[:, None], chosen, torch.full_like(chosen, float("nan")))  # (a NaN action: nothing is applied)
            eng.step(step_to, prev, env_ids=sids, cov_only=True, adaptive=env.adaptive, use_flight_time=env.use_flight_time)
            spent = cost[torch.arange(cost.shape[0], device=cost.device), idx]
            left = torch.where(alive, left - spent, left)
            prev = torch.where(alive[:, None], chosen, prev)
            ways.append(torch.where(alive[:, None], chosen, torch.full_like(chosen, float("nan"))))
            valids.append(alive)
        return torch.stack(ways, dim=1), torch.stack(valids, dim=1)
