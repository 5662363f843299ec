"""
Classic MCTS with rollouts for a whole batch of envs (the reference's planning/mcts_mission.py MCTSMission.replan per env of a VecIPPEnv;
the batched counterpart of planning/mcts_mission.py::ClassicMCTS.execute): the learned planner's main baseline beside VecGreedyPolicy,
VecCmaesPolicy and VecMctsZeroPolicy.

One decision = ClassicMCTS(batched=True).replan with the env slots as roots -- every round of the lock-step search answers all pending
rollouts with one DeviceRollout.run and all pending candidate scorings with one ipp_tree_score_nodes call -- then env.step.  The tree
(UCT, progressive widening, backup) lives on the host, so a decision starts with ONE host read of the envs' budgets and waypoints; the
env states themselves never leave the device and are not written by the search.

tree="device": the tree lives in device tables as well (planning/device_ctree.py, csrc/k_ctree.h) and a decision reads nothing from the
device: budgets and waypoints go in as env.budget / env.prev, the uniforms of a decision come from one NumPy stream per (seed,
decision, env) and are uploaded once.  The two trees consume their random numbers differently: for one seed they do not decide alike.
"""
from typing import Optional

import numpy as np

from .device_ctree import DeviceClassicMCTS
from .mcts_mission import ClassicMCTS


class VecMctsPolicy:
    def __init__(self, env, min_altitude: float, max_altitude: float, altitude_spacing: float, num_simulations: int = 100,
                 gamma: float = 0.95, c: float = 2.0, episode_horizon: int = 5, k: float = 4.0, alpha: float = 0.75,
                 epsilon_expand: float = 0.2, epsilon_rollout: float = 0.5, max_greedy_radius: float = 3, use_gcb_rollout: bool = False,
                 seed: int = 0, tree: str = "host"):
        """env: a budget-mode VecIPPEnv (patch layout) built with node_capacity >= num_envs x (num_simulations + episode_horizon);
        the other arguments are MCTSMission's.  seed: decision t of env e searches with NumPy seed and tie seed derived from
        (seed, t, e), so two policies with the same seed on equal envs decide alike.  tree: "host" (ClassicMCTS(batched=True)) or
        "device" (DeviceClassicMCTS: act() reads nothing from the device; check() is the optional read of the searches' error flags)."""
        if tree not in ("host", "device"):
            raise ValueError(f"tree = {tree!r}: 'host' or 'device'")
        if not hasattr(env, "score_actions") or not hasattr(env, "prev"):
            raise TypeError("env must be a VecIPPEnv")
        if not getattr(env, "budget_mode", False):
            raise ValueError("VecMctsPolicy needs a budget-mode VecIPPEnv (budget=...)")
        eng = env.engine
        if int(eng.info.patch_layout) != 1 or int(eng._c.node_capacity) <= 0:
            raise ValueError("VecMctsPolicy needs a patch-layout engine with node_capacity > 0 (VecIPPEnv(node_capacity=...))")
        need = env.num_envs * (int(num_simulations) + int(episode_horizon))
        if int(eng._c.node_capacity) < need:
            raise ValueError(f"node_capacity {int(eng._c.node_capacity)} < {need} = num_envs x (num_simulations + episode_horizon)")
        self.env, self.cfg, self.seed = env, env.cfg, int(seed)
        uav = {"max_v": float(self.cfg.max_v), "max_a": float(self.cfg.max_a)} if env.use_flight_time else None
        self.tree = tree
        kw = dict(num_simulations=num_simulations, gamma=gamma, c=c, episode_horizon=episode_horizon, k=k, alpha=alpha,
                  epsilon_expand=epsilon_expand, epsilon_rollout=epsilon_rollout, max_greedy_radius=max_greedy_radius,
                  use_gcb_rollout=use_gcb_rollout, adaptive=env.adaptive, batched=True)
        if tree == "device":
            self.mcts = DeviceClassicMCTS(eng, self.cfg, uav, min_altitude, max_altitude, altitude_spacing, roots=env.num_envs, **kw)
            self._slots = env.torch.arange(env.num_envs, dtype=env.torch.int32, device=env.device)
        else:
            self.mcts = ClassicMCTS(eng, self.cfg, uav, min_altitude, max_altitude, altitude_spacing, **kw)
        self.decisions = 0
        self.last = None  # (budget before [B] host, has_action [B] device, roots) of the last act()

    def act(self):
        """One search per env: ([B, 3] waypoints, has_action [B]) on the device.  An env whose search has no best child (no budget
        for any action) keeps its waypoint and its budget is set to 0, so that the next budget step ends its episode."""
        env, torch = self.env, self.env.torch
        B = env.num_envs
        if self.tree == "device":
            return self._act_device()
        state = torch.cat([env.budget[:, None], env.prev], dim=1).cpu().numpy()  # the one host read the host tree needs
        budget, prev = state[:, 0], state[:, 1:]
        mcts = self.mcts
        mcts.pool.clear()
        t = self.decisions
        searches = []
        for e in range(B):
            s = mcts.new_search(e, prev[e].copy(), float(budget[e]), 0, (self.seed * 1000003 + t) * 4099 + e)
            s.np_rng = np.random.RandomState(((self.seed * 1000003 + t) * 4099 + e) % (2 ** 32))
            searches.append(s)
        roots = mcts.run(searches)
        best = [ClassicMCTS.select_best_child(r) for r in roots]
        has_host = np.array([b is not None for b in best])
        acts = np.array([b.action if b is not None else prev[e] for e, b in enumerate(best)], dtype=np.float64)
        actions = torch.as_tensor(acts, dtype=torch.float64, device=env.device)
        has = torch.as_tensor(has_host, device=env.device)
        env.budget.mul_(has.to(env.budget.dtype))
        self.decisions += 1
        self.last = (budget, has, roots)
        return actions, has

    def _act_device(self):
        """act() with the tree in device tables: no host read.  self.last = (budget before [B] device, has_action [B] device, None)."""
        from .device_ctree import uniform_tables

        env, mcts = self.env, self.mcts
        B, t = env.num_envs, self.decisions
        per_env = [uniform_tables(np.random.RandomState(((self.seed * 1000003 + t) * 4099 + e) % (2 ** 32)), mcts.num_simulations, 1,
                                  mcts.episode_horizon) for e in range(B)]
        uniforms = {name: np.concatenate([u[name] for u in per_env], axis=1) for name in ("tie", "expand", "rollout")}
        before = env.budget.clone()
        actions, has_i = mcts.search(self._slots, env.prev, env.budget, uniforms)
        actions, has = actions.clone(), has_i != 0
        env.budget.mul_(has.to(env.budget.dtype))
        self.decisions += 1
        self.last = (before, has, None)
        return actions, has

    def check(self) -> None:
        """tree="device": the one optional read of the last decision's error flags (DeviceClassicMCTS.check); raises on an error."""
        if self.tree == "device":
            self.mcts.check()

    def run(self, steps: int, trace: Optional[list] = None):
        """`steps` times act() then env.step(actions).  trace: a list that receives per step (budget before [B], has_action,
        actions, the step's status, the budget after, done after) -- device tensors but for the first with tree="host", a host array."""
        env = self.env
        for _ in range(int(steps)):
            actions, has = self.act()
            prev = env.prev.clone() if trace is not None else None
            env.step(actions)
            if trace is not None:
                trace.append((self.last[0], has.clone(), actions.clone(), env.status.clone(), env.budget.clone(), env.done.clone(), prev))
        return env.reward
