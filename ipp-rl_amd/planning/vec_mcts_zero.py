"""
The learned planner for a whole batch of envs: MCTSZeroMission.execute / replan (planning/mcts_zero/mcts_zero_mission.py:469-523, 607-652)
and the players of the arena gate (evaluate_trained_agent, :417-455; Arena.play_game, planning/mcts_zero/arenas.py:25-45) on the device --
the batched counterpart of VecGreedyPolicy / VecCmaesPolicy, the two baselines it is compared with.

One VecMctsZeroPolicy.step() is one decision of every env:

    search    DeviceMCTS.search_device for B x workers roots (root e workers + w = worker w of env e: `num_workers` root-parallel
              searches per decision, :504-510, all reading env slot e), read out at temperature 1
                  deploy  deploy_time=True  (run_deploy_time_mcts_worker, :36-55)
                  arena   deploy_time=False with the policy's tie uniforms: get_policy(temperature=0), :421-427
    pick      the workers' policies summed, normalised, arg-max (:516-523); deploy: the first maximiser (np.argmax), arena: the
              temperature-0 choice among equal maxima (mcts.py:134-138) by the draw SelfPlay's record makes         (ipp_play_pick)
    step      VecIPPEnv.step: the fused budget step, episode ends and resets in the same launch
    tally     total_reward += gamma ** depth * reward (arenas.py:38), the games that ended, the next tie uniform     (ipp_play_tally)
    totals    the arena's sums over the counted games into pinned memory: the step's one small read                   (ipp_play_totals)

The host restatements below (ensemble_pick_host, tally_host, totals_host, gate) run without a GPU and are the oracles of the GPU tests.
Divergences from the reference: INTEGRATION.md "Deployment and arena".
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional

import numpy as np

from .. import _ffi

MAX_KMAX = 2048  # widest valid set the pick kernel holds in LDS (csrc/k_selfplay.h kSpMaxK)
MODES = {"deploy": 0, "arena": 1}  # -> ipp_play.tie_rule


# ---------------------------------------------------------------------------------------------------- host restatements
def ensemble_pick_host(policy, valid_idx, ok, tie_rule: int = 0, u: float = 0.0, num_actions: Optional[int] = None):
    """ipp_play_pick for ONE env: policy [workers, kmax], valid_idx [workers, kmax] (-1 padded), ok [workers].  The decision of replan
    (mcts_zero_mission.py:516-523) on the sparse rows, in the kernel's order: total[k] = the workers with ok, in worker order; the sum
    over k sequentially in ascending k; ensemble = total / sum; a maximiser: tie_rule 0 the first (np.argmax), tie_rule 1 number
    min(floor(u n_ties), n_ties - 1) of the maxima in ascending action order (u: the env's IPP_SP_ARGMAX_STREAM uniform).
    Returns dict(action_idx, forced, ensemble [kmax], slot); forced (no worker ok, a NaN, a sum or maximum that is not positive and
    finite, a chosen index >= num_actions): action_idx -1, ensemble zeros, slot -1."""
    policy = np.asarray(policy, dtype=np.float64)
    valid_idx = np.asarray(valid_idx, dtype=np.int64)
    ok = np.asarray(ok).reshape(-1) != 0
    W, K = policy.shape
    none = dict(action_idx=-1, forced=1, ensemble=np.zeros(K), slot=-1)
    if not ok.any():
        return none
    vi = valid_idx[int(np.nonzero(ok)[0][0])]
    valid = vi >= 0
    total = np.zeros(K)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(W):
            if ok[w]:
                total = np.where(valid, total + policy[w], total)
        tot = 0.0
        for k in np.nonzero(valid)[0]:
            tot = tot + float(total[k])
        if np.isnan(total).any() or not (tot > 0.0) or not (tot < np.inf):
            return none
        ens = np.where(valid, total / tot, 0.0)
    if not valid.any():
        return none
    vmax = ens[valid].max()
    if not (vmax > 0.0) or vmax == np.inf:
        return none
    ties = np.nonzero(valid & (ens == vmax))[0]
    pick = 0 if int(tie_rule) == 0 else min(int(float(u) * len(ties)), len(ties) - 1)
    slot = int(ties[pick])
    a = int(vi[slot])
    if num_actions is not None and a >= int(num_actions):
        return none
    return dict(action_idx=a, forced=0, ensemble=ens, slot=slot)


def tally_host(rewards, done, forced, gamma: float, games_per_env: int = 1):
    """ipp_play_tally for ONE env over a sequence of steps (rewards, done, forced: one entry per step): a step that is not forced adds
    gamma ** steps * reward (arenas.py:38) and counts; a step that ends the episode (done or forced) stores the game while fewer than
    games_per_env are stored, and starts the next one.  Returns dict(game_value, game_steps (lists), games, ret, steps)."""
    ret, steps = 0.0, 0
    values, lengths = [], []
    for r, d, f in zip(rewards, done, forced):
        if not f:
            ret += float(gamma) ** steps * float(r)
            steps += 1
        if f or d:
            if len(values) < int(games_per_env):
                values.append(ret)
                lengths.append(steps)
            ret, steps = 0.0, 0
    return dict(game_value=values, game_steps=lengths, games=len(values), ret=ret, steps=steps)


def totals_host(game_value, game_steps, games) -> np.ndarray:
    """ipp_play_totals: [sum of the counted game values, counted games, sum of their steps, envs with all their games] in the kernel's
    order -- item i = e G + g goes to partial sum i % 64 (ascending i within it), the 64 partial sums are added in order.  For up to
    64 items that is the plain sum in (env, game) order."""
    gv = np.asarray(game_value, dtype=np.float64)
    gs, games = np.asarray(game_steps, dtype=np.int64), np.asarray(games, dtype=np.int64).reshape(-1)
    B, G = gv.shape
    part = [0.0] * 64
    count = steps = 0
    for i in range(B * G):
        e, g = divmod(i, G)
        if g < games[e]:
            part[i % 64] += float(gv[e, g])
            steps += int(gs[e, g])
            count += 1
    tot = 0.0
    for x in part:
        tot += x
    return np.array([tot, float(count), float(steps), float(int((games >= G).sum()))])


def gate(total_prev: float, total_curr: float, threshold: float):
    """(accepted, ratio) of evaluate_trained_agent (mcts_zero_mission.py:435-436): ratio = curr / (prev + curr), and the new network is
    rejected exactly when ratio < threshold (so a NaN ratio, 0 / 0, rejects nothing, as there)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(total_curr) / (np.float64(total_prev) + np.float64(total_curr)))
    return (not ratio < float(threshold)), ratio


def valid_set_width(cfg, hyper_params: Dict, meta_data: Dict) -> int:
    """kmax of DeviceMCTS for this grid: every cell within ceil(max_valid_action_distance / resolution) + 1 cells at every altitude
    level, at most the whole action set (vector_mcts.py; actions.py:54-55 for the levels)."""
    levels = int((float(meta_data["max_altitude"]) - float(meta_data["min_altitude"])) / float(meta_data["altitude_spacing"])) + 1
    k = int(np.ceil(float(hyper_params["max_valid_action_distance"]) / float(cfg.resolution))) + 1
    return int(min((2 * k + 1) ** 2 * levels, cfg.x_dim * cfg.y_dim * levels))


def check_args(env, hyper_params: Dict, meta_data: Dict, workers: int, mode: str, games_per_env: int, sims_in_flight: int):
    """What VecMctsZeroPolicy cannot run, refused before anything touches the device.  Returns (roots, simulations, kmax)."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'deploy' or 'arena', not {mode!r}")
    if not getattr(env, "budget_mode", False) or not hasattr(env, "prev") or not hasattr(env, "engine"):
        raise TypeError("env must be a budget-mode VecIPPEnv (VecIPPEnv(budget=...)): the decision ends an episode through its ledger")
    if int(workers) < 1:
        raise ValueError(f"workers = {workers}: at least 1 search per decision")
    if int(games_per_env) < 1:
        raise ValueError(f"games_per_env = {games_per_env}: at least 1")
    if int(sims_in_flight) < 1:
        raise ValueError(f"sims_in_flight = {sims_in_flight}: at least 1")
    if not hyper_params.get("reset_mcts_each_step", True):
        raise ValueError("reset_mcts_each_step=False (tree reuse across steps) is not supported")
    sims = int(hyper_params["num_mcts_simulations"])
    if sims <= 0:
        raise ValueError(f"num_mcts_simulations = {sims}: the network-only decision (mcts_zero_mission.py:478-502) needs the roots' "
                         f"valid sets outside a search and is out of scope; at least 1 simulation is needed")
    eng = env.engine
    if int(eng.info.patch_layout) != 1:
        raise ValueError("patch-layout engines only (ipp_info.patch_layout == 1)")
    R = int(env.num_envs) * int(workers)
    if int(eng.max_batch) < R * int(sims_in_flight):
        raise ValueError(f"the engine's max_batch = {int(eng.max_batch)}: {env.num_envs} envs x {workers} workers x {sims_in_flight} "
                         f"simulations in flight need max_batch >= {R * int(sims_in_flight)}")
    need = R * (sims + 16)
    if int(eng._c.node_capacity) < need:
        raise ValueError(f"the engine's node_capacity = {int(eng._c.node_capacity)}: {env.num_envs} envs x {workers} workers x "
                         f"({sims} simulations + 16) need node_capacity >= {need}")
    kmax = valid_set_width(env.cfg, hyper_params, meta_data)
    if kmax > MAX_KMAX:
        raise ValueError(f"valid-action sets of up to {kmax} actions (max_valid_action_distance "
                         f"{hyper_params['max_valid_action_distance']}): the pick holds at most {MAX_KMAX}")
    return R, sims, kmax


def make_env(cfg, num_envs: int, hyper_params: Dict, meta_data: Dict, workers: int = 1, sims_in_flight: int = 4, seed: int = 0,
             env_id_offset: int = 0, device: str = "cuda:0", **env_kwargs):
    """A budget-mode VecIPPEnv for VecMctsZeroPolicy with the defaults SelfPlay sets (window_rows, adaptive, use_flight_time, rank_cap,
    feature_history = input_history_length) and node_capacity / max_batch sized for num_envs x workers roots.  env_kwargs override."""
    from ..vec_env import VecIPPEnv

    hp, md, B = hyper_params, meta_data, int(num_envs)
    if md.get("initial_budget") is None:
        raise ValueError("budget-mode episodes: meta_data['initial_budget'] is needed")
    steps = int(md.get("max_episode_steps", hp.get("max_episode_steps", 0)))
    horizon, sims = int(md["episode_horizon"]), int(hp["num_mcts_simulations"])
    kw = dict(env_kwargs)
    kw.setdefault("window_rows", -1)
    kw.setdefault("adaptive", md.get("scenario_info") is not None)
    kw.setdefault("use_flight_time", md.get("uav_specifications") is not None)
    kw.setdefault("node_capacity", B * int(workers) * (max(sims, 0) + 16))
    kw.setdefault("max_batch", B * int(workers) * int(sims_in_flight))
    kw.setdefault("rank_cap", 9 * (steps + horizon + 2))  # (a search adds up to horizon + 1 steps of columns to a root)
    return VecIPPEnv(cfg, B, episode_steps=steps, device=device, seed=int(seed), env_id_offset=int(env_id_offset),
                     budget=float(md["initial_budget"]), shuffle_budget=bool(hp.get("shuffle_budget", False)),
                     feature_history=int(hp["input_history_length"]), **kw)


# ---------------------------------------------------------------------------------------------------- the device policy
class VecMctsZeroPolicy:
    def __init__(self, env, hyper_params: Dict, meta_data: Dict, infer: Optional[Callable] = None, workers: Optional[int] = None,
                 mode: str = "deploy", games_per_env: int = 1, sims_in_flight: int = 4, tie_break: str = "first", groups: int = 2,
                 seed: Optional[int] = None):
        """env: a budget-mode VecIPPEnv on a patch-layout engine whose max_batch holds num_envs x workers x sims_in_flight items and
        whose node_capacity holds num_envs x workers x (num_mcts_simulations + 16) nodes (with a network: feature_history =
        input_history_length).  hyper_params / meta_data: the reference's dictionaries, as for SelfPlay.  infer: DeviceMCTS's network
        callback (None: uniform priors, value 0).  workers: searches per decision (default hyper_params['num_workers'], 1 without it).
        mode: 'deploy' (replan) or 'arena' (the temperature-0 player of evaluate_trained_agent).  games_per_env: episodes counted per
        env.  seed: of the search's and the pick's draws (default the env's)."""
        workers = int(hyper_params.get("num_workers", 1) if workers is None else workers)
        R, sims, kmax = check_args(env, hyper_params, meta_data, workers, mode, games_per_env, sims_in_flight)
        from .mcts_zero.device_mcts import DeviceMCTS

        torch = self.torch = env.torch
        self.env, self.mode, self.workers = env, mode, workers
        hp, md = dict(hyper_params), dict(meta_data)
        md.setdefault("budget", md.get("initial_budget", env.initial_budget))
        self.hp, self.md = hp, md
        B = self.num_envs = int(env.num_envs)
        self.games_per_env = G = int(games_per_env)
        self.seed = int(env.seed if seed is None else seed)
        self.max_episode_steps = int(env.episode_steps)
        self.infer = infer
        self.device = dev = env.device
        self.mcts = DeviceMCTS(env.engine, hp, md, infer, sims_in_flight=int(sims_in_flight), tie_break=tie_break, seed=self.seed,
                               groups=groups, dev_per_root=max(1, int(env.engine._c.node_capacity) // R), feature_planes=infer is not None)
        self.mcts._key_base = env.env_id_offset * workers  # (root e workers + w of a shard has the key it has in the whole run)
        geo = self.mcts._geometry(torch, dev)
        self.kmax, self.num_actions = int(geo["kmax"]), int(self.mcts.num_actions)
        if self.kmax != kmax:
            raise RuntimeError(f"valid-set width {self.kmax} of the search differs from the grid's {kmax}")
        self.actions = geo["actions"]
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.ret, self.steps, self.games = z((B,), torch.float64), z((B,), torch.int32), z((B,), torch.int32)
        self.forced, self.tie_u = z((B,), torch.uint8), z((B,), torch.float64)
        self.action, self.action_idx = z((B, 3), torch.float64), z((B,), torch.int32)
        self.game_values, self.game_steps = z((B, G), torch.float64), z((B, G), torch.int32)
        self.ensemble = z((B, self.kmax), torch.float64)
        self._totals = z((4,), torch.float64)
        self._totals_host = torch.zeros((4,), dtype=torch.float64).pin_memory()
        self._totals_ev = torch.cuda.Event()
        self._roots = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(workers)
        self._lib = env.engine._lib
        pl = self._pl = _ffi.IppPlay(num_envs=B, workers=workers, kmax=self.kmax, num_actions=self.num_actions, games_per_env=G,
                                     tie_rule=MODES[mode], device=dev.index or 0, reserved=0, gamma=float(hp["gamma"]),
                                     seed=self.seed & (2 ** 64 - 1), row_offset=env.env_id_offset)
        ptrs = dict(actions=self.actions, budget=env.budget, depth=env.depth, episode=env.episode, done=env.done, prev=env.prev,
                    reward=env.reward, ret=self.ret, steps=self.steps, games=self.games, forced=self.forced, tie_u=self.tie_u,
                    action=self.action, action_idx=self.action_idx, game_value=self.game_values, game_steps=self.game_steps,
                    ensemble=self.ensemble)
        for name, t in ptrs.items():
            setattr(pl, name, t.data_ptr())
        self.t = 0
        self.last = None
        self.totals = np.zeros(4)  # (sum of the counted game values, counted games, their steps, envs with all their games) after step()
        self.timing = None  # dict phase -> list of events while profiling (tools/deploy_bench.py)
        self.reset()

    # ------------------------------------------------------------------
    def reset(self):
        """Every env starts its next episode (the env's reset) at Mission.init_action; the game lists are emptied."""
        from .mcts_zero.selfplay import TIE_STREAM, step_uniform

        torch, env, B = self.torch, self.env, self.num_envs
        env.reset()
        gid = np.arange(B, dtype=np.int64) + env.env_id_offset
        self.tie_u.copy_(torch.as_tensor(step_uniform(TIE_STREAM, self.seed, gid, env.episode.cpu().numpy(), env.depth.cpu().numpy()),
                                         device=self.device))
        for t in (self.ret, self.steps, self.games, self.forced, self.game_values, self.game_steps):
            t.zero_()
        self.totals = np.zeros(4)

    def _mark(self, name):
        if self.timing is not None:
            ev = self.torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timing.setdefault(name, []).append(ev)

    def act(self):
        """One decision per env: ([B, 3] waypoints, has_action [B]).  An env without a decision keeps its waypoint and its budget is
        set to 0, so that the next budget step ends its episode.  self.last: the step's device tensors -- policy / valid_idx / ok of
        the B x workers roots, ensemble [B, kmax], action_idx [B]."""
        env, W = self.env, self.workers
        self._mark("search")
        rep = (lambda x: x.repeat_interleave(W, dim=0)) if W > 1 else (lambda x: x)
        ent = env.history_entries() if self.infer is not None else None
        out = self.mcts.search_device(self._roots, rep(env.prev), rep(env.budget), [1.0], rep(self.tie_u), depth=0,
                                      root_history=rep(ent) if ent is not None else None, deploy_time=self.mode == "deploy")
        pol = out["policy"][0]
        self._mark("pick")
        _ffi.check(self._lib.ipp_play_pick(C.byref(self._pl), pol.data_ptr(), out["valid_idx"].data_ptr(), out["ok"].data_ptr(),
                                           env.engine.stream))
        self.last = dict(policy=pol, valid_idx=out["valid_idx"], ok=out["ok"], ensemble=self.ensemble, action_idx=self.action_idx)
        return self.action, self.forced == 0

    def step(self):
        """act(), env.step(actions), the tally and the totals; returns self.totals (host, the step's one small read)."""
        env = self.env
        self.act()
        self._mark("step")
        env.step(self.action)
        self._mark("tally")
        _ffi.check(self._lib.ipp_play_tally(C.byref(self._pl), env.engine.stream))
        self._mark("totals")
        _ffi.check(self._lib.ipp_play_totals(C.byref(self._pl), self._totals.data_ptr(), env.engine.stream))
        self._totals_host.copy_(self._totals, non_blocking=True)
        self._mark("end")
        self._totals_ev.record()
        self._totals_ev.synchronize()
        self.totals = self._totals_host.numpy().copy()
        self.t += 1
        return self.totals

    def run(self, steps: int, trace: Optional[list] = None, metrics: bool = False):
        """`steps` decisions and env steps.  trace: a list that receives per step a dict of device tensors (budget before, action_idx,
        actions, forced, reward, done after the step) and, with metrics=True, "metrics": env.metrics() after the executed step (the
        reference's Mission.eval after every step, missions.py:176-203)."""
        env = self.env
        for _ in range(int(steps)):
            before = env.budget.clone() if trace is not None else None
            self.step()
            if trace is not None:
                row = dict(budget=before, action_idx=self.action_idx.clone(), actions=self.action.clone(), forced=self.forced.clone(),
                           reward=env.reward.clone(), done=env.done.clone())
                if metrics:
                    row["metrics"] = env.metrics()
                trace.append(row)
        return env.reward

    def play(self):
        """Steps until every env has its games_per_env games, at most games_per_env x (max_episode_steps + 1) steps.  Returns
        dict(game_values [B, G], game_steps [B, G] (device), total, games): the sum of the counted game values and their number."""
        B, G = self.num_envs, self.games_per_env
        for _ in range(G * (self.max_episode_steps + 1)):
            if int(self.totals[3]) >= B:
                break
            self.step()
        return dict(game_values=self.game_values, game_steps=self.game_steps, total=float(self.totals[0]), games=int(self.totals[1]))
