"""
Rollouts of the classic MCTS planner on the device (csrc/k_rollout.h, include/ipp_engine.h ipp_rollout_*): n rollouts of the reference's
MCTSMission.rollout / gcb_rollout (planning/mcts_mission.py:167-256) advance together, level by level, with no host read between the
levels.  A level is {candidates around the current waypoint, their rewards from the node's state (ipp_tree_score_nodes), the eps-greedy
or cost-benefit pick, one recorded ipp_tree_step, the discounted return}.

Randomness: the caller supplies two uniforms per rollout and level.  u0 decides greedy / random (eps mode; `u0 > epsilon` is greedy, as
np.random.uniform(0, 1) > epsilon), u1 picks among the available candidates: number min(floor(u1 count), count - 1) in ascending order
for the unweighted choice, the first index whose normalised cumulative softmax exceeds u1 for the cost-benefit policy (what legacy
np.random.choice(n, p=p) does with its one uniform).  NumPy's unweighted choice draws through randint, so a search that uses these
rollouts does not reproduce a recorded NumPy stream; the distributions are the same.

The candidates of a level come in get_actions order (row, column, level; planning/vec_greedy.py radius_candidates), the reference
enumerates its action table level-major: among EXACTLY equal rewards the greedy pick may differ, and u1 maps to the candidates in this
order.

The host restatements below (pick_host, advance_host, rollout_host) run without a GPU and add in the kernels' order: every fp64
operation rounded on its own, the softmax sum and its cumulative sum sequentially over the available candidates in ascending order.
"""
import ctypes as C
import math
from typing import Dict, Optional

import numpy as np

from .. import _ffi
from .vec_greedy import altitude_levels, radius_candidates, radius_offsets

RUNNING, END, NO_ACTION, RANK_FULL = _ffi.IPP_ROLLOUT_RUNNING, _ffi.IPP_ROLLOUT_END, _ffi.IPP_ROLLOUT_NO_ACTION, _ffi.IPP_ROLLOUT_RANK_FULL
ERR_FOOTPRINT, ERR_NAN, ERR_STEP = _ffi.IPP_ROLLOUT_ERR_FOOTPRINT, _ffi.IPP_ROLLOUT_ERR_NAN, _ffi.IPP_ROLLOUT_ERR_STEP
ERROR_FLAGS = (ERR_FOOTPRINT, ERR_NAN, ERR_STEP)
TREE_DEPTH = 6


# ----------------------------------------------------------------------------------------------- host restatements
def cost_host(action, previous, uav: Optional[Dict]) -> float:
    """action_costs (planning/common/actions.py) in the kernels' order of operations (rollout_cost, csrc/k_rollout.h)."""
    dx, dy, dz = (float(action[q]) - float(previous[q]) for q in range(3))
    dist = math.sqrt(dx * dx + dy * dy + dz * dz)
    if uav is None:
        return dist
    vmax, amax = float(uav["max_v"]), float(uav["max_a"])
    d_acc = min(dist * 0.5, vmax * vmax / (2 * amax))
    return (dist - 2 * d_acc) / vmax + 2 * math.sqrt(2 * d_acc / amax)


def available_host(cand, cost, budget) -> np.ndarray:
    """get_next_actions_mask (:167-173) on a candidate list: a finite row with 0 < cost <= budget."""
    cand, cost = np.asarray(cand, dtype=np.float64), np.asarray(cost, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(cand).all(axis=-1) & (cost > 0) & (cost <= float(budget))


def pick_host(cand, reward, cost, status, budget, depth_left, u0, u1, *, resolution, epsilon, gcb):
    """One decision of k_rollout_pick: (index, flag).  index -1 = the rollout ends with `flag`; otherwise flag is RUNNING.
    reward is compared as given (the device compares the fp32 values of the step kernel)."""
    if depth_left == 0 or budget < resolution:
        return -1, END
    reward = np.asarray(reward)
    av = np.flatnonzero(available_host(cand, cost, budget))
    count = len(av)
    if status is not None and np.any(np.asarray(status)[av] == _ffi.STATUS_BAD_FOOTPRINT):
        return -1, ERR_FOOTPRINT
    if count == 0:
        return -1, NO_ACTION
    if gcb:
        r = [float(reward[k]) for k in av]
        if any(x != x for x in r):
            return -1, ERR_NAN
        try:
            e = [math.exp(x) for x in r]
        except OverflowError:
            return -1, ERR_NAN
        s = 0.0
        for x in e:
            s += x
        if not (0.0 < s < math.inf):
            return -1, ERR_NAN
        tot = 0.0
        for x in e:
            tot += x / s
        cum = 0.0
        for k, x in zip(av, e):
            cum += x / s
            if cum / tot > u1:
                return int(k), RUNNING
        return int(av[-1]), RUNNING
    if u0 > epsilon:
        best, best_r = -1, -math.inf
        for k in av:
            if reward[k] > best_r:
                best, best_r = int(k), reward[k]
        return (best, RUNNING) if best >= 0 else (-1, ERR_NAN)
    return int(av[min(int(math.floor(u1 * count)), count - 1)]), RUNNING


def new_state(root, path, cur, budget, depth) -> Dict:
    """Per-rollout state as ipp_rollout holds it."""
    path = [int(p) for p in path if int(p) >= 0]
    return dict(root=int(root), path=path + [-1] * (TREE_DEPTH - len(path)), plen=len(path), cur=np.array(cur, dtype=np.float64),
                charge_from=np.array(cur, dtype=np.float64), budget=float(budget), depth_left=int(depth), value=0.0, disc=1.0, live=1,
                flag=RUNNING)


def advance_host(st: Dict, action, new_id, step_reward, step_status, *, gamma, uav) -> None:
    """k_rollout_advance on one rollout's state (in place)."""
    if not st["live"]:
        return
    if step_status not in (_ffi.STATUS_OK, _ffi.STATUS_RANK_FULL):
        st["live"], st["flag"] = 0, ERR_STEP
        return
    st["value"] = st["value"] + st["disc"] * float(step_reward)
    st["disc"] = st["disc"] * float(gamma)
    if step_status == _ffi.STATUS_RANK_FULL:
        st["live"], st["flag"] = 0, RANK_FULL
        return
    st["budget"] = st["budget"] - cost_host(action, st["charge_from"], uav)  # (the grandparent quirk, :226)
    st["charge_from"] = st["cur"].copy()
    st["cur"] = np.array(action, dtype=np.float64)
    if st["plen"] < TREE_DEPTH:
        st["path"][st["plen"]] = int(new_id)
        st["plen"] += 1
    st["depth_left"] -= 1


def rollout_host(score_fn, cur, budget, depth, uniforms, *, x_dim, y_dim, resolution, min_altitude, max_altitude, altitude_spacing, radius,
                 gamma, epsilon, gcb, uav, max_depth=None, step_fn=None, node_base=0, index=0, root=0, path=()):
    """One rollout on the host.  score_fn(state, cands [k, 3]) -> (reward [k], status [k] or None) stands for ipp_tree_score_nodes,
    step_fn(state, action) -> (reward, status) for the recorded step (None: the picked candidate's scored reward, status OK -- the two
    are the same number in the reference, compute_reward(node.state, next.state, node.action, action)).  Returns the final state with
    the per-level `actions`, `budgets` (after the level) and `picks`."""
    uniforms = np.asarray(uniforms, dtype=np.float64).reshape(-1, 2)
    max_depth = len(uniforms) if max_depth is None else int(max_depth)
    st = new_state(root, path, cur, budget, depth)
    st.update(actions=[], budgets=[], picks=[])
    for level in range(max_depth):
        if not st["live"]:
            break
        cands = radius_candidates(st["cur"], x_dim, y_dim, resolution, min_altitude, max_altitude, altitude_spacing, radius)
        reward, status = score_fn(st, cands)
        cost = np.array([cost_host(c, st["cur"], uav) if np.isfinite(c).all() else np.nan for c in cands])
        idx, flag = pick_host(cands, reward, cost, status, st["budget"], st["depth_left"], uniforms[level, 0], uniforms[level, 1],
                              resolution=resolution, epsilon=epsilon, gcb=gcb)
        if idx < 0:
            st["live"], st["flag"] = 0, flag
            break
        action = cands[idx]
        step_reward, step_status = (reward[idx], _ffi.STATUS_OK) if step_fn is None else step_fn(st, action)
        advance_host(st, action, node_base + index * max_depth + level, step_reward, step_status, gamma=gamma, uav=uav)
        st["actions"].append(action.copy())
        st["budgets"].append(st["budget"])
        st["picks"].append(idx)
    return st


# ----------------------------------------------------------------------------------------------- the device side
_INT = ("root", "path", "plen", "depth_left", "live", "flag", "status", "new_id", "step_status", "pick_idx")
_F32 = ("reward", "step_reward")


def rollout_buffers(torch, device, n: int, kmax: int, max_depth: int) -> Dict:
    """The [dev] buffers of ipp_rollout for n rollouts, zero-filled, by field name."""
    K, D = int(kmax), int(max_depth)
    shapes = dict(u=(n, D, 2), root=(n,), path=(n, TREE_DEPTH), plen=(n,), cur=(n, 3), charge_from=(n, 3), budget=(n,), depth_left=(n,),
                  value=(n,), disc=(n,), live=(n,), flag=(n,), cand=(n, K, 3), reward=(n, K), cost=(n, K), status=(n, K), action=(n, 3),
                  new_id=(n,), step_reward=(n,), step_status=(n,), pick_idx=(n, D))
    return {name: torch.zeros(shape, dtype=torch.int32 if name in _INT else torch.float32 if name in _F32 else torch.float64, device=device)
            for name, shape in shapes.items()}


def rollout_struct(t: Dict, levels, *, gcb, grid_w, grid_h, half, node_base, device_index, flags, resolution, radius, gamma, epsilon,
                   vmax, amax) -> "_ffi.IppRollout":
    """ipp_rollout over the buffers t (rollout_buffers) and the altitude levels (device float64 tensor); the caller keeps both alive."""
    ro = _ffi.IppRollout()
    ro.n, ro.kmax, ro.max_depth, ro.gcb = int(t["root"].shape[0]), int(t["cand"].shape[1]), int(t["pick_idx"].shape[1]), int(bool(gcb))
    ro.grid_w, ro.grid_h, ro.n_levels, ro.half = int(grid_w), int(grid_h), int(levels.numel()), int(half)
    ro.node_base, ro.device, ro.flags = int(node_base), int(device_index), int(flags)
    ro.resolution, ro.radius, ro.gamma, ro.epsilon, ro.vmax, ro.amax = (float(resolution), float(radius), float(gamma), float(epsilon),
                                                                       float(vmax), float(amax))
    ro.levels = levels.data_ptr()
    for name, tensor in t.items():
        setattr(ro, name, tensor.data_ptr())
    return ro


class DeviceRollout:
    def __init__(self, engine, min_altitude: float, max_altitude: float, altitude_spacing: float, uav: Optional[Dict], radius: float,
                 gamma: float, epsilon: float, gcb: bool, max_depth: int, node_base: int):
        """engine: a windowed factor IPPEngine with node_capacity > 0 (the engines ipp_tree_step runs on).  (min_altitude, max_altitude, altitude_spacing): the actions spec;
        uav: {"max_v", "max_a"} or None (cost = distance); node_base: rollout i records level l as node
        node_base + i max_depth + l of the engine's node pool."""
        if int(engine._c.node_capacity) <= 0 or int(engine._c.window_rows) == 0 or engine.state != "factor":
            raise ValueError("DeviceRollout needs an engine ipp_tree_step runs on: windowed factor state with node_capacity > 0")
        if not 1 <= int(max_depth) <= engine.TREE_DEPTH:
            raise ValueError(f"max_depth {max_depth} outside [1, {engine.TREE_DEPTH}]")
        self.engine, self.uav = engine, uav
        self.cfg = engine.cfg
        self.min_altitude, self.max_altitude, self.altitude_spacing = float(min_altitude), float(max_altitude), float(altitude_spacing)
        self.radius, self.gamma, self.epsilon, self.gcb = float(radius), float(gamma), float(epsilon), bool(gcb)
        self.max_depth, self.node_base = int(max_depth), int(node_base)
        self.heights = altitude_levels(self.min_altitude, self.max_altitude, self.altitude_spacing)
        self.half = int(np.ceil(self.radius / float(self.cfg.resolution)))
        self.kmax = len(radius_offsets(float(self.cfg.resolution), self.radius)) * len(self.heights)
        if uav is not None:
            engine.set_uav(uav["max_v"], uav["max_a"])
        import torch

        self.torch = torch
        self._levels = torch.as_tensor(self.heights, dtype=torch.float64, device=engine.device)
        self._bufs = {}
        self.buf = None   # the buffers of the last run (device tensors by field name)
        self.n = 0

    def host_kwargs(self) -> Dict:
        """The keyword arguments rollout_host needs to restate this object's rollouts."""
        return dict(x_dim=self.cfg.x_dim, y_dim=self.cfg.y_dim, resolution=float(self.cfg.resolution), min_altitude=self.min_altitude,
                    max_altitude=self.max_altitude, altitude_spacing=self.altitude_spacing, radius=self.radius, gamma=self.gamma,
                    epsilon=self.epsilon, gcb=self.gcb, uav=self.uav, max_depth=self.max_depth, node_base=self.node_base)

    def _buffers(self, n: int):
        torch, dev = self.torch, self.engine.device
        b = self._bufs.get(n)
        if b is not None:
            return b
        t = rollout_buffers(torch, dev, n, self.kmax, self.max_depth)
        nbytes = C.c_uint64(0)
        _ffi.check(self.engine._lib.ipp_tree_score_nodes_scratch_bytes(self.engine._h, n, self.kmax, C.byref(nbytes)))
        scratch = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        vmax, amax = (float(self.uav["max_v"]), float(self.uav["max_a"])) if self.uav is not None else (1.0, 1.0)
        ro = rollout_struct(t, self._levels, gcb=self.gcb, grid_w=int(self.cfg.x_dim), grid_h=int(self.cfg.y_dim), half=self.half,
                            node_base=self.node_base, device_index=int(dev.index if dev.index is not None else torch.cuda.current_device()),
                            flags=_ffi.IPP_ADAPTIVE | (_ffi.IPP_USE_FLIGHT_TIME if self.uav is not None else 0),  # (the search masks every reward)
                            resolution=float(self.cfg.resolution), radius=self.radius, gamma=self.gamma, epsilon=self.epsilon, vmax=vmax, amax=amax)
        b = self._bufs[n] = (t, ro, scratch)
        return b

    def load(self, roots, paths, cur, budgets, depths, uniforms):
        """Start state of n rollouts: roots [n] env slots, paths [n] lists of node ids (root side first), cur [n, 3] the nodes'
        waypoints, budgets [n], depths [n] levels left, uniforms [n, >= max depth left, 2] in [0, 1)."""
        torch, dev = self.torch, self.engine.device
        n = len(roots)
        if (self.node_base + n * self.max_depth) > int(self.engine._c.node_capacity):
            raise ValueError(f"rollout nodes [{self.node_base}, {self.node_base + n * self.max_depth}) exceed node_capacity "
                             f"{int(self.engine._c.node_capacity)}")
        t, ro, scratch = self._buffers(n)
        path = np.full((n, TREE_DEPTH), -1, dtype=np.int32)
        plen = np.zeros(n, dtype=np.int32)
        depths = np.asarray(depths, dtype=np.int32).reshape(n)
        for i, p in enumerate(paths):
            p = [int(x) for x in p if int(x) >= 0]
            if len(p) + min(int(depths[i]), self.max_depth) > TREE_DEPTH:
                raise ValueError(f"rollout {i}: a path of {len(p)} nodes and {int(depths[i])} levels exceed the engine's path depth {TREE_DEPTH}")
            path[i, : len(p)] = p
            plen[i] = len(p)
        u = np.zeros((n, self.max_depth, 2))
        uu = np.asarray(uniforms, dtype=np.float64).reshape(n, -1, 2)[:, : self.max_depth]
        u[:, : uu.shape[1]] = uu
        cur = np.asarray(cur, dtype=np.float64).reshape(n, 3)

        def put(name, arr):
            t[name].copy_(torch.as_tensor(np.ascontiguousarray(arr)).to(dev))

        put("u", u); put("root", np.asarray(roots, dtype=np.int32)); put("path", path); put("plen", plen)
        put("cur", cur); put("charge_from", cur); put("budget", np.asarray(budgets, dtype=np.float64).reshape(n)); put("depth_left", depths)
        t["value"].zero_(); t["disc"].fill_(1.0); t["live"].fill_(1); t["flag"].zero_(); t["pick_idx"].fill_(-1)
        self.buf, self._ro, self._scratch, self.n = t, ro, scratch, n
        return t

    # single calls (the tests drive a level by hand with them)
    def candidates(self):
        _ffi.check(self.engine._lib.ipp_rollout_candidates(C.byref(self._ro), self.engine.stream))

    def score(self):
        t = self.buf
        _ffi.check(self.engine._lib.ipp_tree_score_nodes(self.engine._h, t["root"].data_ptr(), t["path"].data_ptr(), self.n, self.kmax,
                                                         t["cand"].data_ptr(), t["cur"].data_ptr(), int(self._ro.flags), t["reward"].data_ptr(),
                                                         t["cost"].data_ptr(), t["status"].data_ptr(), self._scratch.data_ptr(),
                                                         int(self._scratch.numel()), self.engine.stream))

    def pick(self, level: int):
        _ffi.check(self.engine._lib.ipp_rollout_pick(C.byref(self._ro), int(level), self.engine.stream))

    def step(self):
        t = self.buf
        mb = int(self.engine.max_batch)
        for o in range(0, self.n, mb):
            cnt = min(mb, self.n - o)
            _ffi.check(self.engine._lib.ipp_tree_step(self.engine._h, t["root"][o:].data_ptr(), t["path"][o:].data_ptr(), t["new_id"][o:].data_ptr(),
                                                      cnt, t["action"][o:].data_ptr(), t["cur"][o:].data_ptr(), int(self._ro.flags),
                                                      t["step_reward"][o:].data_ptr(), t["step_status"][o:].data_ptr(), self.engine.stream))

    def advance(self):
        _ffi.check(self.engine._lib.ipp_rollout_advance(C.byref(self._ro), self.engine.stream))

    def run(self, roots, paths, cur, budgets, depths, uniforms, level_by_level: bool = False):
        """All levels of n rollouts; returns (values [n] float64, flags [n] int32) as device tensors -- the caller makes one read.
        level_by_level: issue the four calls of every level from here instead of ipp_rollout_run (same results, bit for bit)."""
        t = self.load(roots, paths, cur, budgets, depths, uniforms)
        if level_by_level:
            for level in range(self.max_depth):
                self.candidates(); self.score(); self.pick(level); self.step(); self.advance()
        else:
            _ffi.check(self.engine._lib.ipp_rollout_run(self.engine._h, C.byref(self._ro), self._scratch.data_ptr(),
                                                        int(self._scratch.numel()), self.engine.stream))
        return t["value"], t["flag"]
