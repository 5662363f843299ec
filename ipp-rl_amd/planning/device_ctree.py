"""
Classic MCTS for a batch with the tree on the device (csrc/k_ctree.h, include/ipp_engine.h ipp_ctree_*): the search loop of the
reference's MCTSMission (planning/mcts_mission.py:24-66 Node / UCT, :258-304 progressive widening and simulate, :341-351
select_best_child) in device tables.  All R roots advance one simulation at a time in lock step and nothing is read from the device
between the first simulation and the chosen waypoints.  A simulation is

    descend -> expansion (candidates, ipp_tree_score_nodes, eps-greedy pick, recorded ipp_tree_step) -> attach
            -> rollout (ipp_rollout_run, planning/device_rollout.py) -> backup

for every root at once; a root that does not expand / roll out in a simulation has a dead row (live = 0) in that state.

Tables, per root: cap = simulations + 1 node slots, slot 0 the root, nodes created in ascending slot order -- the children of a node
are the slots with parent == node in ascending order, which is the order of the reference's `children` list.  The engine's node pool
is laid out as R x simulations tree nodes (root i's node of simulation s is node s R + i) followed by R x horizon rollout nodes.

Randomness: the caller supplies every uniform (`uniform_tables`): one tie uniform per simulation, root and level (child number
min(floor(u ties), ties - 1) among the children with exactly the largest UCT value, ascending), two per expansion and two per rollout
level (planning/device_rollout.py).  A root's search depends only on its own rows.  The uniforms are consumed differently from
ClassicMCTS(batched=True) (which draws from a NumPy stream as the search goes): for one seed the two do not build the same trees.  A
device search reproduces its host restatement below (search_host), bit for bit.

An expansion with no available action -- the reference and ClassicMCTS raise there, inside np.random.choice(0) -- makes no child: the
simulation's value at that node is 0 and the node counts as the terminal case (IPP_ROLLOUT_NO_ACTION of the expansion's pick).

The host restatements (descend_host, attach_host, backup_host, best_host, search_host) run without a GPU, with the kernels' order of
operations: every fp64 operation rounded on its own.  UCT values involve log(), which need not agree to the last bit between the two
maths libraries; their output is a choice among children.
"""
import ctypes as C
import math
from typing import Dict, Optional

import numpy as np

from .. import _ffi
from . import device_rollout as dr
from .vec_greedy import altitude_levels, radius_candidates, radius_offsets

TERMINAL, ROLLOUT, EXPAND = _ffi.IPP_CTREE_TERMINAL, _ffi.IPP_CTREE_ROLLOUT, _ffi.IPP_CTREE_EXPAND
ERR_RANGE, ERR_SELECT, ERR_PICK, ERR_STEP, ERR_FULL, ERR_ROLLOUT = (_ffi.IPP_CTREE_ERR_RANGE, _ffi.IPP_CTREE_ERR_SELECT, _ffi.IPP_CTREE_ERR_PICK,
                                                                    _ffi.IPP_CTREE_ERR_STEP, _ffi.IPP_CTREE_ERR_FULL, _ffi.IPP_CTREE_ERR_ROLLOUT)
ERR_NAMES = {ERR_RANGE: "a table value out of range", ERR_SELECT: "no child with a comparable UCT value",
             ERR_PICK: "the expansion's pick ended with error flag", ERR_STEP: "the expansion's recorded step returned status",
             ERR_FULL: "no free node slot", ERR_ROLLOUT: "the leaf's rollout ended with error flag"}
TREE_DEPTH = dr.TREE_DEPTH
NODE_FIELDS = ("parent", "dev", "plen", "path", "action", "visits", "value_sum", "edge_reward")
ROOT_FIELDS = ("count", "err", "t_len", "t_slot", "leaf_kind", "leaf_budget", "leaf_depth")


def widening_table(k: float, alpha: float, n_sims: int) -> np.ndarray:
    """thr[v] = k v^alpha as RolloutPolicy.widen evaluates it (Python floats), for every visit counter a search can reach."""
    return np.array([float(k) * v ** float(alpha) for v in range(2 * int(n_sims) + 3)], dtype=np.float64)


def uniform_tables(rng, n_sims: int, roots: int, horizon: int) -> Dict[str, np.ndarray]:
    """The three uniform tables of a search from one NumPy stream: tie [n_sims, roots, horizon], expand [n_sims, roots, 1, 2],
    rollout [n_sims, roots, horizon, 2]."""
    return dict(tie=rng.random_sample((n_sims, roots, horizon)), expand=rng.random_sample((n_sims, roots, 1, 2)),
                rollout=rng.random_sample((n_sims, roots, horizon, 2)))


# ----------------------------------------------------------------------------------------------- host restatements
def new_table(cap: int, horizon: int, waypoint) -> Dict:
    """One root's tables as ipp_ctree holds them: only the root in slot 0."""
    T = dict(parent=np.full(cap, -1, dtype=np.int32), dev=np.full(cap, -1, dtype=np.int32), plen=np.zeros(cap, dtype=np.int32),
             path=np.full((cap, TREE_DEPTH), -1, dtype=np.int32), action=np.zeros((cap, 3)), visits=np.zeros(cap, dtype=np.int32),
             value_sum=np.zeros(cap), edge_reward=np.zeros(cap), count=1, err=0, t_len=0, t_slot=np.zeros(horizon + 1, dtype=np.int32),
             leaf_kind=TERMINAL, leaf_budget=0.0, leaf_depth=0)
    T["action"][0] = np.asarray(waypoint, dtype=np.float64)
    return T


def n_available_host(waypoint, budget: float, P: Dict) -> int:
    """get_next_actions_mask(node.action, budget).sum() over the candidate square (k_ctree_descend)."""
    cands = radius_candidates(waypoint, P["x_dim"], P["y_dim"], P["resolution"], P["min_altitude"], P["max_altitude"], P["altitude_spacing"],
                              P["radius"])
    n = 0
    for cnd in cands:
        if np.isfinite(cnd).all():
            cost = dr.cost_host(cnd, waypoint, P["uav"])
            n += int(cost > 0.0 and cost <= budget)
    return n


def children_host(T: Dict, node: int):
    return [s for s in range(1, int(T["count"])) if int(T["parent"][s]) == node]


def uct_host(T: Dict, s: int, v: int, lo: float, hi: float, waypoint, budget: float, P: Dict) -> float:
    """Node.uct and the cost bar of select_child (ctree_uct)."""
    cv = int(T["visits"][s])
    if cv == 0:
        u = math.inf
    else:
        value = float(T["value_sum"][s]) / cv
        expl = P["c"] * math.sqrt(math.log(v) / cv)
        if hi == 0.0:
            u = value + expl
        elif hi == lo:
            u = value / hi + expl
        else:
            u = (value - lo / (hi - lo)) + expl
    cost = dr.cost_host(T["action"][s], waypoint, P["uav"])
    if cost == 0.0 or cost >= budget:
        u = -math.inf
    return u


def _row(T: Dict, root_slot: int, node: int, budget: float, depth_left: int) -> Dict:
    plen = int(T["plen"][node])
    return dr.new_state(root_slot, [int(x) for x in T["path"][node][:plen]], T["action"][node], budget, depth_left)


def descend_host(T: Dict, root_slot: int, waypoint, budget: float, tie_u, P: Dict):
    """k_ctree_descend on one root's tables (in place).  Returns (leaf kind, state row or None): the row of the rollout state
    (ROLLOUT) or of the expansion state (EXPAND) in planning/device_rollout.py new_state form."""
    if T["err"] != 0:
        return None, None
    cap, horizon = len(T["parent"]), int(P["horizon"])
    count = int(T["count"])
    if count < 1 or count > cap:
        T["err"] = ERR_RANGE
        return None, None
    T["action"][0] = np.asarray(waypoint, dtype=np.float64)
    budget, depth, node, kind, tlen = float(budget), horizon, 0, TERMINAL, 0
    for lvl in range(horizon + 1):
        T["t_slot"][lvl] = node
        tlen = lvl + 1
        if depth == 0 or budget < P["resolution"]:
            kind = TERMINAL
            break
        v = int(T["visits"][node])
        if v == 0:
            kind = ROLLOUT
            break
        if v < 0 or v >= len(P["thr"]):
            T["err"] = ERR_RANGE
            return None, None
        wp = T["action"][node]
        n_av = n_available_host(wp, budget, P)
        ch = children_host(T, node)
        vals = [float(T["value_sum"][s]) / int(T["visits"][s]) for s in ch if int(T["visits"][s]) > 0]
        lo, hi = (min(vals), max(vals)) if vals else (math.inf, -math.inf)
        if len(ch) == 0 or (len(ch) <= float(P["thr"][v]) and len(ch) < n_av):
            kind = EXPAND
            break
        ucts = [uct_host(T, s, v, lo, hi, wp, budget, P) for s in ch]
        comparable = [u for u in ucts if u == u]
        if not comparable:
            T["err"] = ERR_SELECT
            return None, None
        m = max(comparable)
        ties = [s for s, u in zip(ch, ucts) if u == m]
        chosen = ties[max(0, min(int(math.floor(float(tie_u[lvl]) * len(ties))), len(ties) - 1))]
        budget = budget - dr.cost_host(T["action"][chosen], wp, P["uav"])
        depth -= 1
        node = chosen
    if kind != TERMINAL and not 0 <= int(T["plen"][node]) <= TREE_DEPTH:
        T["err"] = ERR_RANGE
        return None, None
    T["t_len"], T["leaf_kind"], T["leaf_budget"], T["leaf_depth"] = tlen, kind, budget, depth
    if kind == ROLLOUT:
        return kind, _row(T, root_slot, node, budget, depth)
    if kind == EXPAND:
        return kind, _row(T, root_slot, node, budget, 1)
    return kind, None


def attach_host(T: Dict, root_slot: int, ex_live: int, ex_flag: int, action, new_id: int, step_reward, step_status: int, P: Dict):
    """k_ctree_attach on one root's tables (in place); returns the child's rollout row or None."""
    if T["err"] != 0 or T["leaf_kind"] != EXPAND:
        return None
    cap, horizon = len(T["parent"]), int(P["horizon"])
    L, count = int(T["t_len"]), int(T["count"])
    if L < 1 or L > horizon or count < 1 or count > cap:
        T["err"] = ERR_RANGE
        return None
    node = int(T["t_slot"][L - 1])
    if node < 0 or node >= count:
        T["err"] = ERR_RANGE
        return None
    if not ex_live:
        if ex_flag == dr.NO_ACTION:
            T["leaf_kind"] = TERMINAL
        else:
            T["err"] = ERR_PICK | (int(ex_flag) << 8)
        return None
    if step_status != _ffi.STATUS_OK:
        T["err"] = ERR_STEP | (int(step_status) << 8)
        return None
    if count >= cap:
        T["err"] = ERR_FULL
        return None
    pl = int(T["plen"][node])
    if pl < 0 or pl >= TREE_DEPTH:
        T["err"] = ERR_RANGE
        return None
    c = count
    T["parent"][c], T["dev"][c] = node, int(new_id)
    T["path"][c] = -1
    T["path"][c, :pl] = T["path"][node, :pl]
    T["path"][c, pl] = int(new_id)
    T["plen"][c] = pl + 1
    T["action"][c] = np.asarray(action, dtype=np.float64)
    T["visits"][c], T["value_sum"][c] = 0, 0.0
    T["edge_reward"][c] = float(np.float32(step_reward))
    T["count"] = c + 1
    T["t_slot"][L] = c
    T["t_len"] = L + 1
    budget = float(T["leaf_budget"]) - dr.cost_host(T["action"][c], T["action"][node], P["uav"])
    depth = int(T["leaf_depth"]) - 1
    T["leaf_budget"], T["leaf_depth"] = budget, depth
    if depth <= 0 or budget < P["resolution"]:
        T["leaf_kind"] = TERMINAL
        return None
    T["leaf_kind"] = ROLLOUT
    return _row(T, root_slot, c, budget, depth)


def backup_host(T: Dict, value: float, flag: int, P: Dict) -> None:
    """k_ctree_backup on one root's tables (in place); (value, flag) of the leaf's rollout."""
    if T["err"] != 0:
        return
    cap, horizon = len(T["parent"]), int(P["horizon"])
    L, count, kind = int(T["t_len"]), int(T["count"]), int(T["leaf_kind"])
    if L < 1 or L > horizon + 1 or count < 1 or count > cap or kind not in (TERMINAL, ROLLOUT):
        T["err"] = ERR_RANGE
        return
    trace = [int(x) for x in T["t_slot"][:L]]
    if any(s < 0 or s >= count for s in trace):
        T["err"] = ERR_RANGE
        return
    v = 0.0
    if kind == ROLLOUT:
        if flag in dr.ERROR_FLAGS:
            T["err"] = ERR_ROLLOUT | (int(flag) << 8)
            return
        leaf = trace[-1]
        v = float(value)
        T["visits"][leaf] += 1
        T["value_sum"][leaf] = float(T["value_sum"][leaf]) + v
    for j in range(L - 2, -1, -1):
        node, child = trace[j], trace[j + 1]
        v = float(T["edge_reward"][child]) + v
        T["visits"][node] += 1
        T["visits"][child] += 1
        T["value_sum"][node] = float(T["value_sum"][node]) + v


def best_host(T: Dict, waypoint):
    """k_ctree_best: (waypoint [3], has)."""
    best, bv = -1, -math.inf
    if T["err"] == 0:
        for s in children_host(T, 0):
            cv = int(T["visits"][s])
            if cv <= 0:
                continue  # (no search leaves a child unvisited)
            val = float(T["value_sum"][s]) / cv
            if val > bv or (best < 0 and val == bv):
                best, bv = s, val
    if best < 0:
        return np.asarray(waypoint, dtype=np.float64).copy(), 0
    return T["action"][best].copy(), 1


def search_host(score_fn, step_fn, rollout_fn, root_slot: int, waypoint, budget: float, uniforms: Dict, *, n_sims: int, horizon: int, c: float,
                thr, epsilon_expand: float, x_dim, y_dim, resolution, min_altitude, max_altitude, altitude_spacing, radius, uav,
                node_base: int = 0, index: int = 0, roots: int = 1, first_sim: int = 0, table: Optional[Dict] = None) -> Dict:
    """One root's whole search on the host, in the order ipp_ctree_search issues it.  score_fn(state, cands [k, 3]) -> (reward [k],
    status [k] or None) stands for ipp_tree_score_nodes on the expansion's node, step_fn(state, action, new_id) -> (reward, status)
    for its recorded step, rollout_fn(state, u [horizon, 2]) -> (value, flag) for ipp_rollout_run on the leaf's row (`state`: a
    planning/device_rollout.py new_state row).  uniforms: tie [n_sims, horizon], expand [n_sims, 1, 2], rollout [n_sims, horizon, 2]
    of this root.  The node of simulation s gets the id node_base + s roots + index.  Returns the tables."""
    P = dict(x_dim=x_dim, y_dim=y_dim, resolution=float(resolution), min_altitude=min_altitude, max_altitude=max_altitude,
             altitude_spacing=altitude_spacing, radius=float(radius), uav=uav, c=float(c), thr=np.asarray(thr, dtype=np.float64),
             horizon=int(horizon))
    T = new_table(int(first_sim) + int(n_sims) + 1, horizon, waypoint) if table is None else table
    tie, ue, ur = (np.asarray(uniforms[k], dtype=np.float64) for k in ("tie", "expand", "rollout"))
    for s in range(int(first_sim), int(first_sim) + int(n_sims)):
        kind, row = descend_host(T, root_slot, waypoint, budget, tie[s], P)
        if T["err"] != 0:
            break
        if kind == EXPAND:
            cands = radius_candidates(row["cur"], x_dim, y_dim, resolution, min_altitude, max_altitude, altitude_spacing, radius)
            reward, status = score_fn(row, cands)
            cost = np.array([dr.cost_host(cnd, row["cur"], uav) if np.isfinite(cnd).all() else np.nan for cnd in cands])
            idx, flag = dr.pick_host(cands, reward, cost, status, row["budget"], 1, ue[s].reshape(-1)[0], ue[s].reshape(-1)[1],
                                     resolution=float(resolution), epsilon=float(epsilon_expand), gcb=False)
            new_id = node_base + s * roots + index
            if idx < 0:
                row = attach_host(T, root_slot, 0, flag, None, -1, 0.0, _ffi.STATUS_OK, P)
            else:
                step_reward, step_status = step_fn(row, cands[idx], new_id)
                row = attach_host(T, root_slot, 1, dr.RUNNING, cands[idx], new_id, step_reward, int(step_status), P)
            if T["err"] != 0:
                break
            kind = T["leaf_kind"]
        value, flag = rollout_fn(row, ur[s]) if kind == ROLLOUT else (0.0, dr.RUNNING)
        backup_host(T, value, int(flag), P)
        if T["err"] != 0:
            break
    return T


def table_to_nodes(T: Dict, root_slot: int):
    """The mcts_mission.Node tree of one root's tables (children in slot order = creation order)."""
    from .mcts_mission import Node

    nodes = []
    for s in range(int(T["count"])):
        pl = int(T["plen"][s])
        parent = nodes[int(T["parent"][s])] if s > 0 else None
        n = Node(int(root_slot), int(T["dev"][s]), [int(x) for x in T["path"][s][:pl]], parent=parent, action=np.array(T["action"][s]),
                 edge_reward=float(T["edge_reward"][s]))
        n.visits, n.value_sum = int(T["visits"][s]), float(T["value_sum"][s])
        if parent is not None:
            parent.children.append(n)
        nodes.append(n)
    return nodes[0]


def describe_err(code: int) -> str:
    return f"{ERR_NAMES.get(code & 0xff, 'unknown')} ({code & 0xff})" + (f", detail {code >> 8}" if code >> 8 else "")


# ----------------------------------------------------------------------------------------------- the device side
_INT = ("root_slot", "parent", "dev", "plen", "path", "visits", "count", "err", "t_len", "t_slot", "leaf_kind", "leaf_depth")


def ctree_buffers(torch, device, roots: int, cap: int, horizon: int, thr_len: int) -> Dict:
    """The [dev] buffers of ipp_ctree by field name, an empty tree per root (call reset_tables before a search)."""
    R, N = int(roots), int(cap)
    shapes = dict(thr=(thr_len,), root_slot=(R,), root_wp=(R, 3), root_budget=(R,), tie_u=(R, horizon), parent=(R, N), dev=(R, N),
                  plen=(R, N), path=(R, N, TREE_DEPTH), action=(R, N, 3), visits=(R, N), value_sum=(R, N), edge_reward=(R, N), count=(R,),
                  err=(R,), t_len=(R,), t_slot=(R, horizon + 1), leaf_kind=(R,), leaf_budget=(R,), leaf_depth=(R,))
    return {name: torch.zeros(shape, dtype=torch.int32 if name in _INT else torch.float64, device=device) for name, shape in shapes.items()}


def reset_tables(t: Dict) -> None:
    """Every root's tree back to its root alone (device fills, nothing is read)."""
    for name in ("plen", "visits", "value_sum", "edge_reward", "action", "err", "t_len", "t_slot", "leaf_kind", "leaf_budget", "leaf_depth"):
        t[name].zero_()
    for name in ("parent", "dev", "path"):
        t[name].fill_(-1)
    t["count"].fill_(1)
    t["action"][:, 0].copy_(t["root_wp"])


def ctree_struct(t: Dict, *, c: float, tree_node_base: int, device_index: int) -> "_ffi.IppCtree":
    """ipp_ctree over the buffers t (ctree_buffers); the caller keeps them alive."""
    ct = _ffi.IppCtree()
    ct.roots, ct.cap, ct.horizon, ct.thr_len = int(t["parent"].shape[0]), int(t["parent"].shape[1]), int(t["tie_u"].shape[1]), int(t["thr"].numel())
    ct.tree_node_base, ct.device, ct.c = int(tree_node_base), int(device_index), float(c)
    for name, tensor in t.items():
        setattr(ct, name, tensor.data_ptr())
    return ct


class DeviceClassicMCTS:
    def __init__(self, engine, cfg, uav_specifications: Optional[Dict], min_altitude: float, max_altitude: float, altitude_spacing: float,
                 num_simulations: int = 100, gamma: float = 0.95, c: float = 2.0, episode_horizon: int = 5, k: float = 4.0,
                 alpha: float = 0.75, epsilon_expand: float = 0.2, epsilon_rollout: float = 0.5, max_greedy_radius: float = 3,
                 use_gcb_rollout: bool = False, adaptive: bool = False, node_capacity: Optional[int] = None, batched: bool = True,
                 roots: int = 1):
        """The arguments of ClassicMCTS (planning/mcts_mission.py); engine: a windowed factor IPPEngine with node_capacity > 0 whose env
        slots hold the roots; `batched` is accepted for the common signature and has no effect (this search is always batched).
        node_capacity (default: the engine's) must hold roots x (num_simulations + episode_horizon) nodes:
        checked here for `roots` and again by every search for its number of roots."""
        if int(engine._c.node_capacity) <= 0 or int(engine._c.window_rows) == 0 or engine.state != "factor":
            raise ValueError("DeviceClassicMCTS needs an engine ipp_tree_step runs on: windowed factor state with node_capacity > 0")
        self.engine, self.cfg, self.uav = engine, cfg, uav_specifications
        self.num_simulations, self.gamma, self.c = int(num_simulations), float(gamma), float(c)
        self.episode_horizon, self.k, self.alpha = int(episode_horizon), float(k), float(alpha)
        self.epsilon_expand, self.epsilon_rollout = float(epsilon_expand), float(epsilon_rollout)
        self.use_gcb_rollout, self.adaptive = bool(use_gcb_rollout), bool(adaptive)
        self.min_altitude, self.max_altitude, self.altitude_spacing = float(min_altitude), float(max_altitude), float(altitude_spacing)
        self.radius = float(max_greedy_radius)
        self.resolution = float(cfg.resolution)
        self.node_capacity = int(node_capacity or engine._c.node_capacity)
        if not 1 <= self.episode_horizon <= engine.TREE_DEPTH:
            raise ValueError(f"episode_horizon {self.episode_horizon} outside [1, {engine.TREE_DEPTH}]")
        if self.num_simulations < 1:
            raise ValueError("num_simulations must be positive")
        if self.node_capacity > int(engine._c.node_capacity):
            raise ValueError(f"node_capacity {self.node_capacity} exceeds the engine's {int(engine._c.node_capacity)}")
        self._need(int(roots))
        self.heights = altitude_levels(self.min_altitude, self.max_altitude, self.altitude_spacing)
        self.half = int(np.ceil(self.radius / self.resolution))
        self.kmax = len(radius_offsets(self.resolution, self.radius)) * len(self.heights)
        self.thr = widening_table(self.k, self.alpha, self.num_simulations)
        if uav_specifications is not None:
            engine.set_uav(uav_specifications["max_v"], uav_specifications["max_a"])
        import torch

        self.torch = torch
        self._levels = torch.as_tensor(self.heights, dtype=torch.float64, device=engine.device)
        self._bufs = {}
        self.last = None  # the buffers of the last search
        self.stats = dict(searches=0, simulations=0)

    def _need(self, roots: int) -> None:
        need = roots * (self.num_simulations + self.episode_horizon)
        if self.node_capacity < need:
            raise ValueError(f"node_capacity {self.node_capacity} too small for a device tree search: {roots} roots x {self.num_simulations} "
                             f"simulations need {roots * self.num_simulations} tree nodes and {roots} x {self.episode_horizon} rollout nodes "
                             f"behind them")

    def host_kwargs(self) -> Dict:
        """The keyword arguments search_host needs to restate this object's searches (node_base, index and roots apart)."""
        return dict(n_sims=self.num_simulations, horizon=self.episode_horizon, c=self.c, thr=self.thr, epsilon_expand=self.epsilon_expand,
                    x_dim=self.cfg.x_dim, y_dim=self.cfg.y_dim, resolution=self.resolution, min_altitude=self.min_altitude,
                    max_altitude=self.max_altitude, altitude_spacing=self.altitude_spacing, radius=self.radius, uav=self.uav)

    def buffers(self, roots: int) -> Dict:
        """tables, the expansion and rollout states with their structs, the scoring scratch and the read-out of `roots` searches."""
        R = int(roots)
        b = self._bufs.get(R)
        if b is not None:
            return b
        self._need(R)
        torch, dev, eng = self.torch, self.engine.device, self.engine
        index = int(dev.index if dev.index is not None else torch.cuda.current_device())
        t = ctree_buffers(torch, dev, R, self.num_simulations + 1, self.episode_horizon, len(self.thr))
        t["thr"].copy_(torch.as_tensor(self.thr).to(dev))
        vmax, amax = (float(self.uav["max_v"]), float(self.uav["max_a"])) if self.uav is not None else (1.0, 1.0)
        kw = dict(grid_w=int(self.cfg.x_dim), grid_h=int(self.cfg.y_dim), half=self.half, device_index=index,
                  flags=_ffi.IPP_ADAPTIVE | (_ffi.IPP_USE_FLIGHT_TIME if self.uav is not None else 0),  # (the search masks every reward)
                  resolution=self.resolution, radius=self.radius, gamma=self.gamma, vmax=vmax, amax=amax)
        ex_t = dr.rollout_buffers(torch, dev, R, self.kmax, 1)
        ro_t = dr.rollout_buffers(torch, dev, R, self.kmax, self.episode_horizon)
        for st in (ex_t, ro_t):
            st["path"].fill_(-1)
        ex = dr.rollout_struct(ex_t, self._levels, gcb=False, node_base=0, epsilon=self.epsilon_expand, **kw)
        ro = dr.rollout_struct(ro_t, self._levels, gcb=self.use_gcb_rollout, node_base=R * self.num_simulations, epsilon=self.epsilon_rollout, **kw)
        nbytes = C.c_uint64(0)
        _ffi.check(eng._lib.ipp_tree_score_nodes_scratch_bytes(eng._h, R, self.kmax, C.byref(nbytes)))
        b = self._bufs[R] = dict(t=t, ct=ctree_struct(t, c=self.c, tree_node_base=0, device_index=index), ex_t=ex_t, ex=ex, ro_t=ro_t, ro=ro,
                                 scratch=torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev),
                                 action=torch.zeros((R, 3), dtype=torch.float64, device=dev), has=torch.zeros(R, dtype=torch.int32, device=dev),
                                 u=None)
        return b

    def load(self, root_slots, waypoints_dev, budgets_dev, uniforms):
        """Empty trees for the roots and the search's uniform tables (tie [n_sims, R, horizon], expand [n_sims, R, 1, 2], rollout
        [n_sims, R, horizon, 2]; arrays are uploaded, device tensors are used as they are).  Nothing is read from the device."""
        torch, dev = self.torch, self.engine.device
        slots = root_slots if isinstance(root_slots, torch.Tensor) else torch.as_tensor(np.asarray(root_slots, dtype=np.int32))
        R = int(slots.shape[0])
        b = self.buffers(R)
        t, S, H = b["t"], self.num_simulations, self.episode_horizon
        t["root_slot"].copy_(slots.to(device=dev, dtype=torch.int32))
        t["root_wp"].copy_(torch.as_tensor(waypoints_dev).to(device=dev, dtype=torch.float64).reshape(R, 3))
        t["root_budget"].copy_(torch.as_tensor(budgets_dev).to(device=dev, dtype=torch.float64).reshape(R))
        reset_tables(t)
        for st in (b["ex_t"], b["ro_t"]):  # rows that the first simulations leave dead still name a root and an empty path
            st["root"].copy_(t["root_slot"]); st["path"].fill_(-1); st["plen"].zero_(); st["cur"].copy_(t["root_wp"]); st["live"].zero_()
            st["flag"].zero_(); st["pick_idx"].fill_(-1)
        u = {}
        for name, shape in (("tie", (S, R, H)), ("expand", (S, R, 1, 2)), ("rollout", (S, R, H, 2))):
            x = uniforms[name]
            x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))
            if tuple(x.shape) != shape:
                raise ValueError(f"uniforms[{name!r}] has shape {tuple(x.shape)}, the search needs {shape}")
            u[name] = x.to(device=dev, dtype=torch.float64).contiguous()
        b["u"] = u
        b["ct"].tie_u, b["ex"].u, b["ro"].u = u["tie"].data_ptr(), u["expand"].data_ptr(), u["rollout"].data_ptr()
        self.last = b
        return b

    def run(self, b: Dict, first_sim: int = 0, n_sims: Optional[int] = None) -> None:
        """Simulations [first_sim, first_sim + n_sims) of the loaded search (ipp_ctree_search): no host read."""
        eng = self.engine
        n = self.num_simulations - int(first_sim) if n_sims is None else int(n_sims)
        _ffi.check(eng._lib.ipp_ctree_search(eng._h, C.byref(b["ct"]), C.byref(b["ex"]), C.byref(b["ro"]), b["scratch"].data_ptr(),
                                             int(b["scratch"].numel()), int(first_sim), n, eng.stream))
        self.stats["simulations"] += n

    def best(self, b: Dict):
        eng = self.engine
        _ffi.check(eng._lib.ipp_ctree_best(C.byref(b["ct"]), b["action"].data_ptr(), b["has"].data_ptr(), eng.stream))
        return b["action"], b["has"]

    def search(self, root_slots, waypoints_dev, budgets_dev, uniforms):
        """One search per root: (actions [R, 3] float64, has [R] int32) as device tensors -- the best child's waypoint and 1, or the
        root's own waypoint and 0 (no child, or the root's search ended with an error: see check())."""
        b = self.load(root_slots, waypoints_dev, budgets_dev, uniforms)
        self.run(b)
        self.stats["searches"] += 1
        return self.best(b)

    def check(self) -> None:
        """The one optional read of the last search's err column; raises naming the first root with an error and its flag."""
        if self.last is None:
            return
        err = self.last["t"]["err"].cpu().numpy()
        bad = np.flatnonzero(err)
        if len(bad):
            raise ValueError(f"device tree search: root {int(bad[0])} ended with err = {int(err[bad[0]])}: {describe_err(int(err[bad[0]]))}"
                             + (f" ({len(bad)} roots with errors)" if len(bad) > 1 else ""))

    def tables_host(self):
        """The last search's tables, one dict per root in the host restatements' form (reads the device)."""
        t = self.last["t"]
        h = {name: t[name].cpu().numpy() for name in NODE_FIELDS + ROOT_FIELDS}
        slots = t["root_slot"].cpu().numpy()
        out = []
        for i in range(len(slots)):
            T = {name: h[name][i].copy() for name in NODE_FIELDS + ("t_slot",)}
            T.update({name: h[name][i].item() for name in ROOT_FIELDS if name != "t_slot"})
            out.append(T)
        return out, slots

    def to_host(self):
        """The last search's trees as mcts_mission.Node roots (ClassicMCTS.merge_roots / select_best_child work on them)."""
        tables, slots = self.tables_host()
        return [table_to_nodes(T, int(s)) for T, s in zip(tables, slots)]
