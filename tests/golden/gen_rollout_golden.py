#!/usr/bin/env python3
"""
Generate tests/golden/rollout.npz: rollouts of the reference's classic MCTS planner (planning/mcts_mission.py MCTSMission.rollout /
gcb_rollout, imported from the read-only reference checkout like tests/golden/gen_golden.py does) recorded level by level, for the
device rollouts of csrc/k_rollout.h and their host restatement (ipp-rl_amd/planning/device_rollout.py).

The two roots are those of gen_golden.py::gen_mcts_mission (eps10: adaptive mission, eps-greedy rollouts; gcb10: cost-benefit rollouts;
10x10 grid, altitudes 8 and 14, greedy radius 9 m = 98 candidates around a node).  Rollouts start at the root and at depth-1 and
depth-2 children.  np.random.uniform / np.random.choice are wrapped while a rollout runs, so its draws are known; they are stored as the
two uniforms per level the device consumes:
  u0  the eps-greedy draw as drawn (0 for the cost-benefit policy, which has none)
  u1  unweighted choice of index idx among `count` actions: (rank + 0.5) / count, where rank is the chosen action's position among the
      available actions in get_actions order (row, column, level: ascending y, x, z) -- the device's candidate order, the reference
      lists the same set level-major;  cost-benefit: the midpoint of the chosen action's interval of the normalised cumulative softmax,
      summed in that order
A rollout is kept only when fp32 rewards cannot flip a decision: at every greedy decision every other available reward is at least
MARGIN = 1e-4 below the maximum (ten times the project's 1e-5 parity bar), at every cost-benefit decision u1 is at least MARGIN from
both ends of its interval.  Arrays only; rewards are recomputed with the reference's own prediction_step / compute_reward.

Usage:  python tests/golden/gen_rollout_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402  (stubs cv2 / imageio and puts the reference on the path)
from planning import mcts_mission as ref_mm  # noqa: E402
from planning.common.actions import action_costs as ref_action_costs  # noqa: E402
from planning.common.rewards import compute_adaptive_msk, compute_reward  # noqa: E402

MARGIN = 1e-4
UAV = {"max_v": 2, "max_a": 2}
HP = dict(k=4.0, alpha=0.75, epsilon_expand=0.2, epsilon_rollout=0.5, gamma=0.95, c=2.0)
CASES = [
    # name, grid, adaptive, gcb, root steps, sims, (min, max, spacing), budget, horizon, greedy radius [m], seed  (gen_mcts_mission)
    ("eps10", 10, True, False, 3, 40, (8, 14, 6), 60.0, 3, 9.0, 3),
    ("gcb10", 10, False, True, 2, 24, (8, 14, 6), 50.0, 3, 9.0, 5),
]
KMAX, LEVELS = 98, 3
KEEP_PER_MODE, NEED_PER_MODE, NEED_DEEP = 12, 8, 3


def build_root(case):
    """The root of gen_mcts_mission: same seeds, same calls, so the same state as tests/golden/mcts_mission.npz holds."""
    name, dim, adaptive, gcb, root_steps, sims, (amin, amax, aspc), budget, horizon, radius, seed = case
    params = gg.load_params(dim, dim)
    gm, sensor, sim, mapping = gg.build(params, seed=seed)
    rs = np.random.RandomState(200 + seed)
    prev = np.array([2.0, 2.0, 14.0])
    for _ in range(root_steps):
        a = np.array([4.0 * rs.randint(0, dim) + 2.0, 4.0 * rs.randint(0, dim) + 2.0, 8.0])
        z = sensor.take_measurement(a, verbose=False)
        mapping.update_grid_map(a, z)
        prev = a
    mis = ref_mm.MCTSMission(mapping, UAV, dist_to_boundaries=10, min_altitude=amin, max_altitude=amax, budget=budget,
                             altitude_spacing=aspc, num_simulations=sims, gamma=HP["gamma"], c=HP["c"], episode_horizon=horizon,
                             k=HP["k"], alpha=HP["alpha"], epsilon_expand=HP["epsilon_expand"], epsilon_rollout=HP["epsilon_rollout"],
                             max_greedy_radius=radius, use_gcb_rollout=gcb, adaptive=adaptive, value_threshold=0.4, interval_factor=0)
    root = ref_mm.Node(state=gm.cov_matrix.copy(), parent=None, action=prev.copy())
    have = np.load(os.path.join(gg.OUT, "mcts_mission.npz"))
    assert np.array_equal(have[f"{name}_root_mean"], gm.mean) and np.array_equal(have[f"{name}_root_diag"], np.diag(gm.cov_matrix))
    assert np.array_equal(have[f"{name}_prev"], prev)
    return mis, gm, root


def rewards_at(mis, gm, node, actions):
    msk = compute_adaptive_msk(gm.mean, node.state, mis.value_threshold, mis.interval_factor)
    return np.array([compute_reward(node.state, mis.prediction_step(node.state, a), node.action, a, UAV, msk) for a in actions],
                    dtype=np.float64)


def record(mis, gm, node, budget, depth, gcb):
    """One rollout of the reference from `node`; None when it raises (np.random.choice(0)) or a decision is too close to call."""
    draws, levels = [], []
    orig_uniform, orig_choice = np.random.uniform, np.random.choice

    def uniform(*a, **k):
        r = orig_uniform(*a, **k)
        draws.append(("u", float(r)))
        return r

    def choice(*a, **k):
        r = orig_choice(*a, **k)
        draws.append(("c", int(r)))
        return r

    def wrap(fn):
        def policy(nd, remaining, *rest):
            first = len(draws)
            action = fn(nd, remaining, *rest)
            levels.append((nd, float(remaining), np.array(action, dtype=np.float64), draws[first:]))
            return action
        return policy

    np.random.uniform, np.random.choice = uniform, choice
    mis.eps_greedy_policy, mis.gcb_policy = wrap(type(mis).eps_greedy_policy.__get__(mis)), wrap(type(mis).gcb_policy.__get__(mis))
    try:
        value = (mis.gcb_rollout if gcb else mis.rollout)(node, budget, node.action, depth)
    except ValueError:
        return None
    finally:
        np.random.uniform, np.random.choice = orig_uniform, orig_choice
        del mis.eps_greedy_policy, mis.gcb_policy
    out = dict(value=float(value), levels=len(levels), avail=np.full((LEVELS, KMAX, 3), np.nan), reward=np.full((LEVELS, KMAX), np.nan),
               count=np.zeros(LEVELS, dtype=np.int32), u=np.zeros((LEVELS, 2)), chosen=np.full((LEVELS, 3), np.nan),
               budget_after=np.full(LEVELS, np.nan), greedy=np.zeros(LEVELS, dtype=np.int32))
    left, charge_from = float(budget), node.action
    for lv, (nd, remaining, action, drawn) in enumerate(levels):
        assert remaining == left
        avail = mis.actions_np[mis.get_next_actions_mask(nd.action, remaining, UAV)]
        count = len(avail)
        assert 0 < count <= KMAX
        rw = rewards_at(mis, gm, nd, avail)
        order = np.lexsort((avail[:, 2], avail[:, 0], avail[:, 1]))  # get_actions order: row (y), column (x), level (z)
        pos = int(np.flatnonzero((avail[order] == action).all(axis=1))[0])
        which = order[pos]
        if gcb:
            (kind, idx), = drawn
            assert kind == "c" and np.array_equal(avail[idx], action)
            e = np.exp(rw[order])
            s = 0.0
            for x in e:
                s += x
            cum, cdf = 0.0, []
            for x in e:
                cum += x / s
                cdf.append(cum)
            lo, hi = (cdf[pos - 1] / cdf[-1] if pos else 0.0), cdf[pos] / cdf[-1]
            if 0.5 * (hi - lo) < MARGIN:
                return None
            u0, u1 = 0.0, 0.5 * (lo + hi)
        else:
            kind, u0 = drawn[0]
            assert kind == "u"
            if u0 > mis.epsilon_rollout:
                assert len(drawn) == 1 and int(np.argmax(rw)) == int(which)
                if np.any(np.delete(rw, which) > rw[which] - MARGIN):
                    return None
                u1 = 0.0
                out["greedy"][lv] = 1
            else:
                (_, _), (kind, idx) = drawn
                assert kind == "c" and np.array_equal(avail[idx], action)
                u1 = (pos + 0.5) / count
        left -= ref_action_costs(action, charge_from, UAV)  # (rollout :217 / :181: charged from the level above's waypoint)
        charge_from = nd.action
        out["avail"][lv, :count], out["reward"][lv, :count], out["count"][lv] = avail, rw, count
        out["u"][lv], out["chosen"][lv], out["budget_after"][lv] = (u0, u1), action, left
    return out


def child_of(mis, node, budget, rs):
    """A child as simulate makes it: an available action, the predicted state, the budget charged from the parent's waypoint."""
    avail = mis.actions_np[mis.get_next_actions_mask(node.action, budget, UAV)]
    a = avail[rs.randint(len(avail))].copy()
    child = ref_mm.Node(state=mis.prediction_step(node.state, a), parent=node, action=a)
    return child, budget - ref_action_costs(a, node.action, UAV)


def main():
    out = dict(start_actions=[], start_len=[], case=[], budget=[], depth=[], levels=[], value=[], avail=[], reward=[], count=[], u=[],
               chosen=[], budget_after=[], greedy=[], seed=[])
    ended_early = 0
    for ci, case in enumerate(CASES):
        name, gcb, budget0, horizon = case[0], case[3], case[7], case[8]
        mis, gm, root = build_root(case)
        rs = np.random.RandomState(900 + ci)
        starts = []  # (node, path actions, budget, depth)
        for b in (budget0, budget0, budget0, budget0, 7.0, 8.0, 10.0):
            starts.append((root, [], b, horizon))
        for _ in range(4):
            c1, b1 = child_of(mis, root, budget0, rs)
            starts.append((c1, [c1.action], b1, horizon - 1))
            c2, b2 = child_of(mis, c1, b1, rs)
            starts.append((c2, [c1.action, c2.action], b2, horizon - 2))
        kept = deep = 0
        seed = 0
        for node, path, budget, depth in starts:
            got = None
            while got is None and seed < 4000:  # the first seed from here on whose rollout is decided clearly
                np.random.seed(7000 + 100 * ci + seed)
                got, used = record(mis, gm, node, budget, depth, gcb), seed
                seed += 1
            if got is None or kept >= KEEP_PER_MODE:
                continue
            kept += 1
            deep += int(depth == horizon and got["levels"] == horizon)
            ended_early += int(got["levels"] < depth)
            sa = np.full((2, 3), np.nan)
            if path:
                sa[: len(path)] = path
            out["start_actions"].append(sa); out["start_len"].append(len(path)); out["case"].append(ci); out["budget"].append(budget)
            out["depth"].append(depth); out["seed"].append(used)
            for key in ("levels", "value", "avail", "reward", "count", "u", "chosen", "budget_after", "greedy"):
                out[key].append(got[key])
            print(f"  {name}: start depth {len(path)} budget {budget:.3f} levels {got['levels']}/{depth} value {got['value']:.6f} "
                  f"greedy {got['greedy'][:got['levels']].tolist()} counts {got['count'].tolist()}")
        if kept < NEED_PER_MODE or deep < NEED_DEEP:
            sys.exit(f"{name}: kept {kept} rollouts ({deep} of depth {horizon}); need {NEED_PER_MODE} and {NEED_DEEP}")
    if ended_early < 1:
        sys.exit("no rollout was ended early by its budget")
    arrays = {k: np.array(v) for k, v in out.items()}
    arrays.update(case_names=np.array([c[0] for c in CASES]), margin=np.array(MARGIN), kmax=np.array(KMAX),
                  gamma=np.array(HP["gamma"]), epsilon_rollout=np.array(HP["epsilon_rollout"]), radius=np.array(9.0),
                  alts=np.array([8.0, 14.0, 6.0]), resolution=np.array(4.0), dim=np.array(10), max_v=np.array(2.0), max_a=np.array(2.0))
    gg.save("rollout", **arrays)


if __name__ == "__main__":
    main()
