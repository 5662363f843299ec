"""
GPU tests of the classic MCTS with its tree on the device (planning/device_ctree.py, csrc/k_ctree.h, ipp_ctree_search): a whole search
of four roots against the host restatement search_host, whose three questions -- the expansion's candidate scores, its recorded step,
the leaf's rollout -- are answered by the same engine one root at a time (tree_score_nodes, tree_step, a one-rollout DeviceRollout) in
a node range of their own; and VecMctsPolicy(tree="device") on a budget-mode VecIPPEnv.

The roots are those of the mcts_mission golden case eps10, rebuilt as tests/test_hip_rollout.py builds them.  The whole table is compared
exactly: the engine's answers are the same fp32 numbers whether a root is asked alone or in a launch of four, and everything the tree
kernels compute from them is IEEE-exact fp64 in a stated order (UCT values apart, which only choose).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
UAV = {"max_v": 2, "max_a": 2}
TOL = 1e-5
NAME, R = "eps10", 4
FIELDS = ("parent", "action", "visits", "value_sum", "edge_reward", "count", "plen")


def host(t):
    return t.detach().cpu().numpy()


def build(g, copies, node_capacity=512):
    """One engine whose slots hold the recorded root `copies` times (tests/test_hip_rollout.py::build)."""
    from ipp_rl_amd import EngineConfig, IPPEngine

    dim, steps, horizon = int(g[f"{NAME}_dim"]), len(g[f"{NAME}_root_actions"]), int(g[f"{NAME}_horizon"])
    cfg = EngineConfig(x_dim=dim, y_dim=dim)
    eng = IPPEngine(cfg, capacity=copies, state="factor", rank_cap=9 * (steps + horizon + 2), window_rows=-1, fixed_prior=True,
                    node_capacity=node_capacity, max_batch=64)
    for slot in range(copies):
        eng.reset(env_ids=[slot], gt=g[f"{NAME}_gt"][None])
        prev = np.array([2.0, 2.0, 14.0])
        for a, eps in zip(g[f"{NAME}_root_actions"], g[f"{NAME}_root_eps"]):
            _, st = eng.step(a[None], prev[None], env_ids=[slot], meas_noise=eps[None])
            assert int(st[0]) == 0
            prev = a
        assert np.max(np.abs(host(eng.read_mean(slot)).astype(np.float64) - g[f"{NAME}_root_mean"])) < TOL
    return cfg, eng


def planner(g, cfg, eng, **kw):
    from ipp_rl_amd.planning import DeviceClassicMCTS

    amin, amax, aspc = g[f"{NAME}_alts"]
    return DeviceClassicMCTS(eng, cfg, UAV, float(amin), float(amax), float(aspc), num_simulations=int(g[f"{NAME}_sims"]),
                             gamma=float(g["hyper_gamma"]), c=float(g["hyper_c"]), episode_horizon=int(g[f"{NAME}_horizon"]),
                             k=float(g["hyper_k"]), alpha=float(g["hyper_alpha"]), epsilon_expand=float(g["hyper_epsilon_expand"]),
                             epsilon_rollout=float(g["hyper_epsilon_rollout"]), max_greedy_radius=float(g[f"{NAME}_radius"]),
                             use_gcb_rollout=bool(g[f"{NAME}_gcb"]), adaptive=bool(g[f"{NAME}_adaptive"]), **kw)


def same_tree(a, b):
    assert np.array_equal(a.action, b.action) and a.visits == b.visits and len(a.children) == len(b.children)
    assert float(a.value_sum) == float(b.value_sum)
    for x, y in zip(a.children, b.children):
        same_tree(x, y)


def visits_consistent(node, root=True):
    """simulate's counters (tests/test_hip_rollout.py::visits_consistent): a node with children was passed `visits` (root) or
    `visits / 2` times, and each pass after the first went to exactly one child, raising that child's counter by one or two."""
    if node.children:
        assert root or node.visits % 2 == 0
        passes = node.visits if root else node.visits // 2
        total = sum(c.visits for c in node.children)
        assert passes - 1 <= total <= 2 * (passes - 1), (node.visits, total)
    for c in node.children:
        assert c.visits >= 1
        visits_consistent(c, False)


def same_table(got, want):
    n = int(want["count"])
    assert int(got["count"]) == n
    for name in FIELDS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.ndim:
            a, b = a[:n], b[:n]
        assert a.tobytes() == b.astype(a.dtype).tobytes(), name


def test_device_search_equals_its_host_restatement(golden):
    import torch

    from ipp_rl_amd import _ffi
    from ipp_rl_amd.planning import device_ctree as dc
    from ipp_rl_amd.planning.device_rollout import DeviceRollout
    from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

    g = golden("mcts_mission")
    cfg, eng = build(g, R)
    mcts = planner(g, cfg, eng, roots=R)
    sims, horizon = mcts.num_simulations, mcts.episode_horizon
    assert R * (sims + horizon) <= 200   # the restatement's own node ranges start there
    one = dc.uniform_tables(np.random.RandomState(5), sims, 1, horizon)
    u = {k: np.repeat(v, R, axis=1) for k, v in one.items()}          # the four copies get the same uniforms
    wp, budget = g[f"{NAME}_prev"], float(g[f"{NAME}_budget"])
    wps = torch.as_tensor(np.tile(wp, (R, 1)), device=eng.device)
    budgets = torch.full((R,), budget, dtype=torch.float64, device=eng.device)
    actions, has = mcts.search(list(range(R)), wps, budgets, u)
    torch.cuda.synchronize()
    mcts.check()
    tables, slots = mcts.tables_host()
    assert slots.tolist() == list(range(R))
    actions, has = host(actions).copy(), host(has).copy()
    roots = mcts.to_host()

    # the restatement of root 0, answered by the same engine one root at a time, in node ranges of its own
    amin, amax, aspc = (float(x) for x in g[f"{NAME}_alts"])
    ro = DeviceRollout(eng, amin, amax, aspc, UAV, mcts.radius, mcts.gamma, mcts.epsilon_rollout, False, horizon, 300)

    def score_fn(st, cands):
        r, s = eng.tree_score_nodes([st["root"]], np.array([st["path"]], dtype=np.int32), cands[None], st["cur"][None], adaptive=True,
                                    use_flight_time=True)
        return host(r)[0], host(s)[0]

    def step_fn(st, action, new_id):
        r, s = eng.tree_step([st["root"]], [st["path"]], action[None], st["cur"][None], new_ids=[new_id], adaptive=True, use_flight_time=True)
        return host(r)[0], int(host(s)[0])

    def rollout_fn(st, uu):
        v, f = ro.run([st["root"]], [st["path"][: st["plen"]]], st["cur"][None], [st["budget"]], [st["depth_left"]], uu[None])
        return float(host(v)[0]), int(host(f)[0])

    T = dc.search_host(score_fn, step_fn, rollout_fn, 0, wp, budget, {k: v[:, 0] for k, v in u.items()}, node_base=200, **mcts.host_kwargs())
    assert T["err"] == 0
    print(f"[device tree] nodes {int(T['count'])}, root visits {int(T['visits'][0])}, depth {int(T['plen'].max())}")
    for i in range(R):
        same_table(tables[i], T)
        assert roots[i].visits == sims and len(roots[i].children) >= 2
        visits_consistent(roots[i])
        same_tree(roots[0], roots[i])
        # node ids: simulation s of root i made node s R + i
        n = int(tables[i]["count"])
        assert np.all((tables[i]["dev"][1:n] - i) % R == 0) and np.all(np.diff(tables[i]["dev"][1:n]) > 0)
        best = ClassicMCTS.select_best_child(roots[i])
        wa, wh = dc.best_host(tables[i], wp)
        assert int(has[i]) == wh == 1 and np.array_equal(actions[i], wa) and np.array_equal(actions[i], best.action)
    assert int(T["plen"].max()) >= 2 and int(T["count"]) >= 10

    # a root alone: the same tree as in the batch of four (the same object, other buffers)
    mcts.search([0], wps[:1], budgets[:1], {k: v[:, :1] for k, v in u.items()})
    torch.cuda.synchronize()
    mcts.check()
    (alone,), _ = mcts.tables_host()
    same_table(alone, T)
    assert np.array_equal(alone["dev"][1: int(alone["count"])], tables[0]["dev"][1: int(T["count"])] // R)
    # merge_roots works on the rebuilt trees
    a, b = mcts.to_host()[0], roots[1]
    merged = ClassicMCTS.merge_roots(a, b)
    assert merged.visits > sims and ClassicMCTS.select_best_child(merged) is not None
    eng.close()


def test_node_capacity_is_checked_up_front(golden):
    import torch

    from ipp_rl_amd.planning import device_ctree as dc

    g = golden("mcts_mission")
    cfg, eng = build(g, 2, node_capacity=64)
    with pytest.raises(ValueError, match="node_capacity"):
        planner(g, cfg, eng, roots=2)                      # 2 x (40 + 3) > 64
    with pytest.raises(ValueError, match="node_capacity"):
        planner(g, cfg, eng, roots=1, node_capacity=128)   # more than the engine has
    mcts = planner(g, cfg, eng, roots=1)
    u = dc.uniform_tables(np.random.RandomState(1), mcts.num_simulations, 2, mcts.episode_horizon)
    wps = torch.as_tensor(np.tile(g[f"{NAME}_prev"], (2, 1)), device=eng.device)
    with pytest.raises(ValueError, match="node_capacity"):
        mcts.search([0, 1], wps, torch.full((2,), 60.0, dtype=torch.float64, device=eng.device), u)
    with pytest.raises(ValueError, match="shape"):
        mcts.search([0], wps[:1], torch.full((1,), 60.0, dtype=torch.float64, device=eng.device), u)
    eng.close()


# ----------------------------------------------------------------------------------------------- VecMctsPolicy(tree="device")
def _vec_policy(seed, tree):
    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning import VecMctsPolicy
    from ipp_rl_amd.vec_env import VecIPPEnv

    B, sims, horizon, steps = 4, 8, 3, 6
    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    env = VecIPPEnv(cfg, B, episode_steps=steps, seed=11, budget=40.0, window_rows=-1, rank_cap=9 * (steps + horizon + 2),
                    node_capacity=B * (sims + horizon), max_batch=64)
    env.reset()
    return VecMctsPolicy(env, 8.0, 14.0, 6.0, num_simulations=sims, episode_horizon=horizon, max_greedy_radius=9.0, seed=seed, tree=tree)


def test_vec_mcts_policy_with_the_tree_on_the_device():
    import torch

    from ipp_rl_amd.planning import DeviceClassicMCTS
    from ipp_rl_amd.planning.common.actions import action_costs

    traces = []
    for _ in range(2):
        pol = _vec_policy(seed=3, tree="device")
        assert isinstance(pol.mcts, DeviceClassicMCTS)
        trace = []
        pol.run(3, trace=trace)
        torch.cuda.synchronize()
        pol.check()
        traces.append([tuple(host(x) for x in row) for row in trace])
        assert pol.mcts.stats == dict(searches=3, simulations=24)
        pol.env.close()
    moved = 0
    for before, has, actions, status, after, done, prev in traces[0]:
        assert np.all(status == 0)
        for e in range(4):
            if has[e] and not done[e]:
                assert abs(after[e] - (before[e] - action_costs(actions[e], prev[e], {"max_v": 2.0, "max_a": 2.0}))) < 1e-9
                moved += 1
    assert moved >= 8
    for x, y in zip(traces[0], traces[1]):  # the same seed: the same decisions, exactly
        for p, q in zip(x, y):
            assert np.array_equal(p, q)
    # the default tree on an equal env still runs as before
    pol = _vec_policy(seed=3, tree="host")
    trace = []
    pol.run(3, trace=trace)
    torch.cuda.synchronize()
    assert 0 < pol.mcts.stats["rollout_calls"] <= pol.mcts.stats["rounds"]
    assert all(np.all(host(row[3]) == 0) for row in trace)
    pol.check()
    pol.env.close()
