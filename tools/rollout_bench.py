"""
Times one replan of the classic MCTS planner (planning/mcts_mission.py::ClassicMCTS.replan) for R roots searched in lock step:
  (a) batched=True: device rollouts (csrc/k_rollout.h, planning/device_rollout.py), one ipp_tree_score_nodes call per round
  (b) the default path on a band-tile engine with score_scratch: host rollouts, one ipp_tree_score_actions per scoring request
  (c) the tree on the device as well (csrc/k_ctree.h, planning/device_ctree.py DeviceClassicMCTS.search): no host read in the search;
      on the engine of (a), same roots, counts and protocol -- a replan includes drawing and uploading its uniform tables
and splits a rollout level of (a) into its five calls with device events.

  python tools/rollout_bench.py [--roots 1,16,64] [--sims 100] [--horizon 5] [--reps 3] [--skip-default-above 64] [--out profiles/ctree_bench.txt]

Roots: 50x50 grids after three measurements, budget 60, altitudes 8 / 14, greedy radius 9 m (98 candidates per node).  Per R the
median and the min / max of `reps` replans after one warm-up replan, wall clock with the device drained (a replan is host-driven: its
host time is part of what a user waits for).  The paths consume their random streams differently, so they do not search the same
trees; simulations, horizon and candidate sets are the same.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
UAV = {"max_v": 2, "max_a": 2}
ALTS, RADIUS, BUDGET, ROOT_STEPS = (8.0, 14.0, 6.0), 9.0, 60.0, 3


def build(R, sims, horizon, batched):
    from ipp_rl_amd import EngineConfig, IPPEngine

    cfg = EngineConfig(x_dim=50, y_dim=50)
    kw = dict(capacity=R, state="factor", rank_cap=9 * (ROOT_STEPS + horizon + 2), window_rows=-1, fixed_prior=True)
    if batched:
        eng = IPPEngine(cfg, node_capacity=R * (sims + horizon), max_batch=max(512, min(4096, R * 98)), **kw)
    else:
        old = os.environ.get("IPP_PATCH")
        os.environ["IPP_PATCH"] = "0"  # the band-tile kernels: the engine the default path's scorer was built for
        try:
            eng = IPPEngine(cfg, node_capacity=R * (sims * (horizon + 1) + 8), max_batch=512, score_scratch=True, **kw)
        finally:
            if old is None:
                del os.environ["IPP_PATCH"]
            else:
                os.environ["IPP_PATCH"] = old
    rs = np.random.RandomState(5)
    eng.reset(white_noise=rs.normal(size=(R, 50, 50)))
    prev = np.tile([2.0, 2.0, 14.0], (R, 1))
    for _ in range(ROOT_STEPS):
        acts = np.stack([4.0 * rs.randint(0, 50, R) + 2.0, 4.0 * rs.randint(0, 50, R) + 2.0, np.full(R, 8.0)], axis=1)
        eng.step(acts, prev, meas_noise=rs.normal(size=(R, 9)))
        prev = acts
    return cfg, eng, prev


def planner(cfg, eng, sims, horizon, batched):
    from ipp_rl_amd.planning.mcts_mission import ClassicMCTS

    return ClassicMCTS(eng, cfg, UAV, *ALTS, num_simulations=sims, episode_horizon=horizon, max_greedy_radius=RADIUS, adaptive=True,
                       batched=batched)


def time_replan(torch, mcts, R, prev, reps):
    out = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mcts.replan(list(range(R)), prev, [BUDGET] * R, py_seeds=list(range(R)))
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        print(f"    replan {rep}: {out[-1]:.3f} s", flush=True)
    return np.array(out[1:])


def device_planner(cfg, eng, sims, horizon, R):
    from ipp_rl_amd.planning import DeviceClassicMCTS

    return DeviceClassicMCTS(eng, cfg, UAV, *ALTS, num_simulations=sims, episode_horizon=horizon, max_greedy_radius=RADIUS, adaptive=True, roots=R)


def time_device_replan(torch, mcts, R, prev, reps):
    from ipp_rl_amd.planning.device_ctree import uniform_tables

    out = []
    wps = torch.as_tensor(np.asarray(prev, dtype=np.float64), device=mcts.engine.device)
    budgets = torch.full((R,), BUDGET, dtype=torch.float64, device=mcts.engine.device)
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = uniform_tables(np.random.RandomState(100 + rep), mcts.num_simulations, R, mcts.episode_horizon)
        mcts.search(list(range(R)), wps, budgets, u)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        mcts.check()
        print(f"    device-tree replan {rep}: {out[-1]:.3f} s", flush=True)
    return np.array(out[1:])


def level_split(torch, eng, R, prev, horizon, reps=3):
    """ms per call of a rollout level for R rollouts from the roots, summed over the levels of a rollout: device events around every call."""
    from ipp_rl_amd.planning.device_rollout import DeviceRollout

    ro = DeviceRollout(eng, *ALTS, UAV, RADIUS, 0.95, 0.5, False, horizon, 0)
    names = ("candidates", "score", "pick", "step", "advance")
    total = np.zeros(len(names))
    rs = np.random.RandomState(9)
    for rep in range(reps + 1):
        ro.load(list(range(R)), [[] for _ in range(R)], prev, [BUDGET] * R, [horizon] * R, rs.random_sample((R, horizon, 2)))
        marks = []
        for level in range(horizon):
            for name, call in zip(names, (ro.candidates, ro.score, lambda: ro.pick(level), ro.step, ro.advance)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); call(); b.record()
                marks.append((name, a, b))
        torch.cuda.synchronize()
        if rep:
            for name, a, b in marks:
                total[names.index(name)] += a.elapsed_time(b) / reps
    return dict(zip(names, total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", default="1,16,64")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-default-above", type=int, default=64, help="0 skips (b) everywhere")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    lines = [f"ClassicMCTS.replan, R roots of 50x50 in lock step: {args.sims} simulations, horizon {args.horizon}, radius {RADIUS} m, altitudes "
             f"{ALTS[0]:.0f} / {ALTS[1]:.0f}; seconds per replan, median [min, max] of {args.reps} after one warm-up",
             "R   | (a) batched, device rollouts | (b) default path, band-tile engine | (b) / (a) | (a) rounds, rollout calls, score calls | "
             "(c) device tree | (a) / (c) | [min, max] of (c) wholly below that of (a)"]
    split_lines = ["", f"One rollout ({args.horizon} levels) of R rollouts started at the roots, ms per call summed over the levels (device events, "
                   "mean of 3 after a warm-up); share of the level's time",
                   "R   | candidates | score (ipp_tree_score_nodes) | pick | step (ipp_tree_step) | advance"]
    for R in [int(x) for x in args.roots.split(",")]:
        print(f"R = {R}: batched", flush=True)
        cfg, eng, prev = build(R, args.sims, args.horizon, True)
        mcts = planner(cfg, eng, args.sims, args.horizon, True)
        ta = time_replan(torch, mcts, R, prev, args.reps)
        st = dict(mcts.stats)
        per = args.reps + 1
        print(f"R = {R}: device tree", flush=True)
        tc = time_device_replan(torch, device_planner(cfg, eng, args.sims, args.horizon, R), R, prev, args.reps)
        sp = level_split(torch, eng, R, prev, args.horizon)
        eng.close()
        tot = sum(sp.values())
        split_lines.append(f"{R:3d} | " + " | ".join(f"{sp[k]:.3f} ms ({100 * sp[k] / tot:.1f} %)" for k in sp))
        tb = None
        if R <= args.skip_default_above:
            print(f"R = {R}: default path", flush=True)
            cfg, eng, prev = build(R, args.sims, args.horizon, False)
            assert int(eng.info.patch_layout) == 0
            tb = time_replan(torch, planner(cfg, eng, args.sims, args.horizon, False), R, prev, args.reps)
            eng.close()
        b_txt = f"{np.median(tb):8.3f} [{tb.min():.3f}, {tb.max():.3f}]" if tb is not None else "not run"
        ratio = f"{np.median(tb) / np.median(ta):.2f}" if tb is not None else "-"
        lines.append(f"{R:3d} | {np.median(ta):8.3f} [{ta.min():.3f}, {ta.max():.3f}] | {b_txt} | {ratio} | {st['rounds'] // per}, "
                     f"{st['rollout_calls'] // per}, {st['score_calls'] // per} | {np.median(tc):8.3f} [{tc.min():.3f}, {tc.max():.3f}] | "
                     f"{np.median(ta) / np.median(tc):.2f} | {'yes' if tc.max() < ta.min() else 'NO'}")
        print(lines[-1], flush=True)
    text = "\n".join(lines + split_lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
