#!/usr/bin/env python3
"""Seconds per VecCmaesPolicy.plan() (planning/vec_cmaes.py): the greedy look-ahead plus max_iter generations of ask / plan / fork /
horizon covariance-only step launches / objective / tell for `envs` envs at once, and how often the refined trajectory beat greedy's.
The envs carry `--steps` executed measurements; the plan is timed `--reps` times after one warm-up plan, each ending in a device
synchronise.  One JSON line.
usage: python tools/cmaes_bench.py [--envs 64] [--popsize 12] [--horizon 10] [--max-iter 32] [--grid 50] [--budget 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipp_rl_amd import EngineConfig  # noqa: E402
from ipp_rl_amd.planning import VecCmaesPolicy  # noqa: E402
from ipp_rl_amd.vec_env import VecIPPEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--popsize", type=int, default=12)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--max-iter", type=int, default=32)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--budget", type=float, default=200.0)
    ap.add_argument("--steps", type=int, default=4, help="executed measurements before the plan")
    ap.add_argument("--altitudes", type=float, nargs=3, default=[8.0, 14.0, 6.0], metavar=("MIN", "MAX", "SPACING"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cmaes_bench needs a GPU")
    cfg = EngineConfig(x_dim=args.grid, y_dim=args.grid)
    n, lam = args.envs, args.popsize
    slots = n * (1 + lam)
    env = VecIPPEnv(cfg, slots, window_rows=-1, episode_steps=40, seed=11)
    env.reset()
    rs = np.random.RandomState(0)
    for _ in range(args.steps):
        a = np.stack([cfg.resolution * (rs.randint(0, cfg.x_dim, slots) + 0.5), cfg.resolution * (rs.randint(0, cfg.y_dim, slots) + 0.5),
                      np.array(args.altitudes[:2])[rs.randint(0, 2, slots)]], axis=1)
        env.step(a, auto_reset=False)
    policy = VecCmaesPolicy(env, *args.altitudes, horizon=args.horizon, max_iter=args.max_iter, popsize=lam)
    ids, scratch = np.arange(n), n + np.arange(n * lam)
    budget = torch.full((n,), args.budget, dtype=torch.float64, device=env.device)

    def plan():
        out = policy.plan(ids, scratch, budget)
        torch.cuda.synchronize()
        return out

    plan()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ways, valid, info = plan()
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    policy.greedy.search(ids, scratch[:n], budget, args.horizon)
    torch.cuda.synchronize()
    greedy_s = time.perf_counter() - t0
    chose = info["chose_cma"].double()
    gain = (info["utility_cma"] - info["utility_greedy"])[info["chose_cma"]]
    print(json.dumps({
        "tool": "cmaes_bench", "grid": args.grid, "patch_layout": int(env.engine.info.patch_layout), "envs": n, "popsize": lam,
        "horizon": args.horizon, "max_iter": args.max_iter, "budget": args.budget, "altitudes": args.altitudes,
        "seconds_per_plan": float(np.median(times)), "seconds_per_plan_all": [round(t, 4) for t in times],
        "seconds_greedy_lookahead": greedy_s, "prediction_steps_per_plan": n * lam * args.horizon * args.max_iter,
        "prediction_steps_per_second": n * lam * args.horizon * args.max_iter / float(np.median(times)),
        "fraction_chose_cma": float(chose.mean()), "mean_utility_gain_where_chosen": float(gain.mean()) if gain.numel() else 0.0,
        "breakdowns": int((info["status"] != 0).sum()),
    }))
    env.close()


if __name__ == "__main__":
    main()
