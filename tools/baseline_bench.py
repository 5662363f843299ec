#!/usr/bin/env python3
"""Seconds per act() of the four batched baseline policies (planning/vec_baselines.py, ipp_baseline_act) and per MissionLog.curves()
(planning/mission_log.py: extent, the one host read, resample, reduce), beside the per-step time of the env they sit beside.  Every
figure is the median of `--reps` timed windows after a warm-up window; a window is `--calls` calls ending in a device synchronise (the
random kinds draw from Philox; budgets and cursors are restored between windows, outside the clock).  One JSON line.
usage: python tools/baseline_bench.py [--envs 4096] [--grid 50] [--levels 10] [--calls 50] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipp_rl_amd import EngineConfig  # noqa: E402
from ipp_rl_amd.planning import (MissionLog, VecLawnmowerPolicy, VecRandomContinuousPolicy, VecRandomDiscretePolicy,  # noqa: E402
                                 VecSpiralPolicy)
from ipp_rl_amd.vec_env import VecIPPEnv  # noqa: E402


def median_window(fn, restore, reps):
    times = []
    for i in range(reps + 1):  # (window 0 warms up)
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:])), [round(t, 6) for t in times[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--levels", type=int, default=10)
    ap.add_argument("--budget", type=float, default=400.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--log-steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("baseline_bench needs a GPU")
    cfg = EngineConfig(x_dim=args.grid, y_dim=args.grid)
    lo, hi = 5.0, 5.0 + (args.levels - 1)
    env = VecIPPEnv(cfg, args.envs, window_rows=-1, episode_steps=40, budget=args.budget, seed=11)
    env.reset()
    policies = {
        "lawnmower": VecLawnmowerPolicy(env, 10, lo, hi, 5, 1),
        "spiral": VecSpiralPolicy(env, 10, lo, hi, 200, 10),
        "random_discrete": VecRandomDiscretePolicy(env, 10, lo, hi, 1),
        "random_discrete_adaptive": VecRandomDiscretePolicy(env, 10, lo, hi, 1, adaptive=True),
        "random_continuous": VecRandomContinuousPolicy(env, 10, lo, hi),
    }
    out = {"tool": "baseline_bench", "grid": args.grid, "envs": args.envs, "levels": args.levels, "calls_per_window": args.calls,
           "actions_per_env": args.levels * args.grid * args.grid, "seconds_per_act": {}, "windows": {}}
    for name, pol in policies.items():
        def restore(pol=pol):
            env.budget.fill_(args.budget)
            pol.cursor.zero_()

        def window(pol=pol):
            for _ in range(args.calls):
                pol.act()

        med, all_ = median_window(window, restore, args.reps)
        out["seconds_per_act"][name] = med / args.calls
        out["windows"][name] = all_
    # the env's step beside them, and a log to resample: `log_steps` steps of the random-discrete policy
    pol = policies["random_discrete"]
    env.reset()
    log = MissionLog(env, args.log_steps + 1)
    log.record(first=True)
    torch.cuda.synchronize()
    t_step = 0.0
    for _ in range(args.log_steps):
        prev_before = env.prev.clone()
        actions, has = pol.act()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.step(actions, auto_reset=False)
        torch.cuda.synchronize()
        t_step += time.perf_counter() - t0
        log.record(prev_before, actions, has)
    out["seconds_per_env_step"] = t_step / args.log_steps
    curves = {}

    def run_curves():
        curves["out"] = log.curves(args.budget)

    med, all_ = median_window(run_curves, lambda: None, args.reps)
    out["seconds_per_curves"], out["windows"]["curves"] = med, all_
    out["curve_grid_points"] = int(curves["out"]["axis"].numel())
    out["log_points_per_env"] = float(log.count.double().mean())
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
