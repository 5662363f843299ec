#!/usr/bin/env python3
"""Budget mode (VecIPPEnv(budget=B0): device-side ledger, resets on done inside the step launch, refill generator behind every step)
next to the fixed schedule, in the same process, one JSON line per configuration:

  fixed      VecIPPEnv(stagger=True): episodes of exactly max_episode_steps, resets on the host's schedule
  budget_eq  budget = 1e30 with the same stagger: the SAME episodes (tests/test_hip_budget.py) -- the ledger's and the refill's cost
  budget     budget = 200 (config/example.yaml), shuffle_budget: episodes end where the budget runs out (many more resets per step)
  refill_ms  one ipp_generate_grf_refill launch over the batch's positions on the last step's refill list (timed alone)

usage: python tools/budget_bench.py [--steps K] [--warmup W] [--quick]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ipp_rl_amd import EngineConfig  # noqa: E402
from ipp_rl_amd.vec_env import VecIPPEnv  # noqa: E402


def run(env, acts, steps, warmup):
    env.reset()
    for t in range(warmup):
        env.step(acts[t % len(acts)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step(acts[(warmup + t) % len(acts)])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def refill_ms(env, reps=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):  # (re-stages the same envs' next fields: same numbers, same planes)
        env.engine.generate_grf_refill(env.num_envs, env.refill, env.episode, env.seed, env.GT_STREAM, row_offset=env.env_id_offset)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=80)
    ap.add_argument("--quick", action="store_true", help="the 50x50 configurations only")
    a = ap.parse_args()
    configs = [(50, 4096, 1), (50, 4096, 2)] + ([] if a.quick else [(100, 32768, 1)])
    for dim, B, parts in configs:
        cfg = EngineConfig(x_dim=dim, y_dim=dim)
        rs = np.random.RandomState(0)
        acts = [torch.as_tensor(np.stack([4.0 * rs.randint(0, dim, B) + 2.0, 4.0 * rs.randint(0, dim, B) + 2.0,
                                          rs.choice([8.0, 14.0], B)], axis=1), device="cuda:0") for _ in range(16)]
        line = {"grid": f"{dim}x{dim}", "envs": B, "parts": parts, "steps": a.steps, "warmup": a.warmup}
        for tag, kw in (("fixed", {}), ("budget_eq", dict(budget=1e30)), ("budget", dict(budget=200.0, shuffle_budget=True))):
            env = VecIPPEnv(cfg, B, episode_steps=40, stagger=True, window_rows=-1, seed=1, parts=parts, **kw)
            sec = run(env, acts, a.steps, a.warmup)
            line[tag + "_env_steps_per_s"] = B * a.steps / sec
            line[tag + "_ms_per_step"] = 1e3 * sec / a.steps
            if tag == "budget":
                line["budget_done_per_step"] = int(env.done.sum())
                line["refill_ms"] = refill_ms(env)
            env.close()
            del env
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
