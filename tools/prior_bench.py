#!/usr/bin/env python3
"""The prior kinds (EngineConfig.nu: Matern 1/2, 3/2, 5/2, RBF) on BASELINE configs[1] -- 4096 envs of 50x50, 10 altitude levels,
VecIPPEnv(window_rows=-1) at the kind's smallest fixed-prior window -- one JSON line per (nu, parts): ms per env step and env-steps/s.
The window sets the patch area a step streams: nu = 0.5 runs at R = 14 (patches of 34 x 35 cells), 1.5 at 10, 2.5 at 8, inf at 10 (the Matern 3/2 rule).

usage: python tools/prior_bench.py [--steps K] [--warmup W] [--parts 1 2]
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
from ipp_rl_amd.vec_env import VecIPPEnv, cell_centre_actions  # noqa: E402

ALTITUDES = [float(a) for a in range(5, 15)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--parts", type=int, nargs="+", default=[1, 2])
    a = ap.parse_args()
    B, T = a.envs, 40
    for nu in (0.5, 1.5, 2.5, float("inf")):
        cfg = EngineConfig(x_dim=50, y_dim=50, nu=nu)
        acts = [torch.as_tensor(cell_centre_actions(cfg, t, 0, B, B, ALTITUDES), device="cuda:0") for t in range(T)]
        for parts in a.parts:
            env = VecIPPEnv(cfg, B, episode_steps=T, stagger=True, window_rows=-1, seed=1, parts=parts)
            env.reset()

            def step(t):
                if parts > 1:
                    env.step_async(acts[t % T])
                else:
                    env.step(acts[t % T])

            for t in range(a.warmup):
                step(t)
            env.wait()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(a.warmup, a.warmup + a.steps):
                step(t)
            env.wait()
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            info = env.engine.info
            print(json.dumps({"nu": str(nu), "prior": env.engine.prior_kernel, "window_rows": int(info.window_rows),
                              "patch_layout": int(info.patch_layout), "envs": B, "parts": parts, "steps": a.steps,
                              "ms_per_step": 1e3 * sec / a.steps, "env_steps_per_s": B * a.steps / sec}), flush=True)
            env.close()
            del env


if __name__ == "__main__":
    main()
