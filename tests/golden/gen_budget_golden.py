#!/usr/bin/env python3
"""
Generate tests/golden/budget.npz by IMPORTING the reference (/root/reference, read-only) and running its self-play episode loop
(planning/mcts_zero/episode_generators.py:109-150) over the action sequences of the episode_*_50_* fixtures:

    remaining_budget = budget
    while depth < max_episode_steps and remaining_budget >= grid_map.resolution:
        ...
        remaining_budget -= action_costs(action, previous_action, uav_specifications)
        depth += 1

Recorded per (episode fixture, cost mode, start budget): the remaining budget after every one of the 40 actions (charged as the loop
would if it went on) and the number of steps the loop takes with max_episode_steps = 40.  Cost modes: the distance
(uav_specifications = None) and the flight time with tests/params.py's UAV (max_v = 2, max_a = 2).  Start budgets end the episode
early, mid-way and not at all.  The actions start from INIT_ACTION = (2, 2, 14), as in those fixtures.

Usage:  python tests/golden/gen_budget_golden.py        (writes tests/golden/budget.npz; gen_golden.py is not touched)
"""
import os
import sys

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden")

if not os.path.isdir(REF):
    sys.exit("reference checkout not present: golden vectors can only be generated in the build container")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

from planning.common.actions import action_costs  # noqa: E402

EPISODES = ("episode_rf1_50_s0", "episode_mixed_50_s1")
MODES = (("distance", None), ("flight_time", {"max_v": 2, "max_a": 2}))
MAX_STEPS, RESOLUTION = 40, 4
INIT_ACTION = np.array([2.0, 2.0, 14.0])


def reference_loop(actions, budget, uav):
    """The reference's loop, step by step: (remaining budget after each action, charged for all of them; steps the loop takes)."""
    remaining, depth, steps = float(budget), 0, None
    prev = INIT_ACTION
    out = []
    for a in actions:
        if steps is None and not (depth < MAX_STEPS and remaining >= RESOLUTION):
            steps = depth
        remaining -= action_costs(a, prev, uav)
        depth += 1
        out.append(remaining)
        prev = a
    if steps is None:
        steps = depth if not (depth < MAX_STEPS and remaining >= RESOLUTION) else MAX_STEPS
    return np.array(out), steps


def main():
    arrays = {}
    for name in EPISODES:
        acts = np.load(os.path.join(OUT, name + ".npz"))["actions"]
        for mode, uav in MODES:
            total = float(reference_loop(acts, 0.0, uav)[0][-1] * -1.0)
            # early, mid-way, never (the loop ends at max_episode_steps): round numbers away from the thresholds
            budgets = np.array([np.floor(0.2 * total) + 0.5, np.floor(0.6 * total) + 0.5, np.ceil(2.0 * total) + 100.0])
            rem, steps = [], []
            for b in budgets:
                r, s = reference_loop(acts, b, uav)
                rem.append(r)
                steps.append(s)
            key = f"{name}__{mode}"
            arrays[key + "__budget"] = budgets
            arrays[key + "__remaining"] = np.stack(rem)
            arrays[key + "__steps"] = np.array(steps, dtype=np.int64)
            print(f"  {key}: total cost {total:.3f}, budgets {budgets.tolist()}, steps {steps}")
    path = os.path.join(OUT, "budget.npz")
    np.savez_compressed(path, **arrays)
    print(f"  budget.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
