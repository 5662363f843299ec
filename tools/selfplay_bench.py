"""
Throughput of the batched self-play loop (planning/mcts_zero/selfplay.py): samples/s and the split of a step into its phases --
planes (ipp_feature_planes into the ring), search (DeviceMCTS, read-out on the device), record (ipp_selfplay_record), step (the fused
budget step), commit (ipp_selfplay_commit) -- plus one replay minibatch (gather, ipp_replay_gather), from CUDA events around each phase,
and a prioritised-replay leg on the big ring: the PER minibatch (ipp_replay_mass + ipp_replay_draw_per, then ipp_replay_gather_rows)
against the uniform minibatch (the committed prefix count + ipp_replay_gather) at the same n, alternating.

    python tools/selfplay_bench.py [--envs 4096] [--dim 50] [--sims 100] [--steps 8] [--warmup 2] [--planes-envs 8]
                                   [--per-batch 1024] [--per-reps 20] [--planes {dense,compact}] [--simulation KIND]

The 4096-env run keeps no planes (a 50x50 plane is 25 MB per channel): its planes phase is reported as not measured; the planes phase
and the gather kernel (CUDA events around the ipp_replay_gather launch alone, one minibatch of --batch rows with one augmented copy) are
timed on a second, small batch (--planes-envs) with planes in its ring.  --planes compact gives that batch the compact ring
(csrc/k_replay_compact.h); "ring" in the output records the ring's device bytes, the phase that fills it, the archive launch and one
minibatch draw in the chosen mode (medians of 3 after a warm-up).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def params(sims, steps):
    hp = dict(gamma=1.0, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=11.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.25, num_mcts_simulations=sims, temperature_scale=1.0, temperature_threshold=40, input_history_length=3,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=200.0, max_episode_steps=steps, episode_horizon=5, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    return hp, md


def timed(sp, steps):
    import torch

    sp.timing = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sp.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ev = sp.timing
    sp.timing = None
    order = ["planes", "search", "record", "step"] + (["archive"] if "archive" in ev else []) + ["commit", "end"]
    split = {}
    for a, b in zip(order[:-1], order[1:]):
        split[a] = sum(s.elapsed_time(e) for s, e in zip(ev[a], ev[b])) / steps
    return wall, split


def per_leg(sp, n, reps):
    """Prioritised against uniform minibatches of n rows on sp's ring, alternating, medians of `reps` (ms, CUDA events).  The rows
    recorded so far are committed by hand (40-step episodes have not ended after a few steps: their value targets are not final, which
    no timing depends on); the scan covers every ring row, committed or not."""
    import numpy as np
    import torch

    from ipp_rl_amd.planning.mcts_zero.selfplay import COMMITTED, PENDING

    r = sp.replay
    r.flags[r.flags == PENDING] = COMMITTED
    per = r.prioritized(batch_size=n)
    rows = torch.nonzero(per.priorities > 0).reshape(-1)
    per.update(rows, torch.rand(rows.numel(), dtype=torch.float64, device=rows.device) + 1e-8)  # (non-uniform priorities)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for _ in range(3):
        r.sample(n, check_empty=False)
        per.sample()
    uni_total, uni_kernel, per_total, per_draw, per_gather = [], [], [], [], []
    for _ in range(reps):
        r.timing, per.timing = [], []
        a, b, c = ev(), ev(), ev()
        a.record()
        r.sample(n, check_empty=False)
        b.record()
        batch = per.sample()
        idx = batch[5]
        per.update(idx, batch[2].abs() + 1e-8)
        c.record()
        torch.cuda.synchronize()
        uni_total.append(a.elapsed_time(b))
        uni_kernel.append(r.timing[0][0].elapsed_time(r.timing[0][1]))
        per_total.append(b.elapsed_time(c))
        per_draw.append(per.timing[0][0].elapsed_time(per.timing[0][1]))
        per_gather.append(per.timing[0][1].elapsed_time(per.timing[0][2]))
    r.timing, per.timing = None, None
    med = lambda v: float(np.median(v))  # noqa: E731
    return {"ring_rows": r.capacity, "sampled_rows": len(per), "n": n, "reps": reps,
            "uniform_minibatch_ms": med(uni_total), "uniform_gather_kernel_ms": med(uni_kernel),
            "per_minibatch_and_update_ms": med(per_total), "per_mass_and_draw_ms": med(per_draw), "per_gather_rows_ms": med(per_gather)}


def ring_leg(small, batch, reps=3):
    """What the ring costs in its mode (dense planes or compact rows), medians of `reps` after a warm-up (ms, CUDA events): the phase of
    a step that fills the ring (ipp_feature_planes into the row, or ipp_replay_record_compact), the archive launch between step and
    commit (compact only) and one minibatch draw of `batch` rows with one augmented copy (the gather; compact: + the planes of the
    drawn rows).  And the ring's device bytes."""
    import numpy as np
    import torch

    r = small.replay
    small.run(1)
    small.timing = {}
    small.run(reps)
    torch.cuda.synchronize()
    ev, small.timing = small.timing, None
    med = lambda a, b: float(np.median([s.elapsed_time(e) for s, e in zip(ev[a], ev[b])]))  # noqa: E731
    out = {"mode": "compact" if r.compact is not None else "dense", "envs": small.num_envs, "ring_rows": r.capacity,
           "ring_bytes": r.nbytes(), "fill_ms": med("planes", "search"),
           "archive_ms": med("archive", "commit") if "archive" in ev else None}
    r.sample(batch, num_augmented_samples=1, check_empty=False)
    r.timing = []
    for _ in range(reps):
        r.sample(batch, num_augmented_samples=1, check_empty=False)
    torch.cuda.synchronize()
    out["minibatch_rows"] = batch
    out["minibatch_draw_ms"] = float(np.median([a.elapsed_time(b) for a, b in r.timing]))
    r.timing = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--episode-steps", type=int, default=40)
    ap.add_argument("--planes-envs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--per-batch", type=int, default=1024)
    ap.add_argument("--per-reps", type=int, default=20)
    ap.add_argument("--planes", choices=["dense", "compact"], default="dense", help="the small batch's ring: dense planes or compact rows")
    ap.add_argument("--shuffle-prior", action="store_true",
                    help="shuffle_prior_cov: every episode draws its own prior on the device (SelfPlay(episode_priors='device'))")
    ap.add_argument("--window-rows", type=int, default=-1,
                    help="column window of the envs' engines (-1: the smallest the prior allows; 12 = the shuffled priors' window without them)")
    ap.add_argument("--simulation", default=None,
                    help="ground-truth kind (sensor.simulation.type): gaussian_random_field, hotspot_random_field or split_random_field; "
                         "default: EngineConfig's.  A Gaussian random field on a grid other than 50 / 100 runs with grf_rows='all'")
    a = ap.parse_args()
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    cfg = EngineConfig(x_dim=a.dim, y_dim=a.dim) if a.simulation is None else EngineConfig(x_dim=a.dim, y_dim=a.dim, simulation=a.simulation)
    hp, md = params(a.sims, a.episode_steps)
    hp["shuffle_prior_cov"] = bool(a.shuffle_prior)
    kw = dict(episode_priors="device" if a.shuffle_prior else None, window_rows=a.window_rows)
    if cfg.simulation == "gaussian_random_field" and a.dim not in (50, 100):
        kw["grf_rows"] = "all"
    sp = SelfPlay(cfg, a.envs, hp, md, planes=False, seed=1, **kw)
    sp.run(a.warmup)
    wall, split = timed(sp, a.steps)
    window_rows = int(sp.env.engine.info.window_rows)
    ended = int((~torch.isnan(sp.episode_values)).sum().item())
    with_policy = int(sp.last["ok"].sum().item())
    per = per_leg(sp, a.per_batch, a.per_reps)
    sp.close()
    del sp
    # the planes phase with planes in the ring (small batch, history 3, cost plane: 16 channels) and 3-step episodes, so that rows are
    # committed and one minibatch with one augmented copy is gathered (ipp_replay_gather)
    hp3, md3 = params(a.sims, 3)
    hp3["shuffle_prior_cov"] = bool(a.shuffle_prior)
    small = SelfPlay(cfg, a.planes_envs, hp3, md3, planes=True if a.planes == "dense" else "compact", seed=1, **kw)
    small.run(1)
    _, split_small = timed(small, 3)
    small.replay.timing = []
    batch = small.replay.sample(a.batch, num_augmented_samples=1, check_empty=False)
    torch.cuda.synchronize()
    gather_ms = small.replay.timing[0][0].elapsed_time(small.replay.timing[0][1])  # (the ipp_replay_gather kernel alone)
    small.replay.timing = None
    gathered_rows = int((batch[5] >= 0).sum().item())
    ring = ring_leg(small, a.batch)
    small.close()
    split["planes"] = "not measured: the 4096-env batch keeps no planes (planes=False); see planes_ms_small_batch"
    out = {"envs": a.envs, "grid": a.dim, "simulation": cfg.simulation, "grf_rows": kw.get("grf_rows"), "sims": a.sims, "steps": a.steps, "shuffle_prior": bool(a.shuffle_prior), "window_rows": window_rows,
           "samples_per_s": a.envs * a.steps / wall,
           "step_ms": 1e3 * wall / a.steps, "split_ms": split, "episodes_ended_last_step": ended,
           "roots_with_policy_last_step": with_policy, "gather_kernel_ms_small_batch": gather_ms, "gathered_rows": gathered_rows,
           "prioritised_replay": per, "ring": ring,
           "planes_ms_small_batch": {"envs": a.planes_envs, "planes": split_small["planes"], "record": split_small["record"],
                                     "step": split_small["step"]}}  # (3-step episodes: these steps reset envs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
