#!/usr/bin/env python3
"""
Phases of one decision of the batched MCTS-zero planner (planning/vec_mcts_zero.py, VecMctsZeroPolicy.step): search (DeviceMCTS for
envs x workers roots, read-out on the device), pick (ipp_play_pick), step (the fused budget step), tally (ipp_play_tally), totals
(ipp_play_totals + its copy to pinned memory), from events on the stream around each phase; the median of --reps steps after --warmup.

    python tools/deploy_bench.py [--envs 64] [--dim 50] [--workers 1 4] [--sims 256] [--reps 5] [--warmup 1] [--mode deploy]
                                 [--network] [--precision fp32]

--network: config/example.yaml's network (128 channels, 32 pooled, 10 separable blocks with context mixing, SiLU, 3 + 3 head blocks) as
the search's callback, on the engine's own planes.  A plane's side is the number of grid cells (a 50 x 50 grid: 2500 x 2500 per channel
and leaf), so this leg is for small batches of small grids (--envs 4 --dim 40 --sims 8).  Prints one JSON line per worker count.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ["search", "pick", "step", "tally", "totals", "end"]


def params(sims, steps, history):
    hp = dict(gamma=1.0, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=11.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.25, num_mcts_simulations=sims, temperature_scale=1.0, temperature_threshold=40, input_history_length=history,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=200.0, max_episode_steps=steps, episode_horizon=5, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    return hp, md


def example_network(cfg, md, channels, precision, max_batch):
    import torch

    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork

    net_hp = dict(input_channels=channels, num_channels=128, dropout=0.0, use_silu=True, num_encoder_res_blocks=10, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=32, num_policy_head_conv_bn_blocks=3, num_value_head_conv_bn_blocks=3,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    net_md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(0)
    return DevicePolicyValueNet(net_hp, net_md, PolicyValueNetwork(net_hp, net_md).eval().state_dict(), side=cfg.n_cells, precision=precision,
                                max_batch=max_batch, device="cuda:0")


def measure(a, workers):
    import numpy as np
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.feature_planes import PlaneSpec
    from ipp_rl_amd.planning import VecMctsZeroPolicy
    from ipp_rl_amd.planning.vec_mcts_zero import make_env

    cfg = EngineConfig(x_dim=a.dim, y_dim=a.dim) if a.dim in (50, 100) else EngineConfig(x_dim=a.dim, y_dim=a.dim, simulation="split_random_field")
    hp, md = params(a.sims, a.episode_steps, 1 if a.network else 3)
    env = make_env(cfg, a.envs, hp, md, workers=workers, sims_in_flight=a.in_flight, seed=1)
    net = None
    if a.network:
        spec = PlaneSpec.from_params(hp, md, adaptive=env.adaptive, use_flight_time=env.use_flight_time)
        net = example_network(cfg, md, spec.channels, a.precision, a.envs * workers * a.in_flight)
    pol = VecMctsZeroPolicy(env, hp, md, net.infer if net else None, workers=workers, mode=a.mode, games_per_env=1, sims_in_flight=a.in_flight)
    for _ in range(a.warmup):
        pol.step()
    pol.timing = {}
    for _ in range(a.reps):
        pol.step()
    torch.cuda.synchronize()
    ev, pol.timing = pol.timing, None
    split = {p: float(np.median([s.elapsed_time(e) for s, e in zip(ev[p], ev[q])])) for p, q in zip(PHASES[:-1], PHASES[1:])}
    whole = float(np.median([s.elapsed_time(e) for s, e in zip(ev["search"], ev["end"])]))
    new = split["pick"] + split["tally"] + split["totals"]
    out = {"envs": a.envs, "grid": a.dim, "workers": workers, "roots": a.envs * workers, "sims": a.sims, "mode": a.mode,
           "network": (a.precision if a.network else None), "reps": a.reps, "step_ms": whole, "split_ms": split,
           "pick_tally_totals_ms": new, "pick_tally_totals_share_of_step": new / whole, "pick_tally_totals_share_of_search": new / split["search"],
           "roots_with_policy_last_step": int(pol.last["ok"].sum().item()), "decisions_last_step": int((pol.forced == 0).sum().item())}
    if net is not None:
        net.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--sims", type=int, default=256)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--episode-steps", type=int, default=40)
    ap.add_argument("--mode", default="deploy", choices=["deploy", "arena"])
    ap.add_argument("--network", action="store_true")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "deploy_bench needs a GPU"
    for w in a.workers:
        print(json.dumps(measure(a, w)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
