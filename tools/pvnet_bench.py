#!/usr/bin/env python3
"""
Timing of DevicePolicyValueNet.predict (csrc/k_pvnet.h) against the restated module under stock PyTorch on the same GPU.

Network: config/example.yaml's (16 input channels, 128 channels, 32 pooled, 10 separable blocks with context mixing, SiLU, 3 + 3 head
blocks), two altitude levels.  Shape: planes of --side (default 50), n = 4096 leaves, kmax = the valid actions within
max_valid_action_distance = 11.5 at resolution 4 (25 cells x 2 levels = 50).  Both precisions.  The yardstick is the module in eval
mode under no_grad, plus the dense softmax and the gather of INTEGRATION.md's stock `infer`.  Events on the current stream; every shape
warmed up; `--iters` timed calls per figure, the two sides alternating `--rounds` times so that a drift shows in the spread.

A second figure is the share of a search wave that leaf evaluation takes: a SelfPlay search (40 x 40 split field, 4 roots x 8
simulations, 2 in flight, one group of roots so that the phases do not overlap) with the same network at 6 input channels on the
engine's own planes ([n, 6, 1600, 1600]: a plane's side is the number of grid cells), events around the leaves' planes
(ipp_mcts_plane_entries + ipp_feature_planes), `infer` and the whole expansion, over the events around the search.

Usage:  python tools/pvnet_bench.py [--n 4096] [--side 50] [--iters 5] [--rounds 3] [--no-wave]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def conv_flops(plan, n):
    return sum(2.0 * n * op["hout"] * op["wout"] * op["cout"] * op["kh"] * op["kw"] * op["cin"] for op in plan.ops if op["kind"] == 0)


def wave_share(precision, searches=3):
    """Times of one search with net.infer, split into planes / infer / the rest of the expansion (ms per search, median of `searches`)."""
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork, SelfPlay

    cfg, B = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field"), 4
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=11.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.0, num_mcts_simulations=8, temperature_scale=1.0, temperature_threshold=3, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False, shuffle_budget=False)
    md = dict(initial_budget=40.0, max_episode_steps=6, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    net_hp = dict(input_channels=6, num_channels=128, dropout=0.0, use_silu=True, num_encoder_res_blocks=10, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=32, num_policy_head_conv_bn_blocks=3, num_value_head_conv_bn_blocks=3,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    net_md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(0)
    net = DevicePolicyValueNet(net_hp, net_md, PolicyValueNetwork(net_hp, net_md).eval().state_dict(), side=cfg.n_cells, precision=precision,
                               max_batch=8, device="cuda:0")
    marks = []

    def timed(fn, tag):
        def run(*a, **k):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn(*a, **k)
            t1.record()
            marks.append((tag, t0, t1))
            return out
        return run

    sp = SelfPlay(cfg, B, hp, md, infer=timed(net.infer, "infer"), seed=5, sims_in_flight=2, groups=1, planes=False)
    m, env = sp.mcts, sp.env
    m._leaf_planes, m._expand = timed(m._leaf_planes, "planes"), timed(m._expand, "expansion")
    rows = []
    for i in range(searches + 1):  # (the first search warms up)
        del marks[:]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        m.search_device(sp._roots, env.prev, env.budget, sp._temps, sp.tie_u, depth=0, root_history=env.history_entries())
        t1.record()
        torch.cuda.synchronize()
        part = {tag: sum(a.elapsed_time(b) for g, a, b in marks if g == tag) for tag in ("planes", "infer", "expansion")}
        rows.append(dict(search_ms=t0.elapsed_time(t1), planes_ms=part["planes"], infer_ms=part["infer"],
                         expand_rest_ms=part["expansion"] - part["planes"] - part["infer"], waves=sum(g == "infer" for g, _, _ in marks)))
    net.close()
    env.engine.close()
    med = {k: float(np.median([r[k] for r in rows[1:]])) for k in rows[0]}
    med["leaf_evaluation_share"] = (med["planes_ms"] + med["infer_ms"] + med["expand_rest_ms"]) / med["search_ms"]
    med["infer_share"] = med["infer_ms"] / med["search_ms"]
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--side", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-wave", action="store_true")
    args = ap.parse_args()
    import torch

    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork

    assert torch.cuda.is_available(), "pvnet_bench needs a GPU"
    n, side, levels = args.n, args.side, 2
    offs = [(dx, dy) for dx in range(-3, 4) for dy in range(-3, 4) if (4.0 * dx) ** 2 + (4.0 * dy) ** 2 <= 11.5 ** 2]
    kmax = len(offs) * levels
    hp = dict(input_channels=16, num_channels=128, dropout=0.0, use_silu=True, num_encoder_res_blocks=10, use_separable_conv_layers=True,
              use_global_context_mixing=True, num_global_pooling_channels=32, num_policy_head_conv_bn_blocks=3, num_value_head_conv_bn_blocks=3,
              mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    md = dict(num_grid_cells=side * side, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0)
    torch.manual_seed(0)
    module = PolicyValueNetwork(hp, md).eval()
    for m in module.modules():  # (statistics away from the identity: a network after training)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    sd = {k: v.clone() for k, v in module.state_dict().items()}
    A = module.num_actions
    rs = np.random.RandomState(0)
    planes = torch.from_numpy(rs.random_sample((n, 16, side, side)).astype(np.float32)).cuda()
    idx_np = np.stack([np.sort(rs.choice(A, size=kmax, replace=False)) for _ in range(n)]).astype(np.int32)
    idx = torch.from_numpy(idx_np).cuda()
    nets = {p: DevicePolicyValueNet(hp, md, sd, side=side, precision=p, max_batch=n, device="cuda:0") for p in ("fp32", "bf16")}
    module = module.cuda()

    def stock():
        with torch.no_grad():
            mask = torch.zeros((n, A), device="cuda")
            mask.scatter_(1, idx.long(), 1.0)
            lp, v, _, _ = module(planes, mask)
            return torch.exp(lp).gather(1, idx.long()).double(), (v * v + 2 * v).reshape(-1).double()

    runs = {"stock_pytorch": stock, "hip_fp32": lambda: nets["fp32"].predict(planes, idx), "hip_bf16": lambda: nets["bf16"].predict(planes, idx)}
    outs = {}
    for name, fn in runs.items():  # warm-up of every shape
        for _ in range(2):
            outs[name] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.iters)
    flops = conv_flops(nets["fp32"].plan, n)
    res = dict(n=n, side=side, kmax=kmax, conv_gflop=flops / 1e9)
    for name, ts in times.items():
        res[name] = dict(ms=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)), conv_tflops=flops / (np.median(ts) * 1e-3) / 1e12)
    for name in ("hip_fp32", "hip_bf16"):
        res[name]["max_abs_prior_vs_stock"] = float((outs[name][0] - outs["stock_pytorch"][0]).abs().max())
        res[name]["max_abs_value_vs_stock"] = float((outs[name][1] - outs["stock_pytorch"][1]).abs().max())
        res[name]["speedup_vs_stock"] = res["stock_pytorch"]["ms"] / res[name]["ms"]
    for net in nets.values():
        net.close()
    planes = module = nets = outs = None  # (the closures above keep the names: release what they hold)
    torch.cuda.empty_cache()
    if not args.no_wave:
        res["search_wave"] = {p: wave_share(p) for p in ("fp32", "bf16")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
