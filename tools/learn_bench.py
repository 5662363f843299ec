"""
Wall time of the learn loop (planning/mcts_zero/learn.py): iterations of self-play, training and the arena gate on the 40x40 split-field
configuration of tests/test_hip_per.py with a small network, and what the iteration bookkeeping costs a self-play step -- the CUDA-event
time of ipp_selfplay_commit_iter + ipp_selfplay_iter_totals + the pinned copy against ipp_selfplay_commit alone, on the same SelfPlay.

    python tools/learn_bench.py [--envs 8] [--iterations 2] [--episodes 2] [--sims 24] [--blocks 1] [--steps 12] [--out FILE]
                                [--planes {dense,compact}]

--planes selects the ring (dense planes per row, or the compact rows of csrc/k_replay_compact.h); "ring" in the output records its
device bytes, the phase that fills it, the archive launch and one minibatch draw (medians of 3 after a warm-up).

Prints one JSON line (and appends it to --out).  There is no speed bar: the numbers are a record.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def params(sims):
    hp = dict(gamma=0.9, puct_init=15.0, puct_base=10000.0, forced_playout_factor=2.0, max_valid_action_distance=6.5, dirichlet_alpha=1.0,
              dirichlet_eps=0.25, num_mcts_simulations=sims, temperature_scale=1.0, temperature_threshold=3, input_history_length=1,
              use_fov_input=False, use_action_costs_input=True, reset_mcts_each_step=True, use_per=False, shuffle_prior_cov=False,
              shuffle_budget=False)
    md = dict(initial_budget=200.0, max_episode_steps=4, episode_horizon=3, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0,
              uav_specifications={"max_v": 2.0, "max_a": 2.0}, scenario_info={"value_threshold": 0.4, "interval_factor": 0})
    return hp, md


def commit_cost(sp, steps):
    """Median CUDA-event time (ms) from the "commit" mark to the end of a step, plain and in an iteration, `steps` steps each."""
    import numpy as np
    import torch

    out = {}
    for name in ("commit", "commit_iter+totals"):
        if name != "commit":
            sp.begin_iteration(99, 10 ** 6)  # (a cap no env reaches: the same work per step, every episode kept)
        else:
            sp.reset()
        for _ in range(2):
            sp.step_iteration() if name != "commit" else sp.step()
        sp.timing = {}
        for _ in range(steps):
            sp.step_iteration() if name != "commit" else sp.step()
        torch.cuda.synchronize()
        ev, sp.timing = sp.timing, None
        out[name] = float(np.median([a.elapsed_time(b) for a, b in zip(ev["commit"], ev["end"])]))
    return out


def ring_cost(sp, batch, reps=3):
    """The ring in its mode (dense planes or compact rows), medians of `reps` after a warm-up (ms, CUDA events): the phase of a step that
    fills the ring, the archive launch between step and commit (compact only), one minibatch draw of `batch` rows; its device bytes."""
    import numpy as np
    import torch

    r = sp.replay
    sp.reset()
    sp.run(1)
    sp.timing = {}
    sp.run(reps)
    torch.cuda.synchronize()
    ev, sp.timing = sp.timing, None
    med = lambda a, b: float(np.median([s.elapsed_time(e) for s, e in zip(ev[a], ev[b])]))  # noqa: E731
    out = dict(mode="compact" if r.compact is not None else "dense", ring_bytes=r.nbytes(), fill_ms=round(med("planes", "search"), 4),
               archive_ms=round(med("archive", "commit"), 4) if "archive" in ev else None)
    r.sample(batch, check_empty=False)
    r.timing = []
    for _ in range(reps):
        r.sample(batch, check_empty=False)
    torch.cuda.synchronize()
    out.update(minibatch_rows=batch, minibatch_draw_ms=round(float(np.median([a.elapsed_time(b) for a, b in r.timing])), 4))
    r.timing = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--sims", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--planes", choices=["dense", "compact"], default="dense", help="the ring: dense planes or compact rows")
    ap.add_argument("--shuffle-prior", action="store_true",
                    help="shuffle_prior_cov: every self-play episode draws its own prior on the device (Learner(episode_priors='device'))")
    ap.add_argument("--simulation", default="split_random_field",
                    help="ground-truth kind (sensor.simulation.type); gaussian_random_field runs the 40x40 grid with grf_rows='all'")
    a = ap.parse_args()
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import Learner, PolicyValueNetwork

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation=a.simulation)
    grf = dict(grf_rows="all") if a.simulation == "gaussian_random_field" else {}
    hp, md = params(a.sims)
    net_hp = dict(input_channels=6, num_channels=8, dropout=0.0, use_silu=True, num_encoder_res_blocks=a.blocks, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=4, num_policy_head_conv_bn_blocks=1, num_value_head_conv_bn_blocks=1,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    train = dict(batch_size=8, num_augmented_samples=0, num_epochs=1, learning_rate=0.002, max_learning_rate=0.02, weight_decay=3e-5,
                 momentum=0.9, max_grad_norm=2.0, policy_loss_coeff=1.0, value_loss_coeff=1.0, reward_loss_coeff=1.0,
                 reconstruction_loss_coeff=1.0, entropy_regularization_coeff=0.01, replay_alpha=0.75, replay_beta0=0.4)
    loop = dict(shared_network=True, num_self_play_iterations=a.iterations, num_episodes=a.episodes, num_workers=a.envs, puct_init_decay=0.8,
                puct_init_min=4.0, dirichlet_alpha_decay=0.8, dirichlet_alpha_min=0.3, start_train_examples_history=1,
                train_examples_history_step=2, max_train_examples_history=10, continuous_network_update=False, num_arena_games=a.envs,
                network_update_threshold=0.5)
    hp = dict(hp, **net_hp, **train, **loop)
    hp["shuffle_prior_cov"] = bool(a.shuffle_prior)
    md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(0)
    module = PolicyValueNetwork(net_hp, md).to("cuda:0")
    slots = a.iterations * a.episodes * (md["max_episode_steps"] + 1) + 1  # every step of every iteration keeps its slot
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        lr = Learner(cfg, a.envs, hp, md, module, tmp, episodes_per_env=a.episodes, capacity=a.envs * slots, sims_in_flight=2,
                     planes=True if a.planes == "dense" else "compact", episode_priors="device" if a.shuffle_prior else None, **grf)
        build = time.perf_counter() - t0
        recs = lr.learn()
        sp = lr.selfplay
        cost = commit_cost(sp, a.steps)
        ring = ring_cost(sp, int(hp["batch_size"]))
        out = dict(ring=ring, simulation=a.simulation, shuffle_prior=bool(a.shuffle_prior), envs=a.envs, sims=a.sims, blocks=a.blocks, episodes_per_env=a.episodes, ring_rows=a.envs * slots,
                   ring_plane_gib=round(a.envs * slots * 6 * cfg.n_cells ** 2 * 4 / 2 ** 30, 2) if a.planes == "dense" else 0.0, build_s=round(build, 2),
                   iterations=[dict(iteration=r["iteration"], steps=r["totals"]["steps"], examples=r["totals"]["examples"],
                                    window_length=r["window_length"], evicted=r["evicted"],
                                    selfplay_s=round(r["seconds"]["selfplay"], 3), train_s=round(r["seconds"]["train"], 3),
                                    arena_s=round(r["seconds"]["update"], 3), accepted=r["arena"]["accepted"],
                                    selfplay_ms_per_step=round(1e3 * r["seconds"]["selfplay"] / r["totals"]["steps"], 2)) for r in recs],
                   commit_ms=round(cost["commit"], 4), commit_iter_totals_ms=round(cost["commit_iter+totals"], 4))
        lr.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
