"""
What persisting the compact replay ring costs (IPPEngine.export_slots / import_slots, csrc/k_slots.h; Learner(persist_replay=True)):
the learn loop of tools/learn_bench.py --planes compact at its defaults, then, for the ring's archive (the slots that hold an episode):

    export_ms / import_ms   plan + export (with its one host read of the blob size) and import of all of them, wall time around a device
                            synchronisation, median of 3 after a warm-up; *_kernel_ms: the launches alone (CUDA events)
    blob_bytes              the packed records; columns_bytes = sum of rank x pstride x 4 of the exported slots
    replay_state_bytes      the size of replay_state.pt as the Learner wrote it (row arrays + the blob, on the host)
    fork_ms                 ipp_fork of the same slot list onto a rotation of itself, the yardstick that exists without this tool: it copies
                            rank x pstride floats per slot too, and the three map rows [Npad] on top (the archive is restored by the
                            import that is timed afterwards)

    python tools/slots_bench.py [--envs 8] [--iterations 2] [--episodes 2] [--sims 24] [--blocks 1] [--out FILE]

Prints one JSON line (and appends it to --out).  There is no speed bar: the numbers are a record.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from learn_bench import params  # noqa: E402


def median_ms(fn, sync, reps=3):
    import numpy as np

    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def median_event_ms(fn, reps=3):
    import numpy as np
    import torch

    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--sims", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    from ipp_rl_amd import EngineConfig, _ffi
    from ipp_rl_amd.planning.mcts_zero import Learner, PolicyValueNetwork
    from ipp_rl_amd.planning.mcts_zero.learn import REPLAY_FILE
    from ipp_rl_amd.planning.mcts_zero.selfplay import archive_slots_in_use

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
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
    md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(0)
    module = PolicyValueNetwork(net_hp, md).to("cuda:0")
    slots = a.iterations * a.episodes * (md["max_episode_steps"] + 1) + 1
    sync = torch.cuda.synchronize
    with tempfile.TemporaryDirectory() as tmp:
        lr = Learner(cfg, a.envs, hp, md, module, tmp, episodes_per_env=a.episodes, capacity=a.envs * slots, sims_in_flight=2, planes="compact",
                     persist_replay=True)
        t0 = time.perf_counter()
        lr.learn()
        learn_s = time.perf_counter() - t0
        state_bytes = os.path.getsize(os.path.join(tmp, REPLAY_FILE))
        t0 = time.perf_counter()
        lr._save_replay()
        sync()
        save_ms = 1e3 * (time.perf_counter() - t0)
        sp = lr.selfplay
        eng, ring = sp.env.engine, sp.replay
        used = archive_slots_in_use(ring.episodes.cpu().numpy(), ring.num_envs, ring.archive_episodes)
        ids = torch.as_tensor(used, dtype=torch.int32, device=eng.device)
        n = int(ids.numel())
        ranks = eng.ranks()[ids.long()].cpu().numpy()
        lay = eng.slot_layout()
        packed = eng.export_slots(ids, columns=True, maps=False)
        export_ms = median_ms(lambda: eng.export_slots(ids, columns=True, maps=False), sync)
        offsets, blob, status = packed["offsets"], packed["blob"], packed["status"]
        what = _ffi.IPP_SLOT_COLUMNS
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def kernels_export():
            _ffi.check(eng._lib.ipp_slots_plan(eng._h, ptr(ids), n, what, ptr(offsets), ptr(status), eng.stream))
            _ffi.check(eng._lib.ipp_slots_export(eng._h, ptr(ids), n, what, ptr(offsets), ptr(blob), eng.stream))

        export_kernel_ms = median_event_ms(kernels_export)
        rot = torch.roll(ids, 1)
        fork_ms = median_ms(lambda: eng.fork(ids, rot), sync)
        fork_kernel_ms = median_event_ms(lambda: eng.fork(ids, rot))
        # (the rotation scrambled the archive: the imports below put every slot back)
        import_ms = median_ms(lambda: eng.import_slots(ids, packed, check=True), sync)
        import_kernel_ms = median_event_ms(lambda: _ffi.check(eng._lib.ipp_slots_import(eng._h, ptr(ids), n, what, ptr(offsets), ptr(blob),
                                                                                         ptr(status), eng.stream)))
        again = eng.export_slots(ids, columns=True, maps=False)
        restored = bool(torch.equal(again["blob"], blob) and torch.equal(again["offsets"], offsets))
        out = dict(envs=a.envs, iterations=a.iterations, episodes_per_env=a.episodes, ring_rows=a.envs * slots, archive_slots=n,
                   engine_slots=int(eng.capacity), rank_cap=int(eng.rank_cap), pstride=lay["pstride"], rank_mean=round(float(np.mean(ranks)), 1),
                   rank_max=int(np.max(ranks)), blob_bytes=int(blob.numel()), columns_bytes=int(np.sum(ranks) * lay["pstride"] * 4),
                   cov_slot_bytes=int(eng.info.cov_slot_bytes), ring_bytes=ring.nbytes(), replay_state_bytes=int(state_bytes),
                   export_ms=round(export_ms, 3), export_kernel_ms=round(export_kernel_ms, 4), import_ms=round(import_ms, 3),
                   import_kernel_ms=round(import_kernel_ms, 4), fork_ms=round(fork_ms, 3), fork_kernel_ms=round(fork_kernel_ms, 4),
                   save_replay_state_ms=round(save_ms, 1), learn_s=round(learn_s, 2), restored=restored)
        lr.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not restored:
        raise SystemExit("the archive did not come back bit for bit")


if __name__ == "__main__":
    main()
