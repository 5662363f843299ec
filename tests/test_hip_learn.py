"""
GPU tests of the learn loop (planning/mcts_zero/learn.py; SelfPlay.run_iteration, ReplayBuffer.window, DeviceMCTS.set_exploration) on the
40x40 split-field configuration of tests/test_hip_per.py (24 simulations, episodes of 4 steps), without planes unless stated:
  * the iteration rule: exactly `cap` kept episodes per env, the reported rows are the tagged rows, nothing of a later episode is
    committed, a window draws only its iterations' rows;
  * sharding: one process of 4 envs against two of 2: every kept row and its action equal bit for bit;
  * set_exploration gives the search of a freshly constructed DeviceMCTS (groups 1 and 2);
  * the loop with planes and a tiny network: checkpoints, schedules, hand-over, resume; the gate rejecting and accepting;
  * an iteration step reads the device no more often than a plain step, apart from its totals (an event wait on pinned memory).
"""
import os
import shutil

import numpy as np
import pytest

from tests.test_hip_per import _params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

SLOTS = 12  # an iteration of 2 episodes per env takes at most 2 x (4 + 1) steps


def host(t):
    return t.detach().cpu().numpy()


def _cfg():
    from ipp_rl_amd import EngineConfig

    return EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")


def _selfplay(B, slots=SLOTS, seed=3, env_id_offset=0, groups=2, **over):
    from ipp_rl_amd.planning.mcts_zero import SelfPlay

    hp, md = _params(**over)
    return SelfPlay(_cfg(), B, hp, md, planes=False, capacity=B * slots, seed=seed, env_id_offset=env_id_offset, groups=groups)


def test_iteration_rule_and_windows():
    sp = _selfplay(4, slots=2 * SLOTS)
    ring = sp.replay
    assert len(ring.window(0, 9)) == 0 and np.all(host(ring.iter) == -1)  # (a ring that never saw an iteration)
    with pytest.raises(ValueError, match="self-play iterations 0 .. 9"):
        ring.window(0, 9).sample(4)
    tot = sp.run_iteration(0, 2)
    assert tot["episodes_kept"] == 8 and tot["envs_at_cap"] == 4 and 1 <= tot["steps"] <= 10
    n, flags, tags = host(sp.iter_episodes), host(ring.flags), host(ring.iter)
    assert np.all(n >= 2) and np.all(np.minimum(n, 2) == 2)
    rows0 = np.nonzero((flags == 2) & (tags == 0))[0]
    assert tot["examples"] == len(rows0) == int(host(sp.iter_examples).sum()) > 0
    assert np.array_equal(np.nonzero(flags == 2)[0], rows0)  # (every committed row is a tagged one: nothing of a third episode)
    per_env = np.bincount(rows0 % 4, minlength=4)
    assert np.array_equal(per_env, host(sp.iter_examples)) and np.all(per_env <= 2 * 4)
    ev = host(sp.iter_value_sum)
    assert np.all(np.isfinite(ev)) and np.all(ev >= 0) and ev.sum() > 0 and abs(tot["value_sum"] - ev.sum()) < 1e-12
    w = ring.window(0, 0)
    assert len(w) == len(rows0) and np.array_equal(host(w.rows()), rows0)
    batch = w.sample(64)
    assert set(host(batch[5]).tolist()) <= set(rows0.tolist()) and len(set(host(batch[5]).tolist())) > 1
    assert np.array_equal(host(batch[2]), host(ring.value)[host(batch[5])])
    per = w.prioritized(batch_size=4, num_epochs=1)
    assert len(per) == len(rows0) and set(host(per.sample()[5]).tolist()) <= set(rows0.tolist())
    # a second iteration: new episodes (the env's counters went on), its own tag
    epi0 = host(sp.env.episode).copy()
    tot1 = sp.run_iteration(1, 2)
    assert np.all(host(sp.env.episode) > epi0) and tot1["envs_at_cap"] == 4
    flags, tags = host(ring.flags), host(ring.iter)
    rows1 = np.nonzero((flags == 2) & (tags == 1))[0]
    assert len(rows1) == tot1["examples"] and np.array_equal(host(ring.window(1, 1).rows()), rows1)
    assert not set(rows1.tolist()) & set(rows0.tolist())
    both = host(ring.window(0, 1).rows())
    assert np.array_equal(both, np.sort(np.concatenate([rows0, rows1]))) and len(ring.window(0, 1)) == len(rows0) + len(rows1)
    assert set(host(ring.window(1, 1).sample(64)[5]).tolist()) <= set(rows1.tolist())
    assert len(ring) == len(both)  # (the whole-ring view is what it was: every committed row)
    with pytest.raises(RuntimeError, match="max_steps"):
        sp.run_iteration(2, 2, max_steps=1)
    sp.close()


def _iteration_trace(sp, cap):
    """Run iteration 0 step by step; returns the action index of every (step, env)."""
    sp.begin_iteration(0, cap)
    acts = []
    while sp.iteration_totals["envs_at_cap"] < sp.num_envs:
        sp.step_iteration()
        acts.append(host(sp.action_idx).copy())
        assert len(acts) <= cap * (sp.max_episode_steps + 1)
    return np.stack(acts)


def test_two_shards_keep_the_rows_of_one_process():
    one = _selfplay(4, dirichlet_eps=0.25)
    two = [_selfplay(2, env_id_offset=o, dirichlet_eps=0.25) for o in (0, 2)]
    acts1 = _iteration_trace(one, 2)
    kept = 0
    f1, t1 = host(one.replay.flags).reshape(SLOTS, 4), host(one.replay.iter).reshape(SLOTS, 4)
    for sh, off in zip(two, (0, 2)):
        acts2 = _iteration_trace(sh, 2)
        f2, t2 = host(sh.replay.flags).reshape(SLOTS, 2), host(sh.replay.iter).reshape(SLOTS, 2)
        assert np.array_equal(f1[:, off:off + 2] == 2, f2 == 2) and np.array_equal(t1[:, off:off + 2][f2 == 2], t2[f2 == 2])
        assert np.array_equal(host(one.iter_examples)[off:off + 2], host(sh.iter_examples))
        assert np.array_equal(host(one.iter_value_sum)[off:off + 2], host(sh.iter_value_sum))
        for name in ("policy", "idx", "value", "reward"):
            a = host(getattr(one.replay, name)).reshape((SLOTS, 4) + getattr(one.replay, name).shape[1:])[:, off:off + 2]
            b = host(getattr(sh.replay, name)).reshape((SLOTS, 2) + getattr(sh.replay, name).shape[1:])
            assert np.array_equal(a[f2 == 2].view(np.uint8), b[f2 == 2].view(np.uint8)), name
        for s, e in zip(*np.nonzero(f2 == 2)):  # (a kept row of step s: both processes ran that step)
            assert acts1[s, off + e] == acts2[s, e] >= 0
            kept += 1
    assert kept == int(host(one.iter_examples).sum()) > 0
    for sp in [one] + two:
        sp.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_set_exploration_equals_a_fresh_search(groups):
    old = _selfplay(4, groups=groups, dirichlet_eps=0.25)
    new = _selfplay(4, groups=groups, dirichlet_eps=0.25, puct_init=4.0, dirichlet_alpha=0.3)

    def search(sp):
        out = sp.mcts.search_device(sp._roots, sp.env.prev, sp.env.budget, sp._temps, sp.tie_u, depth=0)
        return [host(p).copy() for p in out["policy"]] + [host(out["valid_idx"]).copy(), host(out["ok"]).copy()]

    first = search(old)                      # (builds the tables, and with groups = 2 the sub-searches, from 15 / 1.0)
    old.mcts.set_exploration(4.0, 0.3)
    second, want = search(old), search(new)
    assert all(np.array_equal(a, b) for a, b in zip(second, want))
    assert not all(np.array_equal(a, b) for a, b in zip(first, want))  # (the values do reach the search)
    assert (old.mcts._subs is not None) == (groups == 2)
    # ... and before the first search (nothing allocated yet)
    early = _selfplay(4, groups=groups, dirichlet_eps=0.25)
    early.mcts.set_exploration(4.0, 0.3)
    assert all(np.array_equal(a, b) for a, b in zip(search(early), want))
    for sp in (old, new, early):
        sp.close()


def test_an_iteration_step_reads_the_device_no_more_than_a_step(monkeypatch):
    import torch

    plain, it = _selfplay(4, seed=9), _selfplay(4, seed=9)
    it.begin_iteration(0, 5)
    plain.reset()  # (as begin_iteration did: both play the same episodes)
    calls = []

    def counted(name, fn):
        def wrapper(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    for _ in range(3):
        plain.step()
    base = list(calls)
    del calls[:]
    for _ in range(3):
        tot = it.step_iteration()
    monkeypatch.undo()
    # the search's own reads (its error word once per search) and nothing else: the totals come through pinned memory and an event
    assert calls == base and "synchronize" not in calls
    assert tot["envs_at_cap"] == 0 and tot["examples"] == int(host(it.iter_examples).sum())
    assert np.array_equal(host(plain.replay.flags), host(it.replay.flags)) and np.array_equal(host(plain.replay.value), host(it.replay.value))
    plain.close()
    it.close()


# ---------------------------------------------------------------------------------------------------- the loop
def _learner(tmp, **over):
    import torch

    from ipp_rl_amd.planning.mcts_zero import Learner, PolicyValueNetwork
    from tests import training_cases as tc

    cfg = _cfg()
    hp, md = _params()
    net_hp = dict(input_channels=6, num_channels=8, dropout=0.0, use_silu=True, num_encoder_res_blocks=7, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=4, num_policy_head_conv_bn_blocks=1, num_value_head_conv_bn_blocks=1,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    hp = dict(hp, **net_hp, **tc.E2E_TRAIN)
    hp.update(batch_size=4, num_epochs=1, shared_network=True, num_self_play_iterations=2, num_episodes=1, num_workers=4,
              puct_init_decay=0.8, puct_init_min=4.0, dirichlet_alpha_decay=0.8, dirichlet_alpha_min=0.3,
              start_train_examples_history=2, train_examples_history_step=2, max_train_examples_history=10,
              continuous_network_update=True, num_arena_games=4, network_update_threshold=0.52)
    hp.update(over)
    md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(3)
    module = PolicyValueNetwork(net_hp, md).to("cuda:0")
    learner = Learner(cfg, 4, hp, md, module, str(tmp), seed=6, capacity=4 * SLOTS, sims_in_flight=2)
    assert learner.episodes_per_env == 1
    return learner


def _load_fresh(path, like):
    import torch

    from ipp_rl_amd.planning.mcts_zero import PolicyValueNetwork

    net = PolicyValueNetwork(like.module.hyper_params, like.md)
    net.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    return net


def _same_weights(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(np.array_equal(host(sa[k]).reshape(-1).view(np.uint8), host(sb[k]).reshape(-1).view(np.uint8)) for k in sa)


def _probe(learner):
    rows = learner.selfplay.replay.window(0, 99).rows()[:2]
    return learner.selfplay.replay.planes[rows].clone(), learner.selfplay.replay.idx[rows].clone()


def test_two_iterations_checkpoints_schedule_and_resume(tmp_path):
    """Three iterations of 4 envs x 1 episode in all: about 4 s.  The first backward pass of a process adds the convolution library's
    one-time kernel selection (about 30 s) to whichever test trains first -- this one, or tests/test_hip_trainer.py when run alone."""
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    a = _learner(a_dir)
    seen = []
    rec0 = a.learn(iterations=1, on_iteration=seen.append)
    assert len(rec0) == 1 and seen == rec0 and rec0[0]["iteration"] == 0
    shutil.copytree(a_dir, b_dir)
    planes, idx = _probe(a)
    before = [host(t) for t in a.search_net.predict(planes, idx)]
    rec1 = a.learn()
    assert len(rec1) == 1 and [r["iteration"] for r in a.history] == [0, 1]
    r0, r1 = a.history
    assert (r0["puct_init"], r0["dirichlet_alpha"]) == (15.0, 1.0) and (r1["puct_init"], r1["dirichlet_alpha"]) == (12.0, 0.8)
    assert a.selfplay.mcts.puct_init == 12.0 and a.selfplay.mcts.alpha == 0.8
    assert r0["window"] == (0, 0) and r1["window"] == (0, 1)
    assert r0["window_length"] == r0["totals"]["examples"] >= 4 and r0["evicted"] == 0
    assert r1["window_length"] == r0["totals"]["examples"] + r1["totals"]["examples"] and r1["evicted"] == 0
    assert r0["totals"]["episodes_kept"] == 4 and r0["arena"] is None
    for r in (r0, r1):
        assert len(r["epochs"]) == 1 and all(np.isfinite(v) for v in r["epochs"][0].values()) and r["epochs"][0]["policy_loss"] > 0
    for name in ("shared_net.temp.pth.tar", "shared_net.snapshot_0.pth.tar", "shared_net.snapshot_1.pth.tar", "shared_net.trained_model.pth.tar",
                 "learn_state.pt"):
        assert os.path.exists(a_dir / name), name
    assert _same_weights(_load_fresh(a_dir / "shared_net.trained_model.pth.tar", a), a.module)
    assert _same_weights(_load_fresh(a_dir / "shared_net.snapshot_1.pth.tar", a), a.module)
    assert not _same_weights(_load_fresh(a_dir / "shared_net.snapshot_0.pth.tar", a), a.module)
    assert _same_weights(_load_fresh(a_dir / "shared_net.temp.pth.tar", a), _load_fresh(a_dir / "shared_net.snapshot_0.pth.tar", a))
    after = [host(t) for t in a.search_net.predict(planes, idx)]
    assert np.isfinite(after[0]).all() and not np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])
    assert a.learn() == []  # (num_self_play_iterations are done)
    episodes_a = host(a.selfplay.env.episode).copy()
    a.close()
    # resume behind iteration 0 in a fresh process' stead: the schedule applied once, the deployed weights, an empty window
    b = _learner(b_dir)
    rec = b.learn(resume=True)
    assert len(rec) == 1 and rec[0]["iteration"] == 1 and (rec[0]["puct_init"], rec[0]["dirichlet_alpha"]) == (12.0, 0.8)
    assert rec[0]["window"] == (0, 1) and rec[0]["window_length"] == rec[0]["totals"]["examples"]
    assert rec[0]["evicted"] == r0["totals"]["examples"]  # (the ring is not persisted: iteration 0's rows are gone)
    assert np.array_equal(host(b.selfplay.env.episode), episodes_a)  # (the episodes of iteration 1, not those of iteration 0 again)
    assert os.path.exists(b_dir / "shared_net.snapshot_1.pth.tar")
    b.close()


@pytest.mark.parametrize("threshold", [2.0, 0.0])
def test_the_gate_rejects_and_accepts(tmp_path, threshold):
    lr = _learner(tmp_path, continuous_network_update=False, network_update_threshold=threshold, num_self_play_iterations=1)
    assert lr.arena_envs == 4
    initial = {k: host(v).copy() for k, v in lr.module.state_dict().items()}
    rec = lr.learn()[0]
    planes, idx = _probe(lr)
    verdict = rec["arena"]
    assert verdict["accepted"] is (threshold == 0.0) and verdict["total_prev"] > 0 and verdict["total_curr"] > 0
    deployed = _load_fresh(tmp_path / "shared_net.trained_model.pth.tar", lr)
    temp = _load_fresh(tmp_path / "shared_net.temp.pth.tar", lr)
    snap = _load_fresh(tmp_path / "shared_net.snapshot_0.pth.tar", lr)
    assert all(np.array_equal(host(v), initial[k]) for k, v in temp.state_dict().items()) and not _same_weights(snap, temp)
    search = [host(t) for t in lr.search_net.predict(planes, idx)]
    trained = [host(t) for t in lr.trained_net.predict(planes, idx)]
    if threshold == 2.0:  # rejected: the module is the temp checkpoint again, the search plays on with the old weights
        assert _same_weights(lr.module, temp) and _same_weights(deployed, temp) and verdict["prev_network_wins"] == 1
        assert not np.array_equal(search[0], trained[0])
        lr.trainer.hand_over(lr.trained_net)  # (now the module's = the old weights: what the search net must still hold)
        old = [host(t) for t in lr.trained_net.predict(planes, idx)]
        assert np.array_equal(search[0], old[0]) and np.array_equal(search[1], old[1])
    else:                 # accepted: deployed and handed over
        assert _same_weights(lr.module, snap) and _same_weights(deployed, snap) and verdict["prev_network_wins"] == 0
        assert np.array_equal(search[0], trained[0]) and np.array_equal(search[1], trained[1])
    lr.close()
