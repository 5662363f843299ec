"""
GPU test of the learn loop's persisted replay ring (Learner(persist_replay=True), planning/mcts_zero/learn.py: replay_state.pt beside
learn_state.pt) on the tiny learner of tests/test_hip_learn.py -- 40x40, 4 envs, 24 simulations, one episode per env, 2 iterations,
continuous update -- with the compact ring:
  * a resumed loop trains iteration 1 on the window (0, 1) with iteration 0's rows in it: window_length = both iterations' examples,
    nothing evicted (without the feature: its own examples only);
  * _resume() alone restores iteration 0's rows and their gathered outputs bit for bit;
  * a missing replay_state.pt is named, one of another iteration is refused.
Trained weights and losses are not compared between the two runs: the backward pass goes through the framework's convolution library,
which is not pinned to be run-to-run deterministic.  (The first backward pass of a process pays that library's one-time kernel selection,
as tests/test_hip_learn.py notes.)
"""
import os
import shutil

import pytest

from tests.test_hip_learn import SLOTS, _cfg
from tests.test_hip_per import _params
from tests.test_hip_replay_compact import bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def _learner(tmp, persist_replay=True):
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
    md = dict(md, num_grid_cells=cfg.n_cells)
    torch.manual_seed(3)
    module = PolicyValueNetwork(net_hp, md).to("cuda:0")
    learner = Learner(cfg, 4, hp, md, module, str(tmp), seed=6, capacity=4 * SLOTS, sims_in_flight=2, planes="compact",
                      persist_replay=persist_replay)
    assert learner.episodes_per_env == 1 and learner.selfplay.replay.compact is not None
    return learner


def test_a_resumed_loop_trains_on_the_whole_window(tmp_path):
    import torch

    a_dir, b_dir, c_dir, d_dir, e_dir = (tmp_path / x for x in "abcde")
    a = _learner(a_dir)
    r0 = a.learn(iterations=1)[0]
    assert r0["window"] == (0, 0) and r0["window_length"] == r0["totals"]["examples"] >= 4
    assert os.path.exists(a_dir / "replay_state.pt") and os.path.exists(a_dir / "learn_state.pt") and not os.path.exists(a_dir / "replay_state.pt.tmp")
    ring = a.selfplay.replay
    rows0 = ring.window(0, 0).rows().clone()
    gathered0 = [x.clone() for x in ring.gather_rows(rows0)]
    assert rows0.numel() == r0["totals"]["examples"] and torch.isfinite(gathered0[0]).all()
    for dst in (b_dir, c_dir, d_dir, e_dir):
        shutil.copytree(a_dir, dst)
    r1 = a.learn()[0]
    assert r1["window"] == (0, 1) and r1["window_length"] == r0["totals"]["examples"] + r1["totals"]["examples"] and r1["evicted"] == 0
    st = torch.load(a_dir / "replay_state.pt", map_location="cpu")
    assert st["iteration"] == 1 and not st["replay"]["flags"].is_cuda and not st["replay"]["archive"]["blob"].is_cuda
    a.close()
    # _resume() alone: iteration 0's rows are back, with their planes
    c = _learner(c_dir)
    c._resume()
    assert c.iteration == 0
    rows = c.selfplay.replay.window(0, 0).rows()
    assert torch.equal(rows, rows0)
    for x, y in zip(gathered0, c.selfplay.replay.gather_rows(rows)):
        assert bits_equal(x, y)
    assert int((c.selfplay.replay.flags == 1).sum().item()) == 0
    c.close()
    # the resumed loop: iteration 1 trains on both iterations' rows
    b = _learner(b_dir)
    rec = b.learn(resume=True)
    assert len(rec) == 1 and rec[0]["iteration"] == 1 and rec[0]["window"] == (0, 1)
    assert rec[0]["window_length"] == r0["totals"]["examples"] + rec[0]["totals"]["examples"]  # (without the persisted ring: its own only)
    assert rec[0]["evicted"] == 0
    assert torch.load(b_dir / "replay_state.pt", map_location="cpu")["iteration"] == 1
    b.close()
    # a missing file is named; the ring of another iteration is refused
    os.remove(d_dir / "replay_state.pt")
    d = _learner(d_dir)
    with pytest.raises(FileNotFoundError, match="replay_state.pt"):
        d.learn(resume=True)
    d.close()
    shutil.copy(a_dir / "replay_state.pt", e_dir / "replay_state.pt")  # (a's is behind iteration 1, e's learn_state.pt behind 0)
    e = _learner(e_dir)
    with pytest.raises(ValueError, match="iteration 1"):
        e.learn(resume=True)
    e.close()
