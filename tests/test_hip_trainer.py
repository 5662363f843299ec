"""
GPU tests of Trainer (ipp_rl_amd/planning/mcts_zero/training.py) with fused=True: the forward and backward of the module through
PyTorch, ipp_pvnet_loss and ipp_pvnet_sgd_step (csrc/k_train.h) around them.
  * Three steps on pvnet case "b" (side 13, 16 channels, dropout 0, batch 8; the first minibatches of the recorded uniform reference
    run.  Those of the recorded PER run cannot serve: on them the stock loop is bistable by itself -- two identical stock runs on the
    MI355X differed by 4.4e-6, 300 ulp of the stem's weights, and every rounding-level change of the loss or of the update moves a CPU
    run by exactly that amount: a ReLU / max-pool decision at a tie -- so d_ref below came out as 1.8e-7 or 4.4e-6 from run to run)
    against a stock-torch loop of the reference's own expressions on the GPU, from the same weights.  The bar is 4 x d_ref, d_ref
    measured here from stock runs only: the largest parameter difference between the loss evaluated in float32 and in float64, or
    between two identical stock runs if that is larger (backward convolutions need not be deterministic).  The fused path differs from
    either stock run by roundings of the same kind (the loss gradients, the norm), hence the factor 4.
  * One tiny SelfPlay (the 40 x 40 configuration of test_hip_per.py) until rows are committed, then a one-epoch Trainer.train on its
    ring, uniform and PER: finite losses, the PER priorities equal to the drawn rows' value_loss + 1e-8 (last occurrence wins), and
    hand_over changes what DevicePolicyValueNet.predict returns.
  * A step calls neither torch.cuda.synchronize nor Tensor.item / Tensor.cpu / Tensor.tolist.
"""
import numpy as np
import pytest

from tests import pvnet_cases as pc
from tests import training_cases as tc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

STEPS, SCHEDULE = 3, 6


def host(t):
    return t.detach().cpu().numpy()


def _network(hp, md):
    import torch

    from ipp_rl_amd.planning.mcts_zero import PolicyValueNetwork

    net = PolicyValueNetwork(hp, md)
    net.load_state_dict({k: v.clone() for k, v in pc.case(tc.E2E_CASE)["state_dict"].items()}, strict=True)
    return net.to(torch.device("cuda:0"))


def _flat(net):
    """The parameters as one float64 vector (named_parameters order)."""
    import torch

    return torch.cat([p.detach().double().reshape(-1) for _, p in net.named_parameters()]).cpu().numpy()


def _worst(net, a, b, k=3):
    """Names of the k parameters where the flat vectors a and b differ most (for the printed report)."""
    out, o = [], 0
    for name, p in net.named_parameters():
        n = p.numel()
        out.append((float(np.max(np.abs(a[o:o + n] - b[o:o + n]))), name, float(np.max(np.abs(a[o:o + n])))))
        o += n
    return sorted(out, reverse=True)[:k]


def _batches():
    import torch

    fx = tc.fixture()
    return [tc.e2e_batch(fx["e2e_uni_ids"][s], fx["e2e_uni_index"][s], fx["e2e_uni_weights"][s], torch.float64, device="cuda:0")
            for s in range(STEPS)]


def _stock_run(hp, md, batches, loss_dtype):
    """The reference's loop (policy_value_network_wrappers.py:51-69, :98-173) on the GPU, its loss expressions evaluated in loss_dtype."""
    import torch

    net = _network(hp, md)
    opt = torch.optim.SGD(net.parameters(), lr=hp["learning_rate"], weight_decay=hp["weight_decay"], momentum=hp["momentum"])
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=hp["max_learning_rate"], total_steps=SCHEDULE,
                                              div_factor=hp["max_learning_rate"] / hp["learning_rate"], final_div_factor=100,
                                              anneal_strategy="linear", three_phase=True, pct_start=0.40)
    net.train()
    for states, pol, val, rew, msk, index, weights in batches:
        logits, value, _, _ = net.forward_logits(states)
        m, t = msk.to(loss_dtype), pol.to(loss_dtype)
        log_p = torch.log_softmax(logits.to(loss_dtype) - (1 - m) * 1000, dim=1)  # (PolicyHead.forward after its head)
        pl = -torch.sum(t * log_p * m, dim=1)
        vl = torch.square(value.to(loss_dtype).view(-1) - val.float().to(loss_dtype))
        total = hp["policy_loss_coeff"] * pl + hp["value_loss_coeff"] * vl
        total = total - hp["entropy_regularization_coeff"] * -torch.sum(torch.exp(log_p) * log_p, dim=1)
        total = total * weights.to(loss_dtype)
        opt.zero_grad()
        total.mean().backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=hp["max_grad_norm"], norm_type=2)
        opt.step()
        sch.step()
    return _flat(net)


def test_three_fused_steps_against_the_stock_loop():
    import torch

    from ipp_rl_amd.planning.mcts_zero import Trainer

    hp, md = tc.e2e_params()
    batches = _batches()
    start = _flat(_network(hp, md))
    s32, s32b, s64 = _stock_run(hp, md, batches, torch.float32), _stock_run(hp, md, batches, torch.float32), _stock_run(hp, md, batches, torch.float64)
    d_prec, d_rep = float(np.max(np.abs(s32 - s64))), float(np.max(np.abs(s32 - s32b)))
    d_ref = max(d_prec, d_rep)
    net = _network(hp, md)
    trainer = Trainer(net, hp, fused=True)
    trainer.set_schedule(SCHEDULE)
    for b in batches:
        trainer.step(b)
    got = _flat(net)
    diff = float(np.max(np.abs(got - s32)))
    moved = float(np.max(np.abs(s32 - start)))
    print(f"d_ref = {d_ref:.3e} (f32 against f64 loss {d_prec:.3e}, two identical stock runs {d_rep:.3e}); fused against stock {diff:.3e}; "
          f"against the f64-loss stock run {np.max(np.abs(got - s64)):.3e}; the three steps moved the parameters by {moved:.3e}")
    print("largest differences (difference, parameter, its largest magnitude):", _worst(net, got, s32))
    assert d_ref > 0 and moved > 1e3 * d_ref  # (the steps train: the bar is far below what they change)
    assert diff <= 4 * d_ref
    # the flat buffers are the parameters: every trained parameter is a view of trainer.flat, its .grad of trainer.gflat
    lo, hi = trainer.flat.data_ptr(), trainer.flat.data_ptr() + 4 * trainer.flat.numel()
    used = [p for p in net.parameters() if p.grad is not None]
    assert used and all(lo <= p.data_ptr() < hi for p in used) and sum(p.numel() for p in used) == trainer.flat.numel()
    means = trainer.epoch_means()
    assert all(np.isfinite(v) for v in means.values()) and means["grad_norm"] > 0 and means["reward_loss"] == 0.0


def test_a_step_reads_nothing_from_the_device(monkeypatch):
    import torch

    from ipp_rl_amd.planning.mcts_zero import Trainer

    hp, md = tc.e2e_params()
    batches = _batches()
    trainer = Trainer(_network(hp, md), hp, fused=True)
    trainer.set_schedule(SCHEDULE)
    calls = []

    def counted(name, fn):
        def wrapper(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    for b in batches:  # (the first step, which builds the flat buffers, included)
        assert trainer.step(b) is None
    assert calls == []
    monkeypatch.undo()
    assert np.isfinite(host(trainer.last_value_losses)).all()


def test_a_replaced_gradient_is_refused():
    import torch

    from ipp_rl_amd.planning.mcts_zero import Trainer

    hp, md = tc.e2e_params()
    batches = _batches()
    net = _network(hp, md)
    trainer = Trainer(net, hp, fused=True)
    trainer.set_schedule(SCHEDULE)
    trainer.step(batches[0])
    p = next(q for q in net.parameters() if q.grad is not None)
    p.grad = torch.zeros_like(p)  # (what optimizer.zero_grad(set_to_none) followed by a backward would leave: a new tensor)
    with pytest.raises(RuntimeError, match="flat buffers"):
        trainer.step(batches[1])


def test_selfplay_train_hand_over():
    import torch

    from ipp_rl_amd import EngineConfig
    from ipp_rl_amd.planning.mcts_zero import DevicePolicyValueNet, PolicyValueNetwork, Trainer
    from ipp_rl_amd.planning.mcts_zero.selfplay import per_update
    from tests.test_hip_per import _params, _selfplay

    cfg = EngineConfig(x_dim=40, y_dim=40, simulation="split_random_field")
    hp, md = _params()
    sp = _selfplay(4, True, slots=6, seed=6)  # (test_hip_per.py's ring with planes: 4 envs, episodes of 4 steps)
    sp.run(5)
    committed = len(sp.replay)
    assert committed >= 4
    net_hp = dict(input_channels=sp.spec.channels, num_channels=8, dropout=0.0, use_silu=True, num_encoder_res_blocks=7, use_separable_conv_layers=True,
                  use_global_context_mixing=True, num_global_pooling_channels=4, num_policy_head_conv_bn_blocks=1, num_value_head_conv_bn_blocks=1,
                  mask_policy_head=True, use_reward_target=False, use_autoencoder=False)
    net_md = dict(md, num_grid_cells=cfg.n_cells)
    train_hp = dict(net_hp, **tc.E2E_TRAIN)
    train_hp.update(batch_size=4, num_epochs=1)
    torch.manual_seed(3)
    module = PolicyValueNetwork(net_hp, net_md).to(sp.device)
    device_net = DevicePolicyValueNet(net_hp, net_md, module.state_dict(), side=cfg.n_cells, max_batch=2, device="cuda:0")
    rows = sp.replay.committed_rows()[:2]
    planes, idx = sp.replay.planes[rows], sp.replay.idx[rows]
    before = [host(t) for t in device_net.predict(planes, idx)]
    for use_per in (False, True):
        trainer = Trainer(module, dict(train_hp, use_per=use_per), fused=True)
        seen = []
        step = trainer.step

        def recording(batch):
            step(batch)
            seen.append((batch[5], trainer.last_value_losses))

        trainer.step = recording
        history = trainer.train(sp.replay)
        assert len(history) == 1 and len(seen) == committed // 4
        print(f"use_per = {use_per}: {len(seen)} steps, {history[0]}")
        assert all(np.isfinite(v) for v in history[0].values()) and history[0]["policy_loss"] > 0 and history[0]["value_loss"] > 0
        if use_per:
            per = trainer.per
            want = np.where(host(sp.replay.flags) == 2, 1.0 / committed, 0.0)
            for index, vl in seen:
                assert (host(index) >= 0).all()
                want = per_update(want, host(index), host(vl) + 1e-8)
            assert np.array_equal(host(per.priorities), want)
            assert per.beta == pytest.approx(1.0)
    trainer.hand_over(device_net)
    after = [host(t) for t in device_net.predict(planes, idx)]
    assert np.isfinite(after[0]).all() and np.isfinite(after[1]).all()
    assert not np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])
    device_net.close()
    sp.close()
