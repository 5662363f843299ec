"""
Trainer: the training station of the MCTS-zero loop (PolicyValueNetworkWrapper.train, planning/mcts_zero/network_wrappers/
policy_value_network_wrappers.py:34-215) on the device, with no host read inside an iteration.

One Trainer.step(batch) is one iteration of the reference's inner loop:

    forward     PolicyValueNetwork.forward_logits in train mode, through PyTorch                                       (:116-118)
    loss        the masked log-softmax, policy / value / reward losses, entropy, the weighted total AND the gradient of the batch
                mean with respect to the logits, the value and the reward, one launch                  (:120-154; ipp_pvnet_loss)
    backward    torch.autograd.backward([logits, value, ...], [those gradients]) into ONE flat gradient buffer            (:167-168)
    update      clip_grad_norm_(max_norm, 2) and SGD with momentum and weight decay at the one-cycle schedule's (lr, momentum) on the
                flat parameter / gradient / momentum buffers, two launches                        (:169-173; ipp_pvnet_sgd_step)

Trainer.train(replay) runs the epochs over a SelfPlay ring (uniform minibatches, or prioritised with use_per: per.step() then
per.update(indices, value_loss + 1e-8) after every optimizer step, :174-175) and reads the accumulated losses once per epoch.
Trainer.hand_over(device_net) gives the new weights to the search (DevicePolicyValueNet.load_state_dict).

Host restatements (the oracle of the GPU tests and what tests/test_training_host.py pins to the reference): pv_losses_host,
sgd_clip_step_host, one_cycle.  fused=False runs the reference's stock-torch expressions and torch.optim.SGD instead of the two calls
(also on the CPU): the yardstick of the fused path.

Divergences from the reference (INTEGRATION.md "Training"): the fused loss and update compute in fp64 from the fp32 loads (the reference
in fp32; its total norm is an fp32 norm of per-tensor fp32 norms); the parameters that receive a gradient live in one flat buffer;
targets are rounded to fp32 like the reference's torch.FloatTensor; no TensorBoard writer, no checkpoint files.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

STAT_NAMES = ("policy_loss", "value_loss", "reward_loss", "entropy", "total_loss", "value_relative")
MASK_SHIFT = 1000.0              # layers.py:343-344: logits - (1 - valid_actions_msk) * 1000
PCT_START, FINAL_DIV = 0.40, 100.0  # the reference's OneCycleLR call (:59-69)
BASE_MOMENTUM, MAX_MOMENTUM = 0.85, 0.95  # OneCycleLR's defaults: cycle_momentum=True overrides hyper_params["momentum"]


# ---------------------------------------------------------------------------------------------------- host restatements
def pv_losses_host(logits, target_policy, valid_msk, value, reward, target_value, target_reward, weights, policy_coeff, value_coeff,
                   reward_coeff, entropy_coeff) -> Dict[str, np.ndarray]:
    """ipp_pvnet_loss in fp64 NumPy: stats [n, 6] (STAT_NAMES) and the UNROUNDED gradients of the batch mean, grad_logits [n, A],
    grad_value [n], grad_reward [n] (None without reward).  target_value / target_reward are rounded to float32 first."""
    z = np.asarray(logits, dtype=np.float64)
    t = np.asarray(target_policy, dtype=np.float64)
    m = np.asarray(valid_msk, dtype=np.float64)
    n, A = z.shape
    v = np.asarray(value, dtype=np.float64).reshape(n)
    tv = np.asarray(target_value, dtype=np.float64).reshape(n).astype(np.float32).astype(np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(n)
    pc, vc, rc, ec = float(policy_coeff), float(value_coeff), float(reward_coeff), float(entropy_coeff)
    zs = z - (1.0 - m) * MASK_SHIFT
    mx = zs.max(axis=1, keepdims=True)
    lp = zs - (mx + np.log(np.exp(zs - mx).sum(axis=1, keepdims=True)))
    p = np.exp(lp)
    tm = t * m
    pl = -(tm * lp).sum(axis=1)
    H = -(p * lp).sum(axis=1)
    T = tm.sum(axis=1)
    vl = (v - tv) ** 2
    if reward is not None:
        r = np.asarray(reward, dtype=np.float64).reshape(n)
        tr = np.asarray(target_reward, dtype=np.float64).reshape(n).astype(np.float32).astype(np.float64)
        rl = (r - tr) ** 2
    else:
        rl = np.zeros(n)
    total = (pc * pl + vc * vl + rc * rl - ec * H) * w
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(tv - v) / np.abs(tv)
    wn = w / n
    out = dict(stats=np.stack([pl, vl, rl, H, total, rel], axis=1),
               grad_logits=wn[:, None] * (pc * (T[:, None] * p - tm) + ec * (p * (lp + H[:, None]))),
               grad_value=wn * (2.0 * vc * (v - tv)), grad_reward=None)
    if reward is not None:
        out["grad_reward"] = wn * (2.0 * rc * (r - tr))
    return out


def sgd_clip_step_host(params, grads, momentum_buf, lr, momentum, weight_decay, max_norm):
    """ipp_pvnet_sgd_step in fp64 NumPy: (params', momentum_buf') as float32 and the norm before clipping.  clip_grad_norm_(max_norm, 2),
    then SGD with dampening 0 and no Nesterov; one rounding per stored value."""
    p = np.asarray(params, dtype=np.float32).astype(np.float64)
    g = np.asarray(grads, dtype=np.float32).astype(np.float64)
    b = np.asarray(momentum_buf, dtype=np.float32).astype(np.float64)
    norm = float(np.sqrt((g * g).sum()))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = float(max_norm) / (norm + 1e-6)
    coef = c if (c < 1.0 or c != c) else 1.0
    with np.errstate(invalid="ignore"):
        g2 = coef * g + float(weight_decay) * p
        b2 = float(momentum) * b + g2
        p2 = p - float(lr) * b2
    return p2.astype(np.float32), b2.astype(np.float32), norm


def one_cycle(step: int, total_steps: int, lr0: float, max_lr: float):
    """(lr, momentum) the optimizer holds at its step number `step` (0-based) under the reference's scheduler (:59-69):
    OneCycleLR(max_lr, total_steps, div_factor=max_lr / lr0, final_div_factor=100, anneal_strategy="linear", three_phase=True,
    pct_start=0.4) with its default cycle_momentum=True, so the momentum runs 0.95 -> 0.85 -> 0.95 -> 0.95 whatever
    hyper_params["momentum"] says.  step == total_steps is what the scheduler holds after the last iteration."""
    step, total = int(step), int(total_steps)
    if total < 1 or not 0 <= step <= total:
        raise ValueError(f"one_cycle: step {step} outside [0, {total}] (total_steps must be >= 1)")
    initial = float(max_lr) / (float(max_lr) / float(lr0))
    lowest = initial / FINAL_DIV
    phases = ((float(PCT_START * total) - 1, initial, float(max_lr), MAX_MOMENTUM, BASE_MOMENTUM),
              (float(2 * PCT_START * total) - 2, float(max_lr), initial, BASE_MOMENTUM, MAX_MOMENTUM),
              (total - 1, initial, lowest, MAX_MOMENTUM, MAX_MOMENTUM))
    start = 0.0
    for i, (end, lr_a, lr_b, m_a, m_b) in enumerate(phases):
        if step <= end or i == len(phases) - 1:
            pct = (step - start) / (end - start)
            return (lr_b - lr_a) * pct + lr_a, (m_b - m_a) * pct + m_a
        start = end


def check_batch(network, hyper_params: Dict, batch) -> int:
    """What a Trainer cannot train on, refused before any device call.  Returns the rows n."""
    if len(batch) != 7:
        raise ValueError("a batch is the 7-tuple of ReplayBuffer.sample: states, policies, values, rewards, valid_actions_msk, indices, weights")
    states, pol, val, rew, msk, index, weights = batch
    if states is None:
        raise ValueError("the batch has no states (a ring built with planes=False)")
    A, c_in = int(network.num_actions), int(hyper_params["input_channels"])
    if states.dim() != 4 or states.shape[1] != c_in:
        raise ValueError(f"states: [n, {c_in}, side, side], got {tuple(states.shape)}")
    n = int(states.shape[0])
    if n < 1:
        raise ValueError("an empty batch")
    if tuple(pol.shape) != (n, A) or tuple(msk.shape) != (n, A):
        raise ValueError(f"policies / valid_actions_msk: [{n}, {A}] for this network, got {tuple(pol.shape)} / {tuple(msk.shape)}")
    for name, t in (("values", val), ("rewards", rew), ("indices", index), ("weights", weights)):
        if int(t.numel()) != n:
            raise ValueError(f"{name}: {n} entries expected, got {tuple(t.shape)}")
    # A prioritised draw with no mass left has index -1 and NaN rows (PrioritizedReplay.sample).  Indices in host memory are checked
    # here; indices in device memory are not read (an iteration reads nothing from the device): such a draw needs every sampled row
    # re-opened by self-play running on during training, which train() does not do, and its NaN would show in the epoch's means.
    if not index.is_cuda and bool((index < 0).any()):
        raise ValueError("a prioritised batch with index -1 (no row had mass)")
    return n


# ---------------------------------------------------------------------------------------------------- the trainer
class Trainer:
    def __init__(self, network, hyper_params: Dict, fused: bool = True):
        """network: a PolicyValueNetwork (networks.py), on the device it trains on.  hyper_params: the reference's dictionary
        (config/example.yaml: learning_rate, max_learning_rate, weight_decay, momentum, max_grad_norm, policy / value / reward /
        reconstruction_loss_coeff, entropy_regularization_coeff, use_reward_target, use_autoencoder, num_epochs, batch_size,
        num_augmented_samples, use_per, replay_alpha, replay_beta0).  fused=False: the reference's stock-torch loss and torch.optim.SGD."""
        import torch

        self.torch = torch
        hp = self.hp = dict(hyper_params)
        if not hp.get("mask_policy_head", True) or not network.hyper_params.get("mask_policy_head", True):
            raise ValueError("mask_policy_head=False is not supported: the loss shifts the invalid logits (and the search reads the "
                             "policy on the valid set only)")
        self.network, self.fused = network, bool(fused)
        self.device = next(network.parameters()).device
        if self.fused and self.device.type != "cuda":
            raise ValueError("fused=True trains on the GPU: move the network there, or pass fused=False")
        self.use_reward, self.use_ae = bool(hp.get("use_reward_target", False)), bool(hp.get("use_autoencoder", False))
        if self.use_reward != bool(network.hyper_params.get("use_reward_target", False)) or \
                self.use_ae != bool(network.hyper_params.get("use_autoencoder", False)):
            raise ValueError("use_reward_target / use_autoencoder differ between the network and the trainer's hyper_params")
        self.coeffs = (float(hp["policy_loss_coeff"]), float(hp["value_loss_coeff"]),
                       float(hp.get("reward_loss_coeff", 0.0)) if self.use_reward else 0.0, float(hp["entropy_regularization_coeff"]))
        self.recon_coeff = float(hp.get("reconstruction_loss_coeff", 0.0))
        self.lr0, self.max_lr = float(hp["learning_rate"]), float(hp["max_learning_rate"])
        self.weight_decay, self.max_norm = float(hp["weight_decay"]), float(hp["max_grad_norm"])
        self.total_steps: Optional[int] = None  # the schedule's length: train() sets it, or set_schedule()
        self.iteration = 0                      # optimizer steps under the current schedule
        self.total_iterations = 0
        self._iter_mark = 0                     # total_iterations at the last reset of the accumulators
        self.acc = torch.zeros((8,), dtype=torch.float64, device=self.device)  # sums of the 6 stats, the grad norm, the rows
        self.last_value_losses = None  # [n] f64 on the device: what the priorities are updated with
        self.last_norm = None
        self.per = None  # the PrioritizedReplay of the last train() with use_per
        # fused state, built after the first backward (only then is it known which parameters receive a gradient: the reference's
        # optimizer never touches the others, e.g. the decoder without use_autoencoder)
        self.flat = self.gflat = self.mbuf = None
        self._views = None
        self._optimizer = None
        if self.fused:
            from ... import _ffi

            self._ffi, self._lib = _ffi, _ffi.load()
            self._scratch = torch.empty((_ffi.IPP_PVNET_SGD_SCRATCH,), dtype=torch.float64, device=self.device)
            self._norm = torch.zeros((1,), dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ schedule
    def set_schedule(self, total_steps: int):
        """A new one-cycle schedule of total_steps optimizer steps (train() calls it: num_epochs x num_batches); the momentum buffer
        starts from zero, as the reference builds a new optimizer per train() call (:51-56)."""
        if int(total_steps) < 1:
            raise ValueError("total_steps < 1")
        self.total_steps, self.iteration = int(total_steps), 0
        if self.mbuf is not None:
            self.mbuf.zero_()
        if not self.fused:
            torch = self.torch
            self._optimizer = torch.optim.SGD(self.network.parameters(), lr=self.lr0, weight_decay=self.weight_decay,
                                              momentum=float(self.hp.get("momentum", 0.9)))
            self._scheduler = torch.optim.lr_scheduler.OneCycleLR(
                self._optimizer, max_lr=self.max_lr, total_steps=self.total_steps, div_factor=self.max_lr / self.lr0,
                final_div_factor=FINAL_DIV, anneal_strategy="linear", three_phase=True, pct_start=PCT_START)

    # ------------------------------------------------------------------ flat buffers
    def _flatten(self):
        """After the first backward: the parameters that received a gradient become views of one flat buffer, their .grad views of a
        second one (holding the gradients just computed), the momentum buffer a third."""
        torch = self.torch
        used = [p for p in self.network.parameters() if p.grad is not None]
        if not used:
            raise RuntimeError("no parameter received a gradient")
        if any(p.dtype != torch.float32 for p in used):
            raise ValueError("the fused trainer trains float32 parameters")
        total = sum(p.numel() for p in used)
        self.flat = torch.empty((total,), dtype=torch.float32, device=self.device)
        self.gflat = torch.empty((total,), dtype=torch.float32, device=self.device)
        self.mbuf = torch.zeros((total,), dtype=torch.float32, device=self.device)
        self._views, o = [], 0
        for p in used:
            k = p.numel()
            w, g = self.flat[o:o + k].view(p.shape), self.gflat[o:o + k].view(p.shape)
            w.copy_(p.data)
            g.copy_(p.grad)
            p.data, p.grad = w, g
            self._views.append((p, w.data_ptr(), g.data_ptr()))
            o += k

    def _check_views(self):
        """autograd accumulates in place into the preset .grad views; were it ever to replace one, the update would read a stale buffer."""
        for p, wp, gp in self._views:
            if p.grad is None or p.grad.data_ptr() != gp or p.data_ptr() != wp:
                raise RuntimeError("a parameter or its gradient left the trainer's flat buffers (replaced, not updated in place): "
                                   "refusing to train on stale buffers")

    # ------------------------------------------------------------------ one iteration
    def step(self, batch):
        """One training iteration on the 7-tuple of ReplayBuffer.sample / PrioritizedReplay.sample (device tensors).  Returns nothing:
        the losses go into device accumulators (epoch_means), the per-row value losses into last_value_losses."""
        torch, hp = self.torch, self.hp
        n = check_batch(self.network, hp, batch)
        if self.total_steps is None:
            raise ValueError("no schedule: call set_schedule(total_steps) first (train() does)")
        if self.iteration >= self.total_steps:
            raise ValueError(f"the schedule's {self.total_steps} steps are used up")
        states, pol, val, rew, msk, index, weights = batch
        dev = self.device
        states = states.to(device=dev, dtype=torch.float32)
        self.network.train()
        if not self.fused:
            return self._step_stock(n, states, pol, val, rew, msk, weights)
        pol = pol.to(device=dev, dtype=torch.float32).contiguous()
        msk = msk.to(device=dev, dtype=torch.uint8).contiguous()
        val = val.to(device=dev, dtype=torch.float64).contiguous()
        rew = rew.to(device=dev, dtype=torch.float64).contiguous()
        weights = weights.to(device=dev, dtype=torch.float64).contiguous()
        logits, value, reward, recon = self.network.forward_logits(states)
        A = int(logits.shape[1])
        lg, vv = logits.detach().contiguous(), value.detach().reshape(-1).contiguous()
        rr = reward.detach().reshape(-1).contiguous() if self.use_reward else None
        stats = torch.empty((n, 6), dtype=torch.float64, device=dev)
        g_logits, g_value = torch.empty_like(lg), torch.empty_like(vv)
        g_reward = torch.empty_like(rr) if rr is not None else None
        pc, vc, rc, ec = self.coeffs
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self._ffi.check(self._lib.ipp_pvnet_loss(
            lg.data_ptr(), pol.data_ptr(), msk.data_ptr(), vv.data_ptr(), rr.data_ptr() if rr is not None else None, val.data_ptr(),
            rew.data_ptr() if rr is not None else None, weights.data_ptr(), n, A, pc, vc, rc, ec, stats.data_ptr(), g_logits.data_ptr(),
            g_value.data_ptr(), g_reward.data_ptr() if rr is not None else None, dev.index or 0, stream))
        outs, grads = [logits, value], [g_logits.view_as(logits), g_value.view_as(value)]
        if self.use_reward:
            outs.append(reward)
            grads.append(g_reward.view_as(reward))
        if self.use_ae:  # (:142-147: enters the total as (rc recon_i w_i).mean())
            recon_rows = reconstruction_loss(torch, states[:, 0], recon)
            outs.append((self.recon_coeff * recon_rows * weights.to(recon_rows.dtype)).mean())
            grads.append(None)
        if self.gflat is not None:
            self.gflat.zero_()
        else:  # (the first backward shows which parameters are trained: gradients left by an earlier owner must not count)
            for p in self.network.parameters():
                p.grad = None
        torch.autograd.backward(outs, grads)
        if self.gflat is None:
            self._flatten()
        self._check_views()
        lr, mu = one_cycle(self.iteration, self.total_steps, self.lr0, self.max_lr)
        self._ffi.check(self._lib.ipp_pvnet_sgd_step(self.flat.data_ptr(), self.gflat.data_ptr(), self.mbuf.data_ptr(), int(self.flat.numel()),
                                                     lr, mu, self.weight_decay, self.max_norm, self._norm.data_ptr(), self._scratch.data_ptr(),
                                                     C.c_uint64(self._scratch.numel()), dev.index or 0, stream))
        self.acc[:6] += stats.sum(0)
        self.acc[6:7] += self._norm
        self.acc[7] += n
        self.last_value_losses, self.last_norm = stats[:, 1], self._norm
        self.iteration += 1
        self.total_iterations += 1

    def _step_stock(self, n, states, pol, val, rew, msk, weights):
        """The reference's own expressions (:98-173) on whatever device the network is on."""
        torch, dev = self.torch, self.device
        pol, msk = pol.to(device=dev, dtype=torch.float32), msk.to(device=dev, dtype=torch.float32)
        tv, tr = val.to(device=dev, dtype=torch.float32), rew.to(device=dev, dtype=torch.float32)
        w = weights.to(device=dev, dtype=torch.float32)
        pc, vc, rc, ec = self.coeffs
        log_p, value, reward, recon = self.network(states, msk)
        pl = -torch.sum(pol * log_p * msk, dim=1)
        vl = torch.square(value.view(-1) - tv)
        total = pc * pl + vc * vl
        H = -torch.sum(torch.exp(log_p) * log_p, dim=1)
        total = total - ec * H
        rl = torch.zeros_like(vl)
        if self.use_reward:
            rl = torch.square(reward.view(-1) - tr)
            total = total + rc * rl
        if self.use_ae:
            total = total + self.recon_coeff * reconstruction_loss(torch, states[:, 0], recon)
        total = total * w
        loss = total.mean()
        self._optimizer.zero_grad()
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(self.network.parameters(), max_norm=self.max_norm, norm_type=2)
        self._optimizer.step()
        self._scheduler.step()
        with torch.no_grad():
            rel = torch.abs(tv - value.view(-1)) / torch.abs(tv)
            stats = torch.stack([pl, vl, rl, H, total, rel], dim=1).detach().double()
            self.acc[:6] += stats.sum(0)
            self.acc[6] += norm.detach().double()
            self.acc[7] += n
        self.last_value_losses, self.last_norm = stats[:, 1], norm.detach()
        self.iteration += 1
        self.total_iterations += 1

    # ------------------------------------------------------------------ the reference's train()
    def epoch_means(self, reset: bool = True) -> Dict[str, float]:
        """Means of the accumulators since the last reset: the per-row losses over the rows, the grad norm over the iterations.  ONE
        read of the device."""
        a = self.acc.cpu().numpy()
        rows = max(a[7], 1.0)
        out = {k: float(a[i] / rows) for i, k in enumerate(STAT_NAMES)}
        out["grad_norm"] = float(a[6] / max(self.total_iterations - self._iter_mark, 1))
        if reset:
            self.acc.zero_()
            self._iter_mark = self.total_iterations
        return out

    def train(self, replay):
        """PolicyValueNetworkWrapper.train on a ring (SelfPlay.replay): use_per selects replay.prioritized(batch_size, replay_alpha,
        replay_beta0, num_epochs), else replay.sample(batch_size, num_augmented_samples); num_batches = len(buffer) // sample_size (the
        one device read before the loop, as the reference reads its file list); after each optimizer step per.step(), then
        per.update(indices, value_loss + 1e-8).  Returns the per-epoch means of the losses and the grad norm (one read per epoch)."""
        hp = self.hp
        epochs, batch = int(hp["num_epochs"]), int(hp["batch_size"])
        per = None
        if hp.get("use_per", False):
            per = replay.prioritized(batch, float(hp["replay_alpha"]), float(hp["replay_beta0"]), epochs)
            size, sample_size = len(per), per.sample_size
        else:
            k = int(hp.get("num_augmented_samples", 0))
            size, sample_size = len(replay), max(1, batch // (k + 1))
        num_batches = size // sample_size
        if num_batches < 1:
            raise ValueError(f"{size} committed samples give no batch of {sample_size}")
        self.per = per
        self.set_schedule(epochs * num_batches)
        self.epoch_means()  # (start from empty accumulators)
        history = []
        for _ in range(epochs):
            for _ in range(num_batches):
                if per is not None:
                    b = per.sample()
                    self.step(b)
                    per.step()
                    per.update(b[5], self.last_value_losses + 1e-8)
                else:
                    self.step(replay.sample(batch, k, check_empty=False))
            history.append(self.epoch_means())
        return history

    def hand_over(self, device_net):
        """The new weights to the search (`self.network.load_state_dict`, :249): DevicePolicyValueNet re-folds and uploads them."""
        device_net.load_state_dict(self.network.state_dict())


def reconstruction_loss(torch, first_planes, recon):
    """PolicyValueNetworkWrapper.reconstruction_loss (:267-272): the mean squared error per row over the first plane."""
    n = first_planes.shape[0]
    a, b = first_planes.reshape(n, -1), recon.reshape(n, -1)
    return torch.sum((a - b).pow(2), dim=1) / a.shape[1]
