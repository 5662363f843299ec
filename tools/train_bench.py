#!/usr/bin/env python
"""
Step time of Trainer (ipp_rl_amd/planning/mcts_zero/training.py) with fused=True against fused=False (the reference's stock-torch loss and
torch.optim.SGD), with device events on the stream, and the two fused parts taken alone against their stock counterparts:

    network   config/example.yaml's network: 16 input channels on the 10 x 10 grid's 100 x 100 planes, 128 channels, 10 encoder blocks,
              A = 200 actions, batch 96
    loss      ipp_pvnet_loss against the stock expressions (log_softmax, the four loss methods, autograd's backward to the logits) on
              [96, 200] and on [96, A_max], A_max = 50 x 50 cells x 8 altitude levels = 20 000 actions
    update    ipp_pvnet_sgd_step against clip_grad_norm_ + torch.optim.SGD.step on the network's parameters

    python tools/train_bench.py [--rounds 5] [--iters 20] [--out profiles/train_bench.txt]

Every shape is warmed up first; each figure is the median over the rounds of the mean over `iters` back-to-back iterations.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ipp_rl_amd import _ffi  # noqa: E402
from ipp_rl_amd.planning.mcts_zero import PolicyValueNetwork, Trainer  # noqa: E402

HP = dict(input_channels=16, num_channels=128, dropout=0.0, use_silu=True, num_encoder_res_blocks=10, use_separable_conv_layers=True,
          use_global_context_mixing=True, num_global_pooling_channels=32, num_policy_head_conv_bn_blocks=3, num_value_head_conv_bn_blocks=3,
          mask_policy_head=True, use_reward_target=False, use_autoencoder=False, learning_rate=0.0005, max_learning_rate=0.005,
          weight_decay=0.00003, momentum=0.9, max_grad_norm=10.0, policy_loss_coeff=1.0, value_loss_coeff=1.0, reward_loss_coeff=1.0,
          reconstruction_loss_coeff=1.0, entropy_regularization_coeff=0.0, num_epochs=3, batch_size=96, num_augmented_samples=0,
          use_per=False, replay_alpha=0.75, replay_beta0=0.4)
MD = dict(num_grid_cells=100, min_altitude=8.0, max_altitude=14.0, altitude_spacing=6.0)
BATCH, SIDE, A_MAX = 96, 100, 20000


def timed(fn, rounds, iters):
    """Median over the rounds of the mean milliseconds of `iters` back-to-back calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def batch(n, A, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    msk = (torch.rand((n, A), generator=g) < 0.3)
    msk[:, 0] = True
    pol = torch.rand((n, A), generator=g) * msk
    pol = pol / pol.sum(1, keepdim=True)
    return (torch.rand((n, HP["input_channels"], SIDE, SIDE), generator=g).to(dev), pol.to(dev), torch.rand((n,), generator=g).double().to(dev) + 0.2,
            torch.rand((n,), generator=g).double().to(dev), msk.to(torch.uint8).to(dev), torch.arange(n, device=dev),
            torch.ones((n,), dtype=torch.float64, device=dev))


def loss_parts(A, dev, rounds, iters):
    lib = _ffi.load()
    g = torch.Generator(device="cpu").manual_seed(A)
    _, pol, val, _, msk, _, w = batch(BATCH, A, dev, seed=A)
    logits = torch.randn((BATCH, A), generator=g).to(dev).requires_grad_(True)
    value = (torch.rand((BATCH, 1), generator=g) + 0.1).to(dev).requires_grad_(True)
    stats = torch.empty((BATCH, 6), dtype=torch.float64, device=dev)
    gl, gv = torch.empty((BATCH, A), dtype=torch.float32, device=dev), torch.empty((BATCH,), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lg, vv = logits.detach(), value.detach().reshape(-1)

    def fused():
        _ffi.check(lib.ipp_pvnet_loss(lg.data_ptr(), pol.data_ptr(), msk.data_ptr(), vv.data_ptr(), None, val.data_ptr(), None, w.data_ptr(),
                                      BATCH, A, 1.0, 1.0, 0.0, 0.01, stats.data_ptr(), gl.data_ptr(), gv.data_ptr(), None, dev.index or 0, stream))
        return stats.sum(0)

    mf, tv, wf = msk.float(), val.float(), w.float()

    def stock():
        log_p = torch.log_softmax(logits - (1 - mf) * 1000, dim=1)
        pl = -torch.sum(pol * log_p * mf, dim=1)
        vl = torch.square(value.view(-1) - tv)
        H = -torch.sum(torch.exp(log_p) * log_p, dim=1)
        total = ((1.0 * pl + 1.0 * vl) - 0.01 * H) * wf
        logits.grad = value.grad = None
        total.mean().backward()
        return torch.stack([pl.mean(), vl.mean(), H.mean()])

    return timed(fused, rounds, iters), timed(stock, rounds, iters)


def update_parts(net, dev, rounds, iters):
    lib = _ffi.load()
    params = [p for p in net.parameters()]
    n = sum(p.numel() for p in params)
    flat, gflat = torch.randn((n,), device=dev) * 0.1, torch.randn((n,), device=dev) * 0.01
    buf = torch.zeros((n,), device=dev)
    norm = torch.zeros((1,), dtype=torch.float64, device=dev)
    scratch = torch.empty((_ffi.IPP_PVNET_SGD_SCRATCH,), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fused():
        _ffi.check(lib.ipp_pvnet_sgd_step(flat.data_ptr(), gflat.data_ptr(), buf.data_ptr(), n, 0.001, 0.9, 3e-5, 10.0, norm.data_ptr(),
                                          scratch.data_ptr(), C.c_uint64(scratch.numel()), dev.index or 0, stream))

    opt = torch.optim.SGD(params, lr=0.001, weight_decay=3e-5, momentum=0.9)
    for p in params:
        p.grad = torch.randn_like(p) * 0.01

    def stock():
        torch.nn.utils.clip_grad_norm_(params, max_norm=10.0, norm_type=2)
        opt.step()

    return n, len(params), timed(fused, rounds, iters), timed(stock, rounds, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"train_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; batch {BATCH}, planes {HP['input_channels']} x {SIDE} x {SIDE}, "
             f"{HP['num_channels']} channels, A = 200; ms = median (min .. max) over {args.rounds} rounds of the mean of {args.iters} iterations"]
    fmt = lambda t: f"{t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"  # noqa: E731
    b = batch(BATCH, 200, dev)
    for fused in (True, False):
        torch.manual_seed(0)
        net = PolicyValueNetwork(HP, MD).to(dev)
        tr = Trainer(net, HP, fused=fused)
        tr.set_schedule(10 ** 6)
        lines.append(f"step   {'fused' if fused else 'stock'}  {fmt(timed(lambda: tr.step(b), args.rounds, args.iters))}")
    for A in (200, A_MAX):
        f, s = loss_parts(A, dev, args.rounds, args.iters)
        lines.append(f"loss   [96, {A:5d}]  fused {fmt(f)}   stock {fmt(s)}   stock / fused {s[0] / f[0]:.2f}")
    torch.manual_seed(0)
    n, tensors, f, s = update_parts(PolicyValueNetwork(HP, MD).to(dev), dev, args.rounds, args.iters)
    lines.append(f"update {n} parameters in {tensors} tensors  fused {fmt(f)}   stock {fmt(s)}   stock / fused {s[0] / f[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
