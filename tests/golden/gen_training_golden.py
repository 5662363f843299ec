#!/usr/bin/env python
"""
Generate tests/golden/training.npz by IMPORTING the reference's PolicyValueNetworkWrapper (planning/mcts_zero/network_wrappers/
policy_value_network_wrappers.py) and recording what its training code computes on the cases of tests/training_cases.py.

    python tests/golden/gen_training_golden.py REFERENCE_CHECKOUT          (or IPP_REFERENCE=REFERENCE_CHECKOUT)

The fixture holds numbers only:
    loss{k}_{32|64}_{stats,glogits,gvalue,greward}   per loss shape k of GOLDEN_LOSS_SHAPES, with reward and entropy coefficient 0.2: the
                         wrapper's four static loss methods (policy_loss, entropy_regularization, scalar_loss, relative_scalar_loss)
                         on log_softmax(logits - (1 - mask) 1000), combined as train() combines them (:120-154), per row
                         [pl, vl, rl, H, total, rel], and autograd's gradients of the batch mean; in float32 and in float64
    sched_{a,b}          (lr, momentum) the optimizer holds at each of its steps under train()'s OneCycleLR call for 3 epochs x 4
                         batches and 3 x 50 (learning_rate 0.0005, max_learning_rate 0.005), one row more: the state after the last step
    sgd_params, sgd_buf, sgd_norm   three steps of clip_grad_norm_ + torch.optim.SGD.step on the 300-element vectors of sgd_case(300, 3.0),
                         on float32 tensors; sgd64_*: the same code on float64 tensors, the state stored as float32 between the steps
    e2e_{uni|per}_*      one train() of the reference on the CPU: pvnet case "b" with the redrawn weights (CRC-checked), the 24 dummy
                         samples of e2e_samples(), batch 8, 2 epochs: the sample ids of every minibatch, for PER the buffer indices, the
                         weights and the order of the file list, the (lr, momentum) of every optimizer step, the per-row value losses,
                         the order of the buffer's step / update calls, the final state_dict as one float32 vector, and
                         e2e_*_spread = the largest difference of that vector between one thread and the default thread count
torch.utils.tensorboard and torchvision are stubbed when absent; the train-data directory is a temporary directory.
"""
import bz2
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np

os.environ.setdefault("TQDM_DISABLE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pvnet_cases as pc  # noqa: E402
from tests import training_cases as tc  # noqa: E402


class _Writer:
    def add_scalar(self, *a, **k):
        pass

    add_histogram = add_scalar


def _stub_modules():
    try:
        import torchvision  # noqa: F401
    except ImportError:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    try:
        import torch.utils.tensorboard  # noqa: F401
    except ImportError:
        m = types.ModuleType("torch.utils.tensorboard")
        m.SummaryWriter = _Writer
        sys.modules["torch.utils.tensorboard"] = m


def record_losses(W, out):
    import torch

    for k, (n, A) in enumerate(tc.GOLDEN_LOSS_SHAPES):
        c = tc.loss_case(n, A)
        pcf, vcf, rcf, ecf = tc.COEFFS["policy"], tc.COEFFS["value"], tc.COEFFS["reward"], tc.ENTROPY_COEFFS[1]
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            z = torch.tensor(c["logits"], dtype=dt, requires_grad=True)
            v = torch.tensor(c["value"], dtype=dt).reshape(n, 1).requires_grad_(True)
            r = torch.tensor(c["reward"], dtype=dt).reshape(n, 1).requires_grad_(True)
            t, m = torch.tensor(c["target_policy"], dtype=dt), torch.tensor(c["valid_msk"], dtype=dt)
            tv, tr = torch.FloatTensor(c["target_value"]).to(dt), torch.FloatTensor(c["target_reward"]).to(dt)
            w = torch.FloatTensor(c["weights"]).to(dt) if bits == 32 else torch.tensor(c["weights"], dtype=dt)
            log_p = torch.log_softmax(z - (1 - m) * 1000, dim=1)
            pl, H = W.policy_loss(t, log_p, m), W.entropy_regularization(log_p)
            vl, rl = W.scalar_loss(tv, v), W.scalar_loss(tr, r)
            total = (pcf * pl + vcf * vl - ecf * H + rcf * rl) * w
            total.mean().backward()
            rel = torch.abs(tv - v.view(-1)) / torch.abs(tv)  # (relative_scalar_loss before its mean)
            assert torch.allclose(rel.mean(), W.relative_scalar_loss(tv, v), rtol=1e-5)
            out[f"loss{k}_{bits}_stats"] = torch.stack([pl, vl, rl, H, total, rel], dim=1).detach().double().numpy()
            out[f"loss{k}_{bits}_glogits"] = z.grad.double().numpy()
            out[f"loss{k}_{bits}_gvalue"] = v.grad.double().numpy().reshape(n)
            out[f"loss{k}_{bits}_greward"] = r.grad.double().numpy().reshape(n)


def record_schedule(out):
    import torch

    for tag, (epochs, batches) in (("a", (3, 4)), ("b", (3, 50))):
        lr0, max_lr = 0.0005, 0.005
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr0, weight_decay=3e-5, momentum=0.9)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, epochs=epochs, steps_per_epoch=batches, div_factor=max_lr / lr0,
                                                  final_div_factor=100, anneal_strategy="linear", three_phase=True, pct_start=0.40)
        rows = []
        for _ in range(epochs * batches):
            rows.append((opt.param_groups[0]["lr"], opt.param_groups[0]["momentum"]))
            opt.step()
            sch.step()
        rows.append((opt.param_groups[0]["lr"], opt.param_groups[0]["momentum"]))
        out[f"sched_{tag}"] = np.array(rows, dtype=np.float64)
        out[f"sched_{tag}_meta"] = np.array([epochs, batches, lr0, max_lr], dtype=np.float64)


def record_sgd(out):
    """clip_grad_norm_ + torch.optim.SGD.step, torch's own code, twice: on float32 tensors as the reference runs it (sgd_*), and on
    float64 tensors with the state stored as float32 between the steps (sgd64_*: every step starts from the float32 values of the step
    before, computes in float64 and is rounded once when stored -- the arithmetic of ipp_pvnet_sgd_step)."""
    import torch

    p0, grads = tc.sgd_case(300, 3.0)
    lr, mu, wd, max_norm = 0.05, 0.9, 3e-5, 1.0
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([p], lr=lr, weight_decay=wd, momentum=mu)
    ps, bufs, norms = [], [], []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm=max_norm, norm_type=2)))
        opt.step()
        ps.append(p.detach().numpy().copy())
        bufs.append(opt.state[p]["momentum_buffer"].numpy().copy())
    out["sgd_params"], out["sgd_buf"], out["sgd_norm"] = np.array(ps), np.array(bufs), np.array(norms)
    out["sgd_meta"] = np.array([lr, mu, wd, max_norm], dtype=np.float64)

    p32, b32 = p0.copy(), None
    ps, bufs, norms = [], [], []
    for g in grads:
        q = torch.nn.Parameter(torch.from_numpy(p32.astype(np.float64)))
        opt = torch.optim.SGD([q], lr=lr, weight_decay=wd, momentum=mu)
        if b32 is not None:
            opt.state[q]["momentum_buffer"] = torch.from_numpy(b32.astype(np.float64))
        q.grad = torch.from_numpy(g.astype(np.float64))
        norms.append(float(torch.nn.utils.clip_grad_norm_([q], max_norm=max_norm, norm_type=2)))
        opt.step()
        p32, b32 = q.detach().numpy().astype(np.float32), opt.state[q]["momentum_buffer"].numpy().astype(np.float32)
        ps.append(p32.copy())
        bufs.append(b32.copy())
    out["sgd64_params"], out["sgd64_buf"], out["sgd64_norm"] = np.array(ps), np.array(bufs), np.array(norms)


def run_e2e(pvw, rb, use_per, tmp, threads):
    """One reference train(); returns the records."""
    import torch

    if threads:
        torch.set_num_threads(threads)
    hp, md = tc.e2e_params(use_per)
    random.seed(tc.E2E_SEED)
    np.random.seed(tc.E2E_SEED + int(use_per))
    torch.manual_seed(tc.E2E_SEED)
    rec = dict(ids=[], index=[], weights=[], order=None, lr_mom=[], value_losses=[], calls=[])

    def sample_id(path):
        return int(os.path.basename(path).split("_")[1].split(".")[0])

    base = rb.PrioritizedExperienceReplayBuffer if use_per else rb.ExperienceReplayBuffer

    class Recording(base):
        def sample(self):
            if rec["order"] is None:
                rec["order"] = [sample_id(p) for p in self.data_file_paths]
            o = super().sample()
            rec["index"].append(np.asarray(o[5], dtype=np.int64))
            rec["ids"].append(np.array([rec["order"][i] for i in o[5]], dtype=np.int64))
            rec["weights"].append(np.asarray(o[6], dtype=np.float64))
            return o

        def step(self):
            rec["calls"].append(0)
            return super().step()

        def update(self, indices, priorities):
            rec["calls"].append(1)
            assert np.array_equal(np.asarray(indices), rec["index"][-1])
            rec["value_losses"].append(np.asarray(priorities, dtype=np.float64) - 1e-8)
            return super().update(indices, priorities)

    sgd_step = torch.optim.SGD.step

    def recording_step(self, *a, **k):
        rec["lr_mom"].append((self.param_groups[0]["lr"], self.param_groups[0]["momentum"]))
        return sgd_step(self, *a, **k)

    saved = (pvw.ExperienceReplayBuffer, pvw.PrioritizedExperienceReplayBuffer)
    if use_per:
        pvw.PrioritizedExperienceReplayBuffer = Recording
    else:
        pvw.ExperienceReplayBuffer = Recording
    torch.optim.SGD.step = recording_step
    try:
        wrapper = pvw.PolicyValueNetworkWrapper(hp, md)
        assert wrapper.device.type == "cpu"
        ref_sd = wrapper.network.state_dict()
        keys, shapes = list(ref_sd.keys()), [list(v.shape) for v in ref_sd.values()]
        sd = pc.draw_state_dict(keys, shapes, pc.CONFIGS[tc.E2E_CASE]["seed"])
        fx = pc.fixture()
        assert [pc.crc(sd[k]) for k in keys] == [int(v) for v in fx[f"{tc.E2E_CASE}_crc"]], "not the weights of tests/golden/pvnet.npz"
        wrapper.network.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        wrapper.set_summary_writer(_Writer())
        wrapper.train(0, 1)
        final = np.concatenate([v.detach().double().numpy().reshape(-1) for v in wrapper.network.state_dict().values()])
    finally:
        pvw.ExperienceReplayBuffer, pvw.PrioritizedExperienceReplayBuffer = saved
        torch.optim.SGD.step = sgd_step
    rec["final"] = final
    return rec


def record_e2e(pvw, rb, out):
    import torch

    default_threads = torch.get_num_threads()
    with tempfile.TemporaryDirectory() as tmp:
        rb.TRAIN_DATA_DIR = tmp
        os.makedirs(os.path.join(tmp, "iter_0"))
        for i, s in enumerate(tc.e2e_samples()):
            with bz2.BZ2File(os.path.join(tmp, "iter_0", f"sample_{i:04d}.pkl.bz2"), "wb") as f:
                pickle.dump(s, f)
        for tag, use_per in (("uni", False), ("per", True)):
            one = run_e2e(pvw, rb, use_per, tmp, 1)
            many = run_e2e(pvw, rb, use_per, tmp, default_threads)
            for k in ("ids", "index", "lr_mom", "calls"):
                assert np.array_equal(np.array(one[k]), np.array(many[k])), k
            # (PER weights follow the priorities = the value losses, which carry the threads' rounding)
            assert np.allclose(np.array(one["weights"]), np.array(many["weights"]), rtol=1e-4, atol=0)
            steps = len(one["ids"])
            assert steps == (tc.E2E_SAMPLES // tc.E2E_TRAIN["batch_size"]) * tc.E2E_TRAIN["num_epochs"] == len(one["lr_mom"])
            out[f"e2e_{tag}_ids"] = np.array(one["ids"])
            out[f"e2e_{tag}_index"] = np.array(one["index"])
            out[f"e2e_{tag}_weights"] = np.array(one["weights"])
            out[f"e2e_{tag}_order"] = np.array(one["order"], dtype=np.int64)
            out[f"e2e_{tag}_lr_mom"] = np.array(one["lr_mom"], dtype=np.float64)
            out[f"e2e_{tag}_value_losses"] = np.array(one["value_losses"])
            out[f"e2e_{tag}_calls"] = np.array(one["calls"], dtype=np.int64)
            out[f"e2e_{tag}_final"] = one["final"].astype(np.float32)
            assert np.array_equal(out[f"e2e_{tag}_final"].astype(np.float64), one["final"])  # (float32 values: nothing lost)
            out[f"e2e_{tag}_spread"] = np.float64(np.max(np.abs(one["final"] - many["final"])))
            print(f"e2e {tag}: {steps} steps, {one['final'].size} floats, spread {out[f'e2e_{tag}_spread']:.3e} "
                  f"({default_threads} threads against 1)")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IPP_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("usage: gen_training_golden.py REFERENCE_CHECKOUT (the fixture can only be generated next to the reference)")
    sys.path.insert(1, ref)
    _stub_modules()
    from planning.mcts_zero import replay_buffers as rb
    from planning.mcts_zero.network_wrappers import policy_value_network_wrappers as pvw

    out = {}
    record_losses(pvw.PolicyValueNetworkWrapper, out)
    record_schedule(out)
    record_sgd(out)
    record_e2e(pvw, rb, out)
    path = os.path.join(ROOT, "tests", "golden", "training.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
