"""
CPU tests of the training station (ipp_rl_amd/planning/mcts_zero/training.py) against tests/golden/training.npz, which
tests/golden/gen_training_golden.py records from the reference's PolicyValueNetworkWrapper:
  * pv_losses_host reproduces the reference's static loss methods and autograd's gradients in float64: the six per-row figures at 1e-12
    relative, the gradients at 1e-12 of the row's largest gradient (an entry is a difference T p_j - t_j m_j of terms up to that size,
    so its own rounding is relative to them, not to itself); the float32 records within the float32 rounding of the same scale;
  * one_cycle reproduces (lr, momentum) of the reference's OneCycleLR call, momentum cycling included, at 1e-15 relative;
  * sgd_clip_step_host reproduces three steps of clip_grad_norm_ + torch.optim.SGD within 1 float32 ulp, against torch's own code run
    in float64 with float32 storage (the arithmetic the kernel is specified to have); against torch in float32 within what its extra
    roundings allow (derived in the test), a first step within 1 ulp;
  * the header declares ipp_pvnet_loss / ipp_pvnet_sgd_step and _ffi binds them;
  * Trainer(fused=False) on the CPU, fed the recorded minibatches, reproduces the reference's final parameters within
    8 x max(ref_spread, 2^-24 max|p|) (ref_spread: the reference at one thread against its default thread count), uniform and PER,
    calls the buffer's step() before its update(), hands value_loss + 1e-8 to update(), and runs the recorded (lr, momentum);
  * mask_policy_head=False, a batch of another shape and a PER batch with index -1 raise ValueError.
"""
import os
import re

import numpy as np
import pytest
import torch

from ipp_rl_amd import _ffi
from ipp_rl_amd.planning.mcts_zero import PolicyValueNetwork, Trainer, one_cycle, pv_losses_host, sgd_clip_step_host
from tests import pvnet_cases as pc
from tests import training_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _losses(c, ec, with_reward=True):
    return pv_losses_host(c["logits"], c["target_policy"], c["valid_msk"], c["value"], c["reward"] if with_reward else None, c["target_value"],
                          c["target_reward"] if with_reward else None, c["weights"], tc.COEFFS["policy"], tc.COEFFS["value"],
                          tc.COEFFS["reward"] if with_reward else 0.0, ec)


@pytest.mark.parametrize("k", range(len(tc.GOLDEN_LOSS_SHAPES)))
def test_losses_and_gradients_reproduce_the_reference(k):
    fx = tc.fixture()
    n, A = tc.GOLDEN_LOSS_SHAPES[k]
    c = tc.loss_case(n, A)
    got = _losses(c, tc.ENTROPY_COEFFS[1])
    want = fx[f"loss{k}_64_stats"]
    err = np.abs(got["stats"] - want)
    print(f"(n, A) = {(n, A)}: stats rel err {np.max(err / np.maximum(np.abs(want), 1e-300)):.2e}")
    assert np.all(err <= 1e-12 * np.abs(want)), (got["stats"], want)
    for name, key in (("grad_logits", "glogits"), ("grad_value", "gvalue"), ("grad_reward", "greward")):
        w64, w32 = fx[f"loss{k}_64_{key}"].reshape(n, -1), fx[f"loss{k}_32_{key}"].reshape(n, -1)
        g = got[name].reshape(n, -1)
        scale = np.max(np.abs(w64), axis=1, keepdims=True)
        print(f"  {name}: max err / row scale {np.max(np.abs(g - w64) / np.maximum(scale, 1e-300)):.2e}")
        assert np.all(np.abs(g - w64) <= 1e-12 * scale)
        # the float32 run of the reference rounds its log-softmax at |lp| 2^-24 (|lp| up to ~3000 on the shifted rows): loose, but it
        # shows that the float64 record is the same quantity
        assert np.all(np.abs(g - w32) <= 1e-2 * scale + 1e-6)


def test_weight_zero_row_and_shift_row_are_in_the_cases():
    c = tc.loss_case(96, 200)
    assert c["kinds"][:8] == list(tc.ROW_KINDS) and c["weights"][6] == 0.0
    got = _losses(c, 0.2)
    assert np.all(got["grad_logits"][6] == 0.0) and got["stats"][6, 4] == 0.0
    r = c["kinds"].index("shift_not_mask")
    valid = c["valid_msk"][r] == 1
    # the invalid actions carry the softmax: the policy loss of the valid ones is about 1000, not about log(A)
    assert got["stats"][r, 0] > 900.0 and valid.any() and (~valid).any()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_one_cycle_reproduces_the_scheduler(tag):
    fx = tc.fixture()
    epochs, batches, lr0, max_lr = fx[f"sched_{tag}_meta"]
    total = int(epochs * batches)
    want = fx[f"sched_{tag}"]
    assert want.shape == (total + 1, 2)
    got = np.array([one_cycle(k, total, lr0, max_lr) for k in range(total + 1)])
    assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), np.max(np.abs(got - want) / want)
    assert want[0, 1] == 0.95 and np.min(want[:, 1]) < 0.86  # (the momentum cycles: hyper_params["momentum"] is overridden)
    with pytest.raises(ValueError):
        one_cycle(total + 1, total, lr0, max_lr)


def _ulps(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _sgd_recorded_step(s, tag="sgd"):
    """Step s of a recorded run (tag "sgd": torch on float32 tensors, "sgd64": torch on float64 tensors with float32 storage) redone by the
    restatement FROM THE RECORDED STATE of the step before: (params, buf, norm, the recorded params, the recorded buf, the float32
    scale of the largest operand of the sum that makes each value)."""
    fx = tc.fixture()
    lr, mu, wd, max_norm = fx["sgd_meta"]
    p0, grads = tc.sgd_case(300, 3.0)
    p = fx[f"{tag}_params"][s - 1] if s else p0
    buf = fx[f"{tag}_buf"][s - 1] if s else np.zeros_like(p0)
    a, b, norm = sgd_clip_step_host(p, grads[s], buf, lr, mu, wd, max_norm)
    coef = min(1.0, max_norm / (norm + 1e-6))
    want_p, want_b = fx[f"{tag}_params"][s], fx[f"{tag}_buf"][s]
    scale_b = np.maximum.reduce([np.abs(mu * buf.astype(np.float64)), np.abs(coef * grads[s].astype(np.float64)), np.abs(want_b).astype(np.float64)])
    scale_p = np.maximum.reduce([np.abs(p).astype(np.float64), np.abs(want_p).astype(np.float64), lr * np.abs(want_b).astype(np.float64)])
    return a, b, norm, want_p, want_b, scale_p.astype(np.float32), scale_b.astype(np.float32)


def test_sgd_edge_cases():
    fx = tc.fixture()
    lr, mu, wd, max_norm = fx["sgd_meta"]
    a, b = fx["sgd64_params"][0], fx["sgd64_buf"][0]
    # a NaN norm propagates, a zero gradient leaves weight decay and momentum alone
    pn, bn, nn_ = sgd_clip_step_host(a, np.full_like(a, np.nan), b, lr, mu, wd, max_norm)
    assert np.isnan(nn_) and np.all(np.isnan(pn))
    pz, bz, nz = sgd_clip_step_host(a, np.zeros_like(a), b, lr, mu, 0.0, max_norm)
    assert nz == 0.0 and np.array_equal(bz, (mu * b.astype(np.float64)).astype(np.float32))


def test_sgd_steps_reproduce_torch():
    """The three recorded steps of clip_grad_norm_ + torch.optim.SGD.step within 1 float32 ulp of every value.  The record is torch's own
    code on float64 tensors with the state stored as float32 between the steps (sgd64_*): the arithmetic that ipp_pvnet_sgd_step and its
    restatement are specified to have (fp64 from the fp32 loads, one rounding per stored value).  Checked step by step from the recorded
    state, and as a chain of three steps from the restatement's own state."""
    fx = tc.fixture()
    lr, mu, wd, max_norm = fx["sgd_meta"]
    p0, grads = tc.sgd_case(300, 3.0)
    p, buf = p0, np.zeros_like(p0)
    for s in range(tc.SGD_STEPS):
        a, b, norm, want_p, want_b, _, _ = _sgd_recorded_step(s, "sgd64")
        assert norm > max_norm  # (the clip acts)
        assert abs(norm - fx["sgd64_norm"][s]) <= 1e-14 * norm
        p, buf, _ = sgd_clip_step_host(p, grads[s], buf, lr, mu, wd, max_norm)
        figures = [float(np.max(_ulps(x, w))) for x, w in ((a, want_p), (b, want_b), (p, want_p), (buf, want_b))]
        print(f"step {s + 1}: from the recorded state params {figures[0]} ulp, buffer {figures[1]} ulp; chained {figures[2]} / {figures[3]} ulp")
        assert max(figures) <= 1.0


def test_sgd_steps_against_torch_in_float32():
    """The same three steps as the reference runs them, on float32 tensors (sgd_*), each redone from the recorded state.  torch rounds
    where the restatement does not, so the bar is what those roundings allow, in ulps of the largest operand of the sum that makes a
    value (a float32 sum is exact to half an ulp of its operands, not of a result that cancels):
      momentum buffer: fl(coef g), + fl(wd p), fl(mu buf) and their sum round 4 x 0.5 ulp, the float32 clip coefficient is off by its
        own rounding (1 ulp on coef g) plus the float32 norm's relative error e_n, read off the two records (e_n 2^24 ulp), and the
        restatement's one rounding adds 0.5: 3.5 + e_n 2^24 ulp;
      params: fl(lr buf), the subtraction and the restatement's rounding, 3 x 0.5 ulp, plus lr times the buffer's bound.
    Measured: buffer 1.0 / 1.25 / 1.875 ulp over the three steps, params 1.0 ulp; a first step (zeroed buffer: fewer roundings) agrees
    within 1 ulp of the values themselves, asserted as such."""
    fx = tc.fixture()
    lr = fx["sgd_meta"][0]
    for s in range(tc.SGD_STEPS):
        a, b, norm, want_p, want_b, scale_p, scale_b = _sgd_recorded_step(s, "sgd")
        e_n = abs(fx["sgd_norm"][s] - fx["sgd64_norm"][s]) / fx["sgd64_norm"][s]
        assert e_n <= 2.0 ** -22  # (a float32 norm of 300 terms)
        bar_b = (3.5 + e_n * 2.0 ** 24) * np.spacing(scale_b).astype(np.float64)
        bar_p = 1.5 * np.spacing(scale_p).astype(np.float64) + lr * bar_b
        err_b = np.abs(b.astype(np.float64) - want_b.astype(np.float64))
        err_p = np.abs(a.astype(np.float64) - want_p.astype(np.float64))
        print(f"step {s + 1}: buffer {np.max(err_b / np.spacing(scale_b)):.3f} ulp of its operands (bar {3.5 + e_n * 2.0 ** 24:.2f}), "
              f"params {np.max(err_p / np.spacing(scale_p)):.3f} ulp, worst error / bar {np.max(err_b / bar_b):.2f} / {np.max(err_p / bar_p):.2f}")
        assert np.all(err_b <= bar_b) and np.all(err_p <= bar_p)
        if s == 0:
            assert np.max(_ulps(a, want_p)) <= 1.0 and np.max(_ulps(b, want_b)) <= 1.0


def test_header_declares_and_ffi_binds_the_calls():
    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    for name in ("ipp_pvnet_loss", "ipp_pvnet_sgd_step"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _ffi.PROTOTYPES
    m = re.search(r"#define\s+IPP_PVNET_SGD_SCRATCH\s+(\d+)", txt)
    assert m and int(m.group(1)) == _ffi.IPP_PVNET_SGD_SCRATCH
    assert re.search(r"#define\s+IPP_ABI_VERSION\s+17\b", txt) and _ffi.ABI_VERSION == 17
    lib = _ffi.load()
    assert lib.ipp_pvnet_loss.argtypes is not None and len(lib.ipp_pvnet_loss.argtypes) == 20
    assert len(lib.ipp_pvnet_sgd_step.argtypes) == 13
    # host-side validation needs no GPU: every refusal comes back as an error code with a message, before any device call
    assert lib.ipp_pvnet_loss(*([None] * 8), 4, 8, 1.0, 1.0, 1.0, 0.0, None, None, None, None, 0, None) != 0
    assert b"null" in lib.ipp_last_error()
    assert lib.ipp_pvnet_loss(*([None] * 8), -1, 8, 1.0, 1.0, 1.0, 0.0, None, None, None, None, 0, None) != 0
    assert b"n < 0" in lib.ipp_last_error()
    assert lib.ipp_pvnet_loss(*([None] * 8), 4, 0, 1.0, 1.0, 1.0, 0.0, None, None, None, None, 0, None) != 0
    assert b"num_actions" in lib.ipp_last_error()
    assert lib.ipp_pvnet_sgd_step(None, None, None, 5, 0.1, 0.9, 0.0, 1.0, None, None, 1024, 0, None) != 0
    assert lib.ipp_pvnet_sgd_step(None, None, None, -1, 0.1, 0.9, 0.0, 1.0, None, None, 1024, 0, None) != 0
    assert b"n < 0" in lib.ipp_last_error()


# ------------------------------------------------------------------------------------------------ the recorded train() runs
_batch = tc.e2e_batch


class RecordedReplay:
    """What Trainer.train asks of a ring, served from the fixture's recorded minibatches."""

    def __init__(self, tag):
        fx = tc.fixture()
        self.tag, self.t, self.calls, self.updates = tag, 0, [], []
        self.ids, self.index, self.weights = fx[f"e2e_{tag}_ids"], fx[f"e2e_{tag}_index"], fx[f"e2e_{tag}_weights"]
        self.sample_size = tc.E2E_TRAIN["batch_size"]

    def __len__(self):
        return tc.E2E_SAMPLES

    def _next(self, dtype):
        b = _batch(self.ids[self.t], self.index[self.t], self.weights[self.t], dtype)
        self.t += 1
        return b

    def sample(self, batch_size, num_augmented_samples=0, check_empty=True):
        assert self.tag == "uni" and batch_size == self.sample_size and num_augmented_samples == 0
        return self._next(torch.float64)

    def prioritized(self, batch_size, alpha, beta0, num_epochs):
        assert self.tag == "per" and (batch_size, alpha, beta0, num_epochs) == (self.sample_size, 0.75, 0.4, tc.E2E_TRAIN["num_epochs"])
        outer = self

        class Per:
            sample_size = outer.sample_size

            def __len__(self):
                return len(outer)

            def sample(self):
                return outer._next(torch.float32)

            def step(self):
                outer.calls.append(0)

            def update(self, indices, priorities):
                outer.calls.append(1)
                outer.updates.append((indices.numpy().copy(), priorities.detach().numpy().copy()))

        return Per()


def _network(hp, md):
    case = pc.case(tc.E2E_CASE)
    net = PolicyValueNetwork(hp, md).cpu()
    net.load_state_dict({k: v.clone() for k, v in case["state_dict"].items()}, strict=True)
    return net


@pytest.mark.parametrize("tag", ["uni", "per"])
def test_stock_trainer_reproduces_the_reference_run(tag):
    fx = tc.fixture()
    hp, md = tc.e2e_params(use_per=tag == "per")
    net = _network(hp, md)
    trainer = Trainer(net, hp, fused=False)
    replay = RecordedReplay(tag)
    seen = []
    step = torch.optim.SGD.step

    def recording(self, *a, **k):
        seen.append((self.param_groups[0]["lr"], self.param_groups[0]["momentum"]))
        return step(self, *a, **k)

    # one thread, as the recorded run: the bar's margin is for what is left (another CPU's kernels); more threads change the conv
    # reductions' order, and a ReLU or max-pool that flips on such a rounding moves the PER run by 2e-5 (seen at 8 threads)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    torch.optim.SGD.step = recording
    try:
        history = trainer.train(replay)
    finally:
        torch.optim.SGD.step = step
        torch.set_num_threads(threads)
    steps = fx[f"e2e_{tag}_ids"].shape[0]
    assert replay.t == steps and len(history) == tc.E2E_TRAIN["num_epochs"]
    assert np.array_equal(np.array(seen), fx[f"e2e_{tag}_lr_mom"])
    got = np.concatenate([v.detach().double().numpy().reshape(-1) for v in net.state_dict().values()])
    want = fx[f"e2e_{tag}_final"].astype(np.float64)
    assert got.shape == want.shape
    start = np.concatenate([v.double().numpy().reshape(-1) for v in pc.case(tc.E2E_CASE)["state_dict"].values()])
    bar = 8.0 * max(float(fx[f"e2e_{tag}_spread"]), 2.0 ** -24 * float(np.max(np.abs(want))))
    diff = float(np.max(np.abs(got - want)))
    print(f"{tag}: |got - reference| = {diff:.3e}, bar {bar:.3e}, the run moved the parameters by {np.max(np.abs(want - start)):.3e}")
    assert np.max(np.abs(want - start)) > 100 * bar  # (the run trains: the bar is far below what it changes)
    assert diff <= bar
    for h in history:
        assert all(np.isfinite(v) for v in h.values()) and h["reward_loss"] == 0.0
    if tag == "per":
        # step() before update() after every optimizer step (:174-175), update(indices, value_loss + 1e-8)
        assert replay.calls == [0, 1] * steps and np.array_equal(fx["e2e_per_calls"], replay.calls)
        for s, (idx, pri) in enumerate(replay.updates):
            assert np.array_equal(idx, fx["e2e_per_index"][s])
            assert np.allclose(pri - 1e-8, fx["e2e_per_value_losses"][s], rtol=1e-4, atol=1e-7)
    else:
        assert np.array_equal(fx["e2e_uni_calls"], [0, 1] * steps)  # (the reference calls them on the uniform buffer too: no-ops)


def test_refusals():
    hp, md = tc.e2e_params()
    net = _network(hp, md)
    with pytest.raises(ValueError, match="mask_policy_head"):
        Trainer(net, dict(hp, mask_policy_head=False), fused=False)
    with pytest.raises(ValueError, match="fused=True"):
        Trainer(net, hp, fused=True)  # (a CPU network)
    trainer = Trainer(net, hp, fused=False)
    fx = tc.fixture()
    good = _batch(fx["e2e_uni_ids"][0], fx["e2e_uni_index"][0], fx["e2e_uni_weights"][0], torch.float64)
    with pytest.raises(ValueError, match="schedule"):
        trainer.step(good)
    trainer.set_schedule(4)
    before = [p.detach().clone() for p in net.parameters()]
    bad_actions = tuple(t[:, :-1] if i in (1, 4) else t for i, t in enumerate(good))
    bad_planes = (good[0][:, :-1],) + good[1:]
    bad_rows = good[:2] + (good[2][:-1],) + good[3:]
    minus_one = good[:5] + (torch.full_like(good[5], -1),) + good[6:]
    for bad in (bad_actions, bad_planes, bad_rows, minus_one, good[:6]):
        with pytest.raises(ValueError):
            trainer.step(bad)
    assert all(torch.equal(a, b) for a, b in zip(before, net.parameters())) and trainer.iteration == 0
    trainer.step(good)
    assert trainer.iteration == 1 and not all(torch.equal(a, b) for a, b in zip(before, net.parameters()))


def test_forward_logits_is_forward_without_mask_and_log_softmax():
    hp, md = tc.e2e_params()
    net = _network(hp, md).eval()
    b = _batch(range(5), range(5), np.ones(5), torch.float64)
    msk = b[4].float()
    with torch.no_grad():
        log_p, value, reward, dec = net(b[0], msk)
        logits, value2, reward2, dec2 = net.forward_logits(b[0])
    assert torch.equal(value, value2) and reward is None and reward2 is None and dec is None and dec2 is None
    assert torch.equal(log_p, torch.log_softmax(logits - (1 - msk) * 1000, dim=1))
