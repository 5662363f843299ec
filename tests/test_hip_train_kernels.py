"""
GPU tests of the trainer's two calls (ipp_pvnet_loss, ipp_pvnet_sgd_step: csrc/k_train.h) against the fp64 restatements of
planning/mcts_zero/training.py, which tests/test_training_host.py pins to the reference:
  * loss: (n, A) = (1, 1), (2, 63), (3, 64), (3, 65), (5, 257), (4, 1025), (2, 20011), (96, 200) -- one action, the wave and its
    neighbours, one more than the workgroup, several strides of it, a row beyond any register file, the reference's batch -- with the row
    kinds of tests/training_cases.py (all masked, one valid, all valid, one-hot target, valid mass 0.7, weight 0, logits spanning +-80,
    valid logits at -2000 against invalid ones at 0) in every shape that has the rows, with and without reward, entropy coefficient 0
    and 0.2.  The kernel is fp64 inside and every reduction sums terms of one sign, so: stats within 1e-10 x (pc pl + vc vl + rc rl +
    |ec| H) of the restatement; gradients within 2^-23 |want| + 1e-9 x (the row's largest |want|); two runs bit-identical;
  * SGD: N = 1, 255, 256, 257, 65 537, 200 003 (one element, the workgroup and its neighbours, 65 workgroups and 196 with ragged
    tails), the norm below and above max_norm, zero gradients, wd = 0, mu = 0, three consecutive steps: params and buffer within 1
    float32 ulp of the restatement, the norm within 1e-12 relative, two runs bit-identical;
  * bad arguments return an error and leave the outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

from tests import training_cases as tc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def host(t):
    return t.detach().cpu().numpy()


class Calls:
    def __init__(self):
        import torch

        from ipp_rl_amd import _ffi

        self.torch, self.ffi, self.lib = torch, _ffi, _ffi.load()
        self.dev = torch.device("cuda:0")
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def loss(self, c, with_reward, ec, fill=7.0):
        """(rc, stats, grad_logits, grad_value, grad_reward) of one call; the outputs start at `fill`."""
        torch = self.torch
        n, A = c["logits"].shape
        d = {k: self.up(c[k]) for k in ("logits", "target_policy", "valid_msk", "value", "reward", "target_value", "target_reward", "weights")}
        stats = torch.full((n, 6), fill, dtype=torch.float64, device=self.dev)
        gl = torch.full((n, A), fill, dtype=torch.float32, device=self.dev)
        gv, gr = torch.full((n,), fill, dtype=torch.float32, device=self.dev), torch.full((n,), fill, dtype=torch.float32, device=self.dev)
        ptr = lambda t: t.data_ptr()  # noqa: E731
        rc = self.lib.ipp_pvnet_loss(ptr(d["logits"]), ptr(d["target_policy"]), ptr(d["valid_msk"]), ptr(d["value"]),
                                     ptr(d["reward"]) if with_reward else None, ptr(d["target_value"]),
                                     ptr(d["target_reward"]) if with_reward else None, ptr(d["weights"]), n, A, tc.COEFFS["policy"],
                                     tc.COEFFS["value"], tc.COEFFS["reward"] if with_reward else 0.0, ec, ptr(stats), ptr(gl), ptr(gv),
                                     ptr(gr) if with_reward else None, 0, self.stream)
        return rc, host(stats), host(gl), host(gv), host(gr)

    def sgd(self, p, g, buf, lr, mu, wd, max_norm, scratch_doubles=None):
        torch = self.torch
        norm = torch.full((1,), -1.0, dtype=torch.float64, device=self.dev)
        scratch = torch.zeros((self.ffi.IPP_PVNET_SGD_SCRATCH,), dtype=torch.float64, device=self.dev)
        rc = self.lib.ipp_pvnet_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), int(p.numel()), lr, mu, wd, max_norm, norm.data_ptr(),
                                         scratch.data_ptr(), C.c_uint64(scratch.numel() if scratch_doubles is None else scratch_doubles), 0,
                                         self.stream)
        return rc, norm


@pytest.fixture(scope="module")
def calls():
    return Calls()


@pytest.mark.parametrize("ec", tc.ENTROPY_COEFFS)
@pytest.mark.parametrize("with_reward", [True, False])
@pytest.mark.parametrize("shape", tc.LOSS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_matches_the_restatement(calls, shape, with_reward, ec):
    from ipp_rl_amd.planning.mcts_zero import pv_losses_host

    n, A = shape
    c = tc.loss_case(n, A)
    assert c["kinds"][:min(n, 8)] == list(tc.ROW_KINDS[:min(n, 8)])
    pc_, vc_, rc_ = tc.COEFFS["policy"], tc.COEFFS["value"], tc.COEFFS["reward"] if with_reward else 0.0
    want = pv_losses_host(c["logits"], c["target_policy"], c["valid_msk"], c["value"], c["reward"] if with_reward else None, c["target_value"],
                          c["target_reward"] if with_reward else None, c["weights"], pc_, vc_, rc_, ec)
    rc, stats, gl, gv, gr = calls.loss(c, with_reward, ec)
    assert rc == 0, calls.lib.ipp_last_error()
    ws = want["stats"]
    scale = (pc_ * ws[:, 0] + vc_ * ws[:, 1] + rc_ * ws[:, 2] + abs(ec) * ws[:, 3])[:, None]
    err = np.abs(stats - ws)
    print(f"stats: max err / scale {np.max(err / scale):.2e}")
    assert np.all(scale > 0) and np.all(err <= 1e-10 * scale)
    if not with_reward:
        assert np.all(stats[:, 2] == 0.0) and np.all(gr == 7.0)  # (no reward: the loss is 0, grad_reward is not written)
    for name, got, w in (("logits", gl, want["grad_logits"]), ("value", gv, want["grad_value"])) + \
            ((("reward", gr, want["grad_reward"]),) if with_reward else ()):
        got, w = got.reshape(n, -1).astype(np.float64), w.reshape(n, -1)
        bar = 2.0 ** -23 * np.abs(w) + 1e-9 * np.max(np.abs(w), axis=1, keepdims=True)
        e = np.abs(got - w)
        print(f"grad_{name}: worst err / bar {np.max(e / np.maximum(bar, 1e-300)):.3f}")
        assert np.all(e <= bar)
    if n > 6:
        assert np.all(gl[6] == 0.0) and gv[6] == 0.0 and stats[6, 4] == 0.0  # (weight 0)
    again = calls.loss(c, with_reward, ec, fill=-3.0)
    assert again[0] == 0
    for a, b in zip((stats, gl, gv), again[1:4]):
        assert a.tobytes() == b.tobytes()
    if with_reward:
        assert gr.tobytes() == again[4].tobytes()


def test_loss_bad_arguments_launch_nothing(calls):
    lib, torch = calls.lib, calls.torch
    c = tc.loss_case(3, 65)
    d = {k: calls.up(c[k]) for k in ("logits", "target_policy", "valid_msk", "value", "reward", "target_value", "target_reward", "weights")}
    stats = torch.full((3, 6), 7.0, dtype=torch.float64, device=calls.dev)
    gl = torch.full((3, 65), 7.0, dtype=torch.float32, device=calls.dev)
    gv, gr = torch.full((3,), 7.0, dtype=torch.float32, device=calls.dev), torch.full((3,), 7.0, dtype=torch.float32, device=calls.dev)
    good = [d["logits"].data_ptr(), d["target_policy"].data_ptr(), d["valid_msk"].data_ptr(), d["value"].data_ptr(), d["reward"].data_ptr(),
            d["target_value"].data_ptr(), d["target_reward"].data_ptr(), d["weights"].data_ptr(), 3, 65, 1.0, 1.0, 1.0, 0.1,
            stats.data_ptr(), gl.data_ptr(), gv.data_ptr(), gr.data_ptr(), 0, calls.stream]

    def call(**over):
        a = list(good)
        for k, v in over.items():
            a[int(k[1:])] = v
        return lib.ipp_pvnet_loss(*a)

    for over, text in ((dict(a0=None), b"null"), (dict(a1=None), b"null"), (dict(a2=None), b"null"), (dict(a3=None), b"null"),
                       (dict(a5=None), b"null"), (dict(a7=None), b"null"), (dict(a14=None), b"null"), (dict(a15=None), b"null"),
                       (dict(a16=None), b"null"), (dict(a4=None), b"together"), (dict(a6=None), b"together"), (dict(a17=None), b"together"),
                       (dict(a8=-1), b"n < 0"), (dict(a9=0), b"num_actions < 1")):
        assert call(**over) != 0, over
        assert text in lib.ipp_last_error(), (over, lib.ipp_last_error())
    assert call(a8=0) == 0  # (an empty minibatch: success without a launch)
    torch.cuda.synchronize()
    assert bool((stats == 7.0).all()) and bool((gl == 7.0).all()) and bool((gv == 7.0).all()) and bool((gr == 7.0).all())


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("case", tc.SGD_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("N", tc.SGD_SIZES)
def test_sgd_matches_the_restatement(calls, N, case):
    from ipp_rl_amd.planning.mcts_zero import sgd_clip_step_host

    name, scale, lr, mu, wd, max_norm = case
    p0, grads = tc.sgd_case(N, scale)
    runs = []
    for _ in range(2):
        p, buf = calls.up(p0), calls.up(np.zeros_like(p0))
        hp, hb = p0, np.zeros_like(p0)
        out = []
        for s in range(tc.SGD_STEPS):
            g = calls.up(grads[s])
            rc, norm = calls.sgd(p, g, buf, lr, mu, wd, max_norm)
            assert rc == 0, calls.lib.ipp_last_error()
            hp, hb, hn = sgd_clip_step_host(hp, grads[s], hb, lr, mu, wd, max_norm)
            gp, gb, gn = host(p), host(buf), float(host(norm)[0])
            if not runs:
                if name == "above" and N > 1:
                    assert hn > max_norm
                if name == "below":
                    assert hn < max_norm
                assert abs(gn - hn) <= 1e-12 * hn
                up, ub = float(np.max(_ulps(gp, hp))), float(np.max(_ulps(gb, hb)))
                if s == tc.SGD_STEPS - 1:
                    print(f"N = {N}, {name}: step {s + 1} params {up} ulp, buffer {ub} ulp, norm {gn:.6g}")
                assert up <= 1.0 and ub <= 1.0
            out.append((gp.tobytes(), gb.tobytes(), gn))
        runs.append(out)
    assert runs[0] == runs[1]


def test_sgd_bad_arguments_launch_nothing(calls):
    lib, torch = calls.lib, calls.torch
    p0, grads = tc.sgd_case(65537, 1.0)
    p, g, buf = calls.up(p0), calls.up(grads[0]), calls.up(np.zeros_like(p0))
    assert calls.sgd(p, g, buf, 0.1, 0.9, 0.0, 1.0, scratch_doubles=64)[0] != 0  # (65 workgroups write 65 partial sums)
    assert b"scratch" in lib.ipp_last_error()
    norm = torch.zeros((1,), dtype=torch.float64, device=calls.dev)
    scratch = torch.zeros((1024,), dtype=torch.float64, device=calls.dev)
    good = [p.data_ptr(), g.data_ptr(), buf.data_ptr(), 65537, 0.1, 0.9, 0.0, 1.0, norm.data_ptr(), scratch.data_ptr(), C.c_uint64(1024), 0,
            calls.stream]
    for i in (0, 1, 2, 8, 9):
        a = list(good)
        a[i] = None
        assert lib.ipp_pvnet_sgd_step(*a) != 0 and b"null" in lib.ipp_last_error()
    a = list(good)
    a[3] = -1
    assert lib.ipp_pvnet_sgd_step(*a) != 0 and b"n < 0" in lib.ipp_last_error()
    a[3] = 0
    assert lib.ipp_pvnet_sgd_step(*a) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(p), p0) and not host(buf).any() and float(norm[0]) == 0.0
