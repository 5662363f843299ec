"""
GPU tests of the comparison-curve kernels on bare arrays (csrc/k_curves.h: ipp_curve_record / _extent / _resample / _reduce) against
NumPy.  Resampling bar: the interpolation is three fp64 roundings on values no larger than max|ys|: 1e-13 max(1, max|ys|) absolute;
the reduction sums at most 67 fp64 terms: 1e-12 relative.
"""
import ctypes as C

import numpy as np
import pytest

from ipp_rl_amd.planning import vec_baselines as vb
from ipp_rl_amd.planning.common.actions import _trapezoid_time

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
MAX_V, MAX_A = 2.0, 2.0


def _env():
    import torch
    from ipp_rl_amd import _ffi

    dev = torch.device("cuda:0")
    return torch, _ffi, _ffi.load(), dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def test_record_appends_and_flags_a_full_log():
    torch, _ffi, lib, dev, stream = _env()
    B, T = 4, 3
    f64 = dict(dtype=torch.float64, device=dev)
    log = torch.full((B, T, 9), -5.0, **f64)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    overflow = torch.zeros(B, dtype=torch.uint8, device=dev)
    rs = np.random.RandomState(0)
    want_x = [[] for _ in range(B)]
    want_y = [[] for _ in range(B)]
    # the step-0 point of every env, then three steps: env 0 stops at length 1, env 1 at 2, env 2 fills the log and overflows, env 3 repeats a time
    executed = [None, [0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 1, 0]]
    prev = np.tile(np.array([2.0, 2.0, 14.0]), (B, 1))
    for step, ex in enumerate(executed):
        metrics = rs.uniform(-2, 2, (B, 8)).astype(np.float32)
        action = prev + rs.uniform(1.0, 9.0, (B, 3))
        action[3] = prev[3] if step == 2 else action[3]  # a hop of length 0: a repeated time
        m_t = torch.as_tensor(metrics, device=dev)
        a_t, p_t = torch.as_tensor(action, **f64), torch.as_tensor(prev, **f64)
        e_t = torch.as_tensor(np.array(ex if ex is not None else [0] * B, dtype=np.uint8), device=dev)
        before = log.clone()
        first = ex is None
        _ffi.check(lib.ipp_curve_record(None, m_t.data_ptr(), None if first else a_t.data_ptr(), None if first else p_t.data_ptr(),
                                        None if first else e_t.data_ptr(), B, int(first), MAX_V, MAX_A, log.data_ptr(), count.data_ptr(),
                                        overflow.data_ptr(), T, 0, stream))
        torch.cuda.synchronize()
        d = action - prev
        dt = _trapezoid_time(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), MAX_V, MAX_A)
        for e in range(B):
            if first or ex[e]:
                if len(want_x[e]) < T:
                    want_x[e].append(0.0 if first else want_x[e][-1] + dt[e])
                    want_y[e].append(metrics[e].astype(np.float64))
                else:
                    assert e == 2 and int(overflow[e]) == 1 and torch.equal(log[e], before[e])  # flag set, log unchanged
        prev = np.where(np.array(ex if ex is not None else [0] * B, dtype=bool)[:, None], action, prev)
    assert [len(x) for x in want_x] == [1, 2, T, 3] and want_x[3][1] == want_x[3][2]
    assert np.array_equal(count.cpu().numpy(), [1, 2, T, 3]) and np.array_equal(overflow.cpu().numpy(), [0, 0, 1, 0])
    got = log.cpu().numpy()
    for e in range(B):
        n = len(want_x[e])
        assert np.allclose(got[e, :n, 0], want_x[e], rtol=1e-15, atol=0) and got[e, 0, 0] == 0.0
        assert np.array_equal(got[e, :n, 1:], np.array(want_y[e]))
        assert np.all(got[e, n:] == -5.0)  # nothing behind the count is written
    # the extent: the largest last time
    mx = torch.zeros(1, **f64)
    _ffi.check(lib.ipp_curve_extent(log.data_ptr(), count.data_ptr(), B, T, mx.data_ptr(), 0, stream))
    assert float(mx.item()) == max(got[e, len(want_x[e]) - 1, 0] for e in range(B))
    # refused calls leave everything as it is
    assert lib.ipp_curve_record(None, None, None, None, None, B, 1, MAX_V, MAX_A, log.data_ptr(), count.data_ptr(), overflow.data_ptr(), T, 0,
                                stream) == -1 and b"ipp_curve_record" in lib.ipp_last_error()


@pytest.mark.parametrize("G", [1, 65])
def test_resample_matches_np_interp(G):
    torch, _ffi, lib, dev, stream = _env()
    T = 6
    rs = np.random.RandomState(1)
    # lengths 1, 2 and T; a repeated time; knots on grid points (max_x = 8, G = 65: a step of 1/8) and a last knot left of max_x; an empty log
    xs = [np.array([0.0]), np.array([0.0, 3.0]), np.array([0.0, 2.0, 2.0, 5.0, 7.5, 8.0]), np.array([0.0, 1.25, 5.0]), np.array([])]
    B, max_x = len(xs), 8.0
    ys = [rs.uniform(-40.0, 40.0, (len(x), 8)) for x in xs]
    log = np.full((B, T, 9), np.nan)
    for e in range(B):
        log[e, :len(xs[e]), 0], log[e, :len(xs[e]), 1:] = xs[e], ys[e]
    log_t = torch.as_tensor(log, dtype=torch.float64, device=dev)
    count = torch.as_tensor(np.array([len(x) for x in xs], dtype=np.int32), device=dev)
    out = torch.full((B, G, 8), 123.0, dtype=torch.float64, device=dev)
    _ffi.check(lib.ipp_curve_resample(log_t.data_ptr(), count.data_ptr(), B, T, max_x, G, out.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    axis = np.linspace(0, max_x, G)
    assert (G == 1 and axis[0] == 0.0) or (2.0 in axis and 5.0 in axis and axis[-1] == 8.0)
    bar = 1e-13 * max(1.0, max(np.abs(y).max() for y in ys if len(y)))
    for e in range(B - 1):
        want = vb.curve_resample_host(xs[e], ys[e], max_x, G)
        err = np.abs(got[e] - want).max()
        print(f"resample G={G} env {e}: max error {err:.3e} (bar {bar:.1e})")
        assert err <= bar, (e, err)
    assert np.all(np.isnan(got[B - 1]))
    if G > 1:  # on a knot: the knot's values; on the repeated time: the later point's; beyond the last knot: the last values
        assert np.array_equal(got[2, 16], ys[2][2]) and np.array_equal(got[2, 40], ys[2][3]) and np.array_equal(got[1, 30:], np.tile(ys[1][1], (35, 1)))
        assert np.array_equal(got[0], np.tile(ys[0][0], (G, 1)))


@pytest.mark.parametrize("B", [1, 3, 67])
def test_reduce_mean_sd_and_reproducible_bits(B):
    torch, _ffi, lib, dev, stream = _env()
    G, T = 5, 4
    rs = np.random.RandomState(B)
    per_env = rs.uniform(1.0, 20.0, (B, G, 8))  # (one sign: the relative bar on the mean is not a statement about cancellation)
    p_t = torch.as_tensor(per_env, dtype=torch.float64, device=dev)
    log = np.zeros((B, T, 9)); log[:, 1, 0] = rs.uniform(1, 50, B)
    log_t = torch.as_tensor(log, dtype=torch.float64, device=dev)
    count = torch.full((B,), 2, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        mean = torch.zeros((G, 8), dtype=torch.float64, device=dev); sd = torch.full((G, 8), -1.0, dtype=torch.float64, device=dev)
        mx = torch.zeros(1, dtype=torch.float64, device=dev)
        _ffi.check(lib.ipp_curve_reduce(p_t.data_ptr(), B, G, mean.data_ptr(), sd.data_ptr(), 0, stream))
        _ffi.check(lib.ipp_curve_extent(log_t.data_ptr(), count.data_ptr(), B, T, mx.data_ptr(), 0, stream))
        torch.cuda.synchronize()
        outs.append((mean.cpu().numpy(), sd.cpu().numpy(), float(mx.item())))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])  # two runs: the same bits
    want_mean, want_sd = vb.curve_reduce_host(per_env)
    mean, sd, mx = outs[0]
    print(f"reduce B={B}: mean error {np.abs(mean - want_mean).max():.3e}, sd error {np.abs(sd - want_sd).max():.3e}")
    assert np.all(np.abs(mean - want_mean) <= 1e-12 * np.abs(want_mean))
    assert np.all(np.abs(sd - want_sd) <= 1e-12 * np.abs(want_sd))
    if B == 1:
        assert np.all(sd == 0.0) and np.array_equal(mean, per_env[0])
    assert mx == log[:, 1, 0].max()
