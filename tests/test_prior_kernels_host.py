"""
CPU-only checks of the prior kinds (include/ipp_engine.h IPP_PRIOR_*): the closed forms against the reference's priors for
nu = 0.5, 2.5 and inf (tests/golden/priors_nu.npz, gen_prior_golden.py), the window rule of every kind
(ipp_min_window_rows_prior), refusal of an unknown kind, and the nu plumbing of EngineConfig / IPPEngine that needs no device.
"""
import ctypes

import numpy as np
import pytest

from tests.conftest import load_golden

NUS = (("nu05_", 0.5), ("nu25_", 2.5), ("nuinf_", float("inf")))


def closed_form(nu, d, sv, ls):
    """sigma^2 * sklearn.gaussian_process.kernels.Matern(ls, nu) at distance d (metres)."""
    u = d / ls
    if nu == 0.5:
        return sv * np.exp(-u)
    if nu == 1.5:
        t = u * np.sqrt(3)
        return sv * (1.0 + t) * np.exp(-t)
    if nu == 2.5:
        t = u * np.sqrt(5)
        return sv * (1.0 + t + t ** 2 / 3.0) * np.exp(-t)
    return sv * np.exp(-(u ** 2) / 2.0)


def prior_matrix(nu, dim, sv=1.82, ls=3.67, res=4.0):
    rows, cols = np.divmod(np.arange(dim * dim), dim)
    d = res * np.hypot(rows[:, None] - rows[None, :], cols[:, None] - cols[None, :])
    return closed_form(nu, d, sv, ls)


def host_config(**kw):
    from ipp_rl_amd import _ffi

    c = _ffi.IppConfig(x_dim=50, y_dim=50, resolution=4.0, tan_half_fov_x=0.57735, tan_half_fov_y=0.57735,
                       rf_altitude=10.0, coeff_a=0.05, coeff_b=0.2, signal_variance=1.82, length_scale=3.67, max_v=2,
                       max_a=2, value_threshold=0.4, interval_factor=0, cluster_radius=5, state_repr=_ffi.IPP_FACTOR,
                       capacity=64, rank_cap=360, max_batch=64, max_measurements=9, tile_threads=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("prefix,nu", NUS)
def test_closed_forms_match_the_reference_priors(prefix, nu):
    g = load_golden("priors_nu")
    assert np.max(np.abs(prior_matrix(nu, 10) - g[prefix + "P0_10"])) < 1e-12
    P50 = prior_matrix(nu, 50)
    assert np.max(np.abs(P50[[0, 1234, 2499]] - g[prefix + "P0_50_rows"])) < 1e-12
    assert np.max(np.abs(np.diag(P50) - g[prefix + "P0_50_diag"])) < 1e-12
    for sv, ls, p00, p01, p011, p599 in g[prefix + "shuffle"]:
        P = prior_matrix(nu, 10, sv, ls)
        assert np.max(np.abs(np.array([P[0, 0], P[0, 1], P[0, 11], P[5, 99]]) - [p00, p01, p011, p599])) < 1e-12


def min_rows(kind, c):
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    rows = ctypes.c_int32(0)
    assert lib.ipp_min_window_rows_prior(ctypes.byref(c), kind, ctypes.byref(rows)) == 0, lib.ipp_last_error()
    return int(rows.value)


def test_min_window_rows_of_every_kind():
    """The smallest windows of the example prior at 4 m cells (fixed prior / shuffled): nu = 0.5 14/16, 1.5 10/12, 2.5 10/12,
    inf 10/12 (both by the Matern 3/2 rule); kind 0 is the old entry point; other priors follow a search of the same 1e-6 bound."""
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    want = {_ffi.IPP_PRIOR_MATERN12: (14, 16), _ffi.IPP_PRIOR_MATERN32: (10, 12), _ffi.IPP_PRIOR_MATERN52: (10, 12),
            _ffi.IPP_PRIOR_RBF: (10, 12)}
    for kind, (fixed, shuffled) in want.items():
        assert min_rows(kind, host_config(fixed_prior=1)) == fixed
        assert min_rows(kind, host_config(fixed_prior=0)) == shuffled
    for fp in (0, 1):
        old = ctypes.c_int32(0)
        c = host_config(fixed_prior=fp)
        assert lib.ipp_min_window_rows(ctypes.byref(c), ctypes.byref(old)) == 0
        assert old.value == min_rows(_ffi.IPP_PRIOR_MATERN32, c)
    nus = {_ffi.IPP_PRIOR_MATERN12: 0.5, _ffi.IPP_PRIOR_MATERN32: 1.5, _ffi.IPP_PRIOR_MATERN52: 1.5, _ffi.IPP_PRIOR_RBF: 1.5}
    for sv, ls, res in ((1.0, 2.0, 1.0), (3.5, 10.0, 4.0), (0.3, 1.5, 2.0)):
        for fp in (0, 1):
            l_max = ls * (1.0 if fp else 1.2)
            for kind, nu in nus.items():
                r = 1
                while closed_form(nu, r * res, sv, l_max) > 1e-6:
                    r += 1
                assert min_rows(kind, host_config(signal_variance=sv, length_scale=ls, resolution=res, fixed_prior=fp)) == r


def test_unknown_kind_is_refused():
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    c = host_config()
    rows, nbytes = ctypes.c_int32(0), ctypes.c_uint64(0)
    for kind in (-1, 4, 99):
        assert lib.ipp_min_window_rows_prior(ctypes.byref(c), kind, ctypes.byref(rows)) < 0
        assert b"prior kind" in lib.ipp_last_error()
        assert lib.ipp_engine_arena_bytes_prior(ctypes.byref(c), kind, ctypes.byref(nbytes)) < 0
        assert b"prior kind" in lib.ipp_last_error()
        handle = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(512)
        arena = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
        assert lib.ipp_engine_create_prior(ctypes.byref(c), kind, 0, arena, 256, ctypes.byref(handle)) < 0
        assert b"prior kind" in lib.ipp_last_error()


def test_arena_bytes_of_kind_0_and_narrow_windows():
    """Kind 0 sizes the arena as the old entry does; a window below a kind's minimum is refused with that minimum."""
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for wr in (0, 10, 12):
        c = host_config(window_rows=wr, fixed_prior=1)
        assert lib.ipp_engine_arena_bytes(ctypes.byref(c), ctypes.byref(a)) == 0
        assert lib.ipp_engine_arena_bytes_prior(ctypes.byref(c), _ffi.IPP_PRIOR_MATERN32, ctypes.byref(b)) == 0
        assert a.value == b.value
    for kind, rows in ((_ffi.IPP_PRIOR_MATERN12, 14), (_ffi.IPP_PRIOR_MATERN52, 10), (_ffi.IPP_PRIOR_RBF, 10)):
        c = host_config(window_rows=rows, fixed_prior=1)
        assert lib.ipp_engine_arena_bytes_prior(ctypes.byref(c), kind, ctypes.byref(a)) == 0, lib.ipp_last_error()
        c.window_rows = rows - 1
        assert lib.ipp_engine_arena_bytes_prior(ctypes.byref(c), kind, ctypes.byref(a)) < 0
        assert f"window_rows >= {rows}".encode() in lib.ipp_last_error()


def test_nu_plumbing_without_device():
    from ipp_rl_amd import EngineConfig, _ffi, engine
    from tests.params import example_params

    assert EngineConfig().nu == 1.5
    p = example_params(20, 20)
    assert EngineConfig.from_params(p).nu == float(p["mapping"].get("nu", 1.5))
    for nu in (0.5, 2.5, float("inf"), 1.5):
        p["mapping"]["nu"] = nu
        assert EngineConfig.from_params(p).nu == nu
    del p["mapping"]["nu"]
    assert EngineConfig.from_params(p).nu == 1.5
    assert engine.prior_kind(1.5) == _ffi.IPP_PRIOR_MATERN32 and engine.prior_kind(0.5) == _ffi.IPP_PRIOR_MATERN12
    assert engine.prior_kind(2.5) == _ffi.IPP_PRIOR_MATERN52 and engine.prior_kind(np.inf) == _ffi.IPP_PRIOR_RBF
    assert engine.prior_kind("inf") == _ffi.IPP_PRIOR_RBF
    for bad in (1.0, 0.0, -0.5, 3.5, None, "x"):
        with pytest.raises(ValueError, match="0.5, 1.5, 2.5 or inf"):
            engine.prior_kind(bad)
    assert EngineConfig(nu=0.5) != EngineConfig()  # (the compat engines are cached per configuration)
    from ipp_rl_amd import _runtime

    assert _runtime.config_key(EngineConfig(nu=0.5)) != _runtime.config_key(EngineConfig())
    assert _runtime.prior_nu({"nu": 2.5, "fit_gaussian_process": True}) == 2.5
    assert _runtime.prior_nu({"nu": 2.5, "fit_gaussian_process": False}) == 1.5
