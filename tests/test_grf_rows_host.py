"""
CPU tests of grf_rows (IPPEngine / VecIPPEnv, ipp_set_grf_rows): the argument is validated before the device is touched, and the
grid rule of grf_rows="all" -- square, even, 4 .. 256 cells a side -- is stated once on the host.
"""
import pytest


@pytest.mark.parametrize("bad", ["ALL", "none", "", True, 1, 0, ("all",)])
def test_other_values_raise_before_the_device_is_touched(bad):
    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.vec_env import VecIPPEnv

    cfg = EngineConfig(x_dim=40, y_dim=40)
    with pytest.raises(ValueError, match="grf_rows"):
        IPPEngine(cfg, capacity=4, grf_rows=bad)
    with pytest.raises(ValueError, match="grf_rows"):
        VecIPPEnv(cfg, 4, episode_steps=4, window_rows=-1, budget=60.0, grf_rows=bad)
    with pytest.raises(ValueError, match="grf_rows"):
        VecIPPEnv(cfg, 4, episode_steps=4, grf_rows=bad)


def test_grid_rule_table():
    from ipp_rl_amd.engine import GRF_ROWS_MAX, check_grf_rows, grf_rows_grid_ok

    assert GRF_ROWS_MAX == 256
    for n in (4, 34, 50, 128, 130, 256):
        assert grf_rows_grid_ok(n, n), n
    for n in (2, 9, 35, 258):
        assert not grf_rows_grid_ok(n, n), n
    assert not grf_rows_grid_ok(40, 50) and not grf_rows_grid_ok(50, 40)
    assert check_grf_rows(None) is None and check_grf_rows("all") == "all"


def test_the_binding_declares_the_call():
    from ipp_rl_amd import _ffi

    assert "ipp_set_grf_rows" in _ffi.PROTOTYPES and _ffi.ABI_VERSION == 17
