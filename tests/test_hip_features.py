"""
GPU tests of the NN input state planes (ipp_state_plane, csrc/k_plane.h) against the golden
planes recorded from the reference's planning/common/features.py and against the oracle on engine states.
"""
import numpy as np
import pytest

from oracle import ipp_oracle as orc
from tests.test_feature_planes_host import KF, check_margin, plane_walk
from tests.test_prior_kernels_host import prior_matrix

pytestmark = pytest.mark.gpu
TOL = 1e-5
UAV = {"max_v": 2, "max_a": 2}


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def test_feature_planes_drop_in_vs_reference(golden):
    """The mirrored generate_input_feature_planes (device state planes) reproduces the reference's output, the
    in-place masking of the history included (features.py:98-99)."""
    from tests.params import example_params
    from ipp_rl_amd.mapping.grid_maps import GridMap
    from ipp_rl_amd.mapping.mappings import Mapping
    from ipp_rl_amd.planning.common.features import EpisodeHistory, generate_input_feature_planes
    from ipp_rl_amd.sensors.cameras import RGBCamera
    from ipp_rl_amd.sensors.models.sensor_models import AltitudeSensorModel

    g = golden("features")
    params = example_params(10)
    gm = GridMap(params)
    sensor = RGBCamera(params["sensor"]["field_of_view"], AltitudeSensorModel(0.05, 0.2), gm)
    mapping = Mapping(gm, sensor)
    info = {"mean": g["mean"], "value_threshold": 0.4, "interval_factor": 0}
    for key, k, adaptive, costs in (("planes_full_adaptive_costs", 3, True, True), ("planes_two_plain", 2, False, False),
                                    ("planes_one_adaptive", 1, True, False)):
        hist = EpisodeHistory(3)
        for i in range(k):
            hist.push(g["states"][i].copy(), g["positions"][i].copy(), float(g["budgets"][i]))
        got = generate_input_feature_planes(mapping, hist, 8, 14, info if adaptive else None, UAV, use_action_costs_input=costs)
        assert got.shape == g[key].shape
        assert np.max(np.abs(got - g[key])) < TOL, key
        if adaptive:  # the history's arrays were masked in place like the reference does
            msk = orc.adaptive_mask(g["mean"], g["states"][k - 1], 0.4, 0.0)
            assert np.all(hist.states[0][~msk, :] == 0) and np.all(hist.states[0][:, ~msk] == 0)


@pytest.mark.parametrize("state,window_rows,dim,fixed,nu", [
    pytest.param("factor", 0, 20, False, 1.5, id="factor-0"), pytest.param("factor", 12, 20, False, 1.5, id="factor-12"),
    pytest.param("dense", 0, 20, False, 1.5, id="dense-0"), pytest.param("factor", -1, 40, True, 1.5, id="patch40"),
    pytest.param("factor", 0, 20, False, 2.5, id="factor-0-nu2.5")])
def test_state_plane_of_engine_slots_vs_oracle(state, window_rows, dim, fixed, nu):
    """Plane of a stepped env slot (factor slots are densified on the device) vs the oracle's plane of the same
    state, with the slot's own mean and with an explicit mean for the mask; then again with interval_factor = 0.5, where the
    mask depends on the slot's diagonal, at a threshold with a margin (tests/test_feature_planes_host.py: pick_threshold)."""
    from ipp_rl_amd import EngineConfig, IPPEngine

    cfg = EngineConfig(x_dim=dim, y_dim=dim, nu=nu)
    ocfg = orc.OracleConfig(x_dim=dim, y_dim=dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b)
    eng = IPPEngine(cfg, capacity=2, state=state, rank_cap=96, window_rows=window_rows, fixed_prior=fixed, score_scratch=True)
    assert int(eng.info.patch_layout) == (1 if window_rows < 0 else 0)
    w = plane_walk(dim)  # (seed 21: white noise, then a waypoint and the measurement noise of each of 6 steps, then other_mean)
    white = w.white
    eng.reset(env_ids=[1], white_noise=white[None])
    st = orc.env_reset(ocfg, white)
    if nu != 1.5:
        st.P = prior_matrix(nu, dim)
    prev = np.array([2.0, 2.0, 14.0])
    for a, eps in zip(w.actions, w.eps):
        eng.step(a[None], prev[None], env_ids=[1], meas_noise=eps[None])
        m = orc.num_measurements(orc.project_fov(ocfg, a), orc.resolution_factor(a))
        orc.env_step(ocfg, st, a, eps[:m])
        prev = a
    mask = orc.adaptive_mask(st.mean, st.P, 0.4, 0.0)
    assert 0 < mask.sum() < mask.size
    assert np.max(np.abs(host(eng.state_plane(1)) - orc.state_plane(st.P, mask))) < TOL
    assert np.max(np.abs(host(eng.state_plane(1, adaptive=False)) - orc.state_plane(st.P))) < TOL
    other_mean = w.other_mean
    mask2 = orc.adaptive_mask(other_mean, st.P, 0.4, 0.0)
    assert np.max(np.abs(host(eng.state_plane(1, mean_for_mask=other_mean)) - orc.state_plane(st.P, mask2))) < TOL
    for label, mean_arg, mean in (("own mean", None, st.mean), ("other mean", other_mean, other_mean)):
        thr, margin = check_margin([st.P], mean, f"{state} {window_rows} {dim} nu={nu} {label}")
        eng.set_adaptive(thr, KF)
        mask3 = orc.adaptive_mask(mean, st.P, thr, KF)
        err = float(np.max(np.abs(host(eng.state_plane(1, mean_for_mask=mean_arg)) - orc.state_plane(st.P, mask3))))
        print(f"state_plane {state} window {window_rows} {dim} x {dim} nu = {nu}, kf = {KF}, {label}: margin {margin:.3g}, max error {err:.3g}")
        assert err < TOL
    eng.close()
