"""
CPU checks of the batched feature planes (ipp_feature_planes): the entry record and its packing, the channel layout of every
spec, rejected specs and arguments, and a NumPy restatement of generate_input_feature_planes (planning/common/features.py:83-151)
against the reference's outputs recorded in tests/golden/planes.npz (gen_plane_golden.py) at 1e-12.  The restatement is the
definition the device kernel is tested against in tests/test_hip_feature_planes.py.
"""
import ctypes
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planes.npz")
RES, DIM = 4.0, 10
TAN = math.tan(0.5 * math.radians(60.0))


# ----------------------------------------------------------------------------- NumPy restatement
def min_max_normalize(x):
    lo, hi = np.min(x), np.max(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / hi if lo == hi else (x - lo) / (hi - lo)


def footprint(pos, W, H, res=RES, tanx=TAN, tany=TAN):
    """sensors/cameras.py:49-75: (xl, xr, yu, yd)."""
    cx, cy = np.floor(2 * pos[2] * tanx / res), np.floor(2 * pos[2] * tany / res)
    gx, gy = np.floor(pos[0] / res), np.floor(pos[1] / res)
    rx, ry = np.floor(0.5 * cx), np.floor(0.5 * cy)
    return (int(np.clip(gx - rx, 0, W - 1)), int(np.clip(gx + rx, 0, W - 1)), int(np.clip(gy - ry, 0, H - 1)), int(np.clip(gy + ry, 0, H - 1)))


def fov_plane(pos, W, H):
    xl, xr, yu, yd = footprint(pos, W, H)
    sel = np.zeros(W * H, dtype=bool)
    for x in range(xl, xr):
        for y in range(yu, yd):
            sel[W * x + y] = True  # flatten_grid_index of (x, y): x_dim * x + y
    return np.outer(sel, sel).astype(np.float64)


def cost_plane(pos0, W, H, min_alt, uav=None, res=RES):
    n = W * H
    costs = np.zeros(n)
    for x in range(W):
        for y in range(H):
            d = np.array([x * res + 0.5 * res, y * res + 0.5 * res, min_alt]) - np.array([pos0[0], pos0[1], min_alt])
            dist = np.sqrt(np.sum(d * d))
            if uav is None:
                costs[W * x + y] = dist
            else:
                d_acc = min(dist * 0.5, uav["max_v"] ** 2 / (2 * uav["max_a"]))
                costs[W * x + y] = (dist - 2 * d_acc) / uav["max_v"] + 2 * np.sqrt(2 * d_acc / uav["max_a"])
    return min_max_normalize(np.repeat(costs[:, None], n, axis=1))


def state_plane(state, mean=None, thr=None, kf=None):
    s = np.array(state, dtype=np.float64, copy=True)
    if mean is not None:
        m = np.asarray(mean).ravel() + kf * np.diag(s) >= thr
        s[~m, :] = 0
        s[:, ~m] = 0
    return min_max_normalize(s)


def ref_planes(states, positions, budgets, H, W, Hg, *, fov, costs, mean=None, thr=None, kf=None, min_alt=8.0, max_alt=14.0, uav=None):
    """generate_input_feature_planes on copies: states / positions / budgets newest first (len <= H)."""
    n = W * Hg
    out = []
    for s, p, b in zip(states, positions, budgets):
        sp = state_plane(s, mean, thr, kf)
        if fov:
            out += [sp, fov_plane(p, W, Hg), b * np.ones((n, n))]
        else:
            out += [sp, p[0] / (W * RES) * np.ones((n, n)), p[1] / (W * RES) * np.ones((n, n)),
                    (p[2] - min_alt) / (max_alt - min_alt) * np.ones((n, n)), b * np.ones((n, n))]
    out += [np.zeros((n, n))] * ((3 if fov else 5) * (H - len(states)))
    if costs and not fov:
        out.append(cost_plane(positions[0], W, Hg, min_alt, uav))
    return np.array(out)


def golden_case(g, name):
    """The inputs of one recorded case (newest first) and its spec."""
    desc = bool(g[f"{name}_descent"])
    idx = g[f"{name}_idx"]
    S = g["descent_states"] if desc else g["states"]
    P = g["descent_positions"] if desc else g["positions"]
    B = g["descent_budgets"] if desc else g["budgets"]
    kw = dict(fov=bool(g[f"{name}_fov"]), costs=bool(g[f"{name}_costs"]))
    if g[f"{name}_adaptive"]:
        kw.update(mean=g["mean"].ravel(), thr=float(g[f"{name}_thr"]), kf=float(g[f"{name}_kf"]))
    return [S[i] for i in idx], [P[i] for i in idx], [B[i] for i in idx], kw


def case_names(g):
    return sorted(k[:-len("_idx")] for k in g.files if k.endswith("_idx"))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_matches_reference(golden):
    g = golden
    uav = {"max_v": float(g["max_v"]), "max_a": float(g["max_a"])}
    names = case_names(g)
    assert len(names) == 8 + 5 + 2
    for name in names:
        S, P, B, kw = golden_case(g, name)
        got = ref_planes(S, P, B, int(g["history"]), DIM, DIM, uav=uav, min_alt=float(g["min_altitude"]), max_alt=float(g["max_altitude"]), **kw)
        with np.errstate(invalid="ignore"):
            proj = got @ g["proj"]
        np.testing.assert_allclose(proj, g[f"{name}_proj"], rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
        if f"{name}_planes" in g.files:
            np.testing.assert_allclose(got.astype(np.float32), g[f"{name}_planes"], rtol=0, atol=0, equal_nan=True, err_msg=name)
    # the recorded cases cover what the device must reproduce: short histories, the empty mask, FoV sets
    assert np.isnan(g["nanmask_proj"][0]).all() and not np.isnan(g["nanmask_proj"][1:]).any()
    assert len(g["grow0_idx"]) == 1 and len(g["grow1_idx"]) == 2
    assert g["final_f1c0a1_proj"].shape[0] == 9 and g["final_f0c1a1_proj"].shape[0] == 16
    assert np.array_equal(g["final_f1c1a1_proj"], g["final_f1c0a1_proj"], equal_nan=True)  # FoV mode returns before the cost plane


# ----------------------------------------------------------------------------- spec, entries, channel layout
def test_channel_layout_of_every_spec():
    from ipp_rl_amd.feature_planes import PlaneSpec

    for H in (1, 3, 8):
        assert PlaneSpec(H, min_altitude=8, max_altitude=14).channels == 5 * H
        assert PlaneSpec(H, use_costs=True, min_altitude=8, max_altitude=14).channels == 5 * H + 1
        assert PlaneSpec(H, use_fov=True).channels == 3 * H
        assert PlaneSpec(H, use_fov=True, use_costs=True).channels == 3 * H  # FoV mode has no cost plane
    assert PlaneSpec(2, use_costs=True, min_altitude=8, max_altitude=14).channel_names() == [
        "state[0]", "x[0]", "y[0]", "z[0]", "budget[0]", "state[1]", "x[1]", "y[1]", "z[1]", "budget[1]", "cost"]
    assert PlaneSpec(1, use_fov=True).channel_names() == ["state[0]", "fov[0]", "budget[0]"]
    hp = {"input_history_length": 3, "use_fov_input": False, "use_action_costs_input": True}
    s = PlaneSpec.from_params(hp, {"min_altitude": 8, "max_altitude": 14})
    assert (s.history, s.use_fov, s.use_costs, s.min_altitude, s.max_altitude, s.channels) == (3, False, True, 8.0, 14.0, 16)
    s = PlaneSpec.from_params(dict(hp, use_fov_input=True), {"min_altitude": 8, "max_altitude": 14})
    assert s.use_fov and s.channels == 9


def test_entry_record_matches_the_c_struct():
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.feature_planes import ENTRY_DTYPE, ENTRY_WORDS, PlaneSpec

    assert ENTRY_DTYPE.itemsize == 72 and ENTRY_WORDS == 18
    assert [ENTRY_DTYPE.fields[k][1] for k in ("root_env", "rank", "path", "valid", "reserved", "position", "budget")] == [0, 4, 8, 32, 36, 40, 64]
    assert ctypes.sizeof(_ffi.IppPlaneSpec) == 6 * 4 + 2 * 8
    c = PlaneSpec(3, use_costs=True, adaptive=False, min_altitude=8, max_altitude=14).to_c()
    assert (c.history, c.use_fov, c.use_costs, c.adaptive, c.use_flight_time, c.min_altitude, c.max_altitude) == (3, 0, 1, 0, 1, 8.0, 14.0)
    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    import re

    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ipp_plane_spec \{(.*?)\} ipp_plane_spec;", txt, flags=re.S).group(1), flags=re.S)
    names = [n.strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert names == [f[0] for f in _ffi.IppPlaneSpec._fields_]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ipp_plane_entry \{(.*?)\} ipp_plane_entry;", txt, flags=re.S).group(1), flags=re.S)
    names = [re.sub(r"\[.*\]", "", n).strip() for part in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in part.split(",")]
    assert names == list(ENTRY_DTYPE.names)


def test_entry_packing():
    from ipp_rl_amd.feature_planes import ENTRY_WORDS, make_entry, pack_entries

    e = make_entry(7, [1.0, 2.0, 3.0], 0.25, rank=4, path=[3, 9, -1])
    assert (int(e["root_env"]), int(e["rank"]), int(e["valid"]), list(e["path"])) == (7, 4, 1, [3, 9, -1, -1, -1, -1])
    recs = pack_entries([[e], [e, make_entry(1, [0, 0, 8], 1.0)], []], history=3)
    assert recs.shape == (3, 3)
    assert list(recs["valid"].sum(axis=1)) == [1, 2, 0]
    assert (recs["path"][recs["valid"] == 0] == -1).all()
    words = recs.view(np.int32).reshape(3, 3, ENTRY_WORDS)
    assert words[0, 0, 0] == 7 and words[0, 0, 1] == 4 and words[0, 0, 8] == 1
    assert recs.view(np.float64).reshape(3, 3, 9)[0, 0, 5:9].tolist() == [1.0, 2.0, 3.0, 0.25]
    with pytest.raises(ValueError):
        pack_entries([[e] * 4], history=3)
    with pytest.raises(ValueError):
        make_entry(0, [0, 0, 8], 1.0, path=list(range(7)))


def test_bad_specs_raise():
    from ipp_rl_amd.feature_planes import PlaneSpec

    with pytest.raises(ValueError):
        PlaneSpec(0, use_fov=True)
    with pytest.raises(ValueError):
        PlaneSpec(65, use_fov=True)
    with pytest.raises(ValueError):
        PlaneSpec(3)  # position mode without altitudes
    with pytest.raises(ValueError):
        PlaneSpec(3, min_altitude=8, max_altitude=8)
    with pytest.raises(ValueError):
        PlaneSpec(3, min_altitude=float("nan"), max_altitude=14)


def test_c_entry_point_rejects_bad_calls_without_a_gpu():
    from ipp_rl_amd import _ffi

    lib = _ffi.load()
    spec = _ffi.IppPlaneSpec(history=3, use_fov=1)
    assert lib.ipp_feature_planes(None, ctypes.byref(spec), None, 1, None, None, None, None) == -1
    assert b"null" in lib.ipp_last_error()


def test_vec_env_feature_history_needs_budget_mode():
    from ipp_rl_amd.vec_env import VecIPPEnv

    with pytest.raises(ValueError):
        VecIPPEnv.check_feature_history(3, budget=None)
    with pytest.raises(ValueError):
        VecIPPEnv.check_feature_history(-1, budget=200.0)
    VecIPPEnv.check_feature_history(3, budget=200.0)
    VecIPPEnv.check_feature_history(0, budget=None)
