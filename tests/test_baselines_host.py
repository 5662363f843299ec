"""
CPU checks of the baseline missions' host restatements (planning/vec_baselines.py) against tests/golden/baselines.npz, recorded from the
reference's planning/baselines/*.py by tests/golden/gen_golden_baselines.py: the lawnmower and spiral tables, the replay of every
recorded random-discrete and random-continuous sequence, the np.interp curves, and the ABI's declarations.
"""
import os
import re

import numpy as np
import pytest

from ipp_rl_amd.planning import vec_baselines as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, DTB, ALT_LO, ALT_HI, SPACING, STEP_SIZE, NUM_WAYPOINTS, SLOPE = 4, 4, 8, 14, 3, 8, 40, 10  # gen_golden_baselines.py
MAX_V, MAX_A = 2.0, 2.0
INIT = np.array([2.0, 2.0, 14.0])


@pytest.mark.parametrize("dim", [10, 50])
def test_tables_equal_the_reference_waypoints(golden, dim):
    g = golden("baselines")
    lawn = vb.lawnmower_table(dim, dim, RES, DTB, ALT_LO, ALT_HI, STEP_SIZE, SPACING)
    spiral = vb.spiral_table(dim, dim, RES, DTB, ALT_LO, ALT_HI, NUM_WAYPOINTS, SLOPE)
    assert lawn.dtype == np.float64 and spiral.dtype == np.float64 and spiral.shape == (NUM_WAYPOINTS, 3)
    for uav in ("dist", "time"):
        for cut in ("cut", "all"):
            for name, table in (("lawn", lawn), ("spiral", spiral)):
                want = g[f"{name}_g{dim}_{uav}_{cut}"]
                assert 0 < len(want) <= len(table)
                assert np.array_equal(table[:len(want)], want), (name, uav, cut)  # exactly: the planned prefix
        assert np.array_equal(g[f"lawn_g{dim}_{uav}_all"], lawn) and np.array_equal(g[f"spiral_g{dim}_{uav}_all"], spiral)


@pytest.mark.parametrize("uav", ["dist", "time"])
@pytest.mark.parametrize("name", ["lawn", "spiral"])
def test_table_rules_cut_the_path_where_the_reference_does(golden, name, uav):
    """The per-decision rule on a ledger charged like the env's reproduces create_waypoints followed by execute's break."""
    g = golden("baselines")
    flight = uav == "time"
    table = vb.lawnmower_table(10, 10, RES, DTB, ALT_LO, ALT_HI, STEP_SIZE, SPACING) if name == "lawn" else \
        vb.spiral_table(10, 10, RES, DTB, ALT_LO, ALT_HI, NUM_WAYPOINTS, SLOPE)
    for cut in ("cut", "all"):
        planned, budget = g[f"{name}_g10_{uav}_{cut}"], float(g[f"{name}_g10_{uav}_{cut}_budget"])
        # execute(): the spiral flies all planned waypoints, the lawnmower stops where remaining_budget <= cost
        flown, left, prev = [], budget, INIT
        for w in planned:
            c = float(vb.mission_cost(w, prev, flight, MAX_V, MAX_A))
            if name == "lawn" and left <= c:
                break
            flown.append(w); left -= c; prev = w
        got, left, prev, cursor = [], budget, INIT, 0
        while True:
            has, w = vb.table_next("lawnmower" if name == "lawn" else "spiral", table, cursor, prev, left, STEP_SIZE, flight, MAX_V, MAX_A)
            if not has:
                break
            got.append(w); left -= float(vb.mission_cost(w, prev, flight, MAX_V, MAX_A)); prev = w; cursor += 1
        assert len(got) == len(flown) and np.array_equal(np.array(got), np.array(flown)), (cut, len(got), len(flown))


@pytest.mark.parametrize("dim", [10, 50])
@pytest.mark.parametrize("tag", ["na", "ad"])
def test_random_discrete_replays_the_recorded_draws(golden, dim, tag):
    g = golden("baselines")
    actions = vb.discrete_actions(dim, dim, RES, vb.altitude_linspace(ALT_LO, ALT_HI, SPACING))
    assert actions.shape == (3 * dim * dim, 3)
    for s in range(3):
        rec = {k: g[f"disc_g{dim}_{tag}_s{s}_{k}"] for k in ("prev", "budget", "count", "idx", "way")}
        assert len(rec["way"]) >= 3
        for i in range(len(rec["way"])):
            u = (rec["idx"][i] + 0.5) / rec["count"][i]
            count, k, idx, way, has = vb.random_discrete_next(actions, rec["prev"][i], rec["budget"][i], u, tag == "ad", MAX_V, MAX_A)
            assert has and count == rec["count"][i] and k == rec["idx"][i], (s, i)
            assert np.array_equal(way, rec["way"][i]), (s, i)


@pytest.mark.parametrize("dim", [10, 50])
def test_random_continuous_replays_the_recorded_iterations(golden, dim):
    g = golden("baselines")
    low, high = vb.continuous_box(dim, dim, RES, DTB, ALT_LO, ALT_HI)
    exhausted = 0
    for s in range(3):
        rec = {k: g[f"cont_g{dim}_s{s}_{k}"] for k in ("prev", "budget", "used", "u", "way")}
        pos = 0
        for i in range(len(rec["way"])):
            used = int(rec["used"][i])
            u = np.full((vb.TRIALS, 3), 0.5)
            u[:used] = rec["u"][pos: pos + used]
            pos += used
            t, _, has, chosen = vb.random_continuous_next(rec["prev"][i], rec["budget"][i], u, low, high, True, MAX_V, MAX_A)
            assert t == used - 1, (s, i)
            assert np.array_equal(chosen, rec["way"][i]), (s, i)  # bit for bit
            exhausted += used == vb.TRIALS
            # an iteration that exhausts its trials ends the mission: execute never flies its waypoint (:118)
            assert has == (i < len(rec["way"]) - 1), (s, i)
        assert pos == len(rec["u"])
    assert exhausted >= 3


def test_curves_equal_the_recorded_interp(golden):
    g = golden("baselines")
    xs = [g[f"curve_xs{i}"] for i in range(3)]
    assert sorted(len(x) for x in xs) == [2, 6, 12] and np.any(np.diff(xs[1]) == 0)
    max_x, G = vb.curve_axis(max(x[-1] for x in xs), float(g["curve_budget"]))
    assert np.array_equal(np.linspace(0, max_x, G), g["curve_axis"])
    per_env = np.stack([vb.curve_resample_host(xs[i], g[f"curve_ys{i}"], max_x, G) for i in range(3)])
    for i in range(3):
        assert np.array_equal(per_env[i], g[f"curve_interp{i}"])
    mean, sd = vb.curve_reduce_host(per_env)
    assert np.allclose(mean, per_env.mean(axis=0), rtol=1e-15) and np.allclose(sd, per_env.std(axis=0, ddof=1), rtol=1e-15)
    assert np.array_equal(vb.curve_reduce_host(per_env[:1])[1], np.zeros((G, 8)))


def test_header_and_binding_declare_the_calls():
    from ipp_rl_amd import _ffi
    from ipp_rl_amd.vec_env import philox_uniform

    txt = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    for name in ("ipp_baseline_act", "ipp_curve_record", "ipp_curve_extent", "ipp_curve_resample", "ipp_curve_reduce"):
        assert re.search(rf"\bint {name}\(", txt) and name in _ffi.PROTOTYPES, name
    m = re.search(r"#define\s+IPP_BASELINE_STREAM\s+\((\d+)ull << (\d+)\)", txt)
    assert m and int(m.group(1)) << int(m.group(2)) == _ffi.IPP_BASELINE_STREAM
    streams = [_ffi.IPP_BUDGET_STREAM, _ffi.IPP_CMA_STREAM, _ffi.IPP_SP_ACTION_STREAM, _ffi.IPP_SP_INIT_STREAM, _ffi.IPP_SP_TIE_STREAM,
               _ffi.IPP_SP_ARGMAX_STREAM, _ffi.IPP_REPLAY_STREAM, _ffi.IPP_BASELINE_STREAM]
    assert len(set(streams)) == len(streams)
    assert re.search(r"#define\s+IPP_ABI_VERSION\s+17\b", txt) and _ffi.ABI_VERSION == 17
    for macro, val in (("IPP_BASELINE_TRIALS", _ffi.IPP_BASELINE_TRIALS), ("IPP_CURVE_VALUES", _ffi.IPP_CURVE_VALUES),
                       ("IPP_CURVE_POINT", _ffi.IPP_CURVE_POINT), ("IPP_BASELINE_RANDOM_CONTINUOUS", _ffi.IPP_BASELINE_RANDOM_CONTINUOUS)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", txt).group(1)) == val
    # the struct: same field order as the header
    body = re.search(r"typedef struct ipp_baseline \{(.*?)\} ipp_baseline;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        m = re.match(r"\s*(?:const\s+)?(?:int32_t|int64_t|double|uint64_t|uint8_t)\s*\*?\s*(.*)", stmt, flags=re.S)
        if m and m.group(1).strip():
            names += [n.strip().lstrip("*").split("[")[0].strip() for n in m.group(1).split(",")]
    assert names == [f[0] for f in _ffi.IppBaseline._fields_]
    # the host copy of the device's uniform
    u = vb.baseline_uniform(5, np.arange(4), 3, trial=7, component=2)
    assert np.array_equal(u, philox_uniform(np.arange(4) * 512 + 30, _ffi.IPP_BASELINE_STREAM + 3, 5)) and np.all((u > 0) & (u < 1))
