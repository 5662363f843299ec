"""Hotspot and split ground truths without a GPU: the host copy of the fields (ipp_rl_amd.fields) against the reference's maps
(tests/golden/fields.npz, gen_field_golden.py), the ipp_field_record layout, config parsing, rejections, and the distribution of the
direct second-centre draw against the reference's rejection loop."""
import ctypes as C
import os

import numpy as np
import pytest

from ipp_rl_amd import EngineConfig, _ffi, fields
from tests.params import example_params

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fields.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def fixture_cases(g):
    """(prefix, kind, dim, radius, seed) of every recorded map."""
    out = []
    for key in g.files:
        if key.endswith("_map"):
            prefix, dim, rt, st = key[:-len("_map")].split("_")
            out.append((key[:-len("map")], prefix, int(dim), float(rt[1:].replace("p", ".")), int(st[1:])))
    return out


def record_of(g, key):
    rec = np.zeros((), dtype=fields.RECORD_DTYPE)
    rec["inside"], rec["outside"], rec["rect"] = g[key + "inside"], g[key + "outside"], g[key + "rect"]
    return rec


def test_fixture_covers_kinds_grids_and_radii(golden):
    cases = fixture_cases(golden)
    for prefix in ("hotspot", "split"):
        got = {(d, r) for _, p, d, r, _ in cases if p == prefix}
        assert {d for d, _ in got} == {20, 50, 100}
        assert {r for _, r in got} == {3.0, 5.0, 2.5}
    assert len(cases) == 2 * 3 * 3 * 3


def test_host_fill_reproduces_reference_maps(golden):
    for key, prefix, dim, r, seed in fixture_cases(golden):
        m = fields.fill(record_of(golden, key), dim, dim)
        assert np.array_equal(m, golden[key + "map"]), key


def test_numpy_stream_records_match_reference(golden):
    """The drop-ins' record functions draw with the reference's calls: same record, and the stream is left where the reference left it."""
    for key, prefix, dim, r, seed in fixture_cases(golden):
        np.random.seed(seed)
        rec = fields.hotspot_record_numpy(dim, dim, r) if prefix == "hotspot" else fields.split_record_numpy(dim, dim)
        assert np.random.random() == float(golden[key + "next"]), key
        assert rec["inside"] == golden[key + "inside"] and rec["outside"] == golden[key + "outside"], key
        assert np.array_equal(rec["rect"], golden[key + "rect"]), key


def test_field_record_layout():
    assert C.sizeof(_ffi.IppFieldRecord) == 48 == fields.RECORD_DTYPE.itemsize
    assert _ffi.IppFieldRecord.inside.offset == 0 and _ffi.IppFieldRecord.outside.offset == 8 and _ffi.IppFieldRecord.rect.offset == 16
    assert [fields.RECORD_DTYPE.fields[n][1] for n in ("inside", "outside", "rect")] == [0, 8, 16]
    assert (_ffi.IPP_FIELD_GRF, _ffi.IPP_FIELD_HOTSPOT, _ffi.IPP_FIELD_SPLIT) == (0, 1, 2)
    assert _ffi.ABI_VERSION == 17
    # the record written through ctypes and read through the dtype agree
    r = _ffi.IppFieldRecord(0.75, 0.125)
    for q in range(2):
        for k in range(4):
            r.rect[q][k] = 10 * q + k
    arr = np.frombuffer(bytes(r), dtype=fields.RECORD_DTYPE)[0]
    assert arr["inside"] == 0.75 and arr["outside"] == 0.125 and arr["rect"].tolist() == [[0, 1, 2, 3], [10, 11, 12, 13]]


def test_header_declares_the_field_entries():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "ipp_engine.h")).read()
    for name in ("ipp_generate_field_groups", "ipp_generate_field_refill", "ipp_fill_fields", "ipp_field_record"):
        assert name in hdr
    assert "#define IPP_ABI_VERSION 17" in hdr
    for name in ("ipp_generate_field_groups", "ipp_generate_field_refill", "ipp_fill_fields"):
        assert name in _ffi.PROTOTYPES


def test_from_params_reads_the_simulation_type():
    p = example_params(20)
    assert EngineConfig.from_params(p).simulation == "gaussian_random_field"
    for t in ("hotspot_random_field", "split_random_field", "temperature_data_field"):
        p["sensor"]["simulation"]["type"] = t
        assert EngineConfig.from_params(p).simulation == t
    del p["sensor"]["simulation"]["type"]
    assert EngineConfig.from_params(p).simulation == "gaussian_random_field"


def test_kinds_and_rejections():
    assert fields.field_kind("gaussian_random_field") == _ffi.IPP_FIELD_GRF
    assert fields.field_kind("hotspot_random_field") == _ffi.IPP_FIELD_HOTSPOT
    assert fields.field_kind("split_random_field") == _ffi.IPP_FIELD_SPLIT
    with pytest.raises(ValueError, match="dataset"):
        fields.field_kind("temperature_data_field")
    with pytest.raises(ValueError, match="unknown"):
        fields.field_kind("perlin_noise_field")
    # the reference's rejection loop hangs (a first centre leaves no admissible second one) or its randint raises
    for dims, r in (((10, 10), 5), ((10, 10), 10), ((20, 20), 25), ((7, 7), 2.5), ((20, 9), 4), ((20, 20), -1.0)):
        with pytest.raises(ValueError):
            fields.check_hotspot(*dims, r)
        with pytest.raises(ValueError):
            fields.draw_records(_ffi.IPP_FIELD_HOTSPOT, *dims, r, np.arange(4), 0, 1)
    np.random.seed(0)
    st = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        fields.hotspot_record_numpy(10, 10, 5)
    assert np.array_equal(np.random.get_state()[1], st)  # (rejected before any draw)
    for dims, r in (((10, 10), 2), ((20, 20), 5), ((50, 50), 2.5), ((40, 40), 5), ((20, 9), 2)):
        fields.check_hotspot(*dims, r)
    # accepted exactly where every first centre has a second one more than r away (brute force over the pairs)
    for dim in range(1, 31):
        for r in (0.0, 1.0, 2.0, 2.5, 3.0, 4.5, 5.0, 7.0):
            lo = int(r)
            ends = lo < dim and all(any(abs(c2 - c) > r for c2 in range(lo, dim)) for c in range(lo, dim))
            try:
                fields.check_hotspot(dim, dim, r)
                ok = True
            except ValueError:
                ok = False
            assert ok == ends, (dim, r)


def test_vec_env_rejects_unsupported_kinds_before_the_engine():
    pytest.importorskip("torch")
    from ipp_rl_amd.vec_env import VecIPPEnv

    for sim, dims, r in (("temperature_data_field", 20, 5.0), ("nonsense", 20, 5.0), ("hotspot_random_field", 10, 5.0)):
        cfg = EngineConfig(x_dim=dims, y_dim=dims, simulation=sim, cluster_radius=r)
        with pytest.raises(ValueError):
            VecIPPEnv(cfg, 8, episode_steps=4, device="cpu")


def test_host_draws_stay_in_the_reference_ranges():
    rows = np.arange(20000)
    for dim, r in ((20, 3.0), (50, 5.0), (40, 2.5), (23, 5.0)):
        rec = fields.draw_records(_ffi.IPP_FIELD_HOTSPOT, dim, dim, r, rows, 1 << 40, 9)
        assert np.all((rec["inside"] >= 0.7) & (rec["inside"] <= 1.0) & (rec["outside"] >= 0.0) & (rec["outside"] <= 0.3))
        lo = int(r)
        for q in range(2):
            for a in (0, 2):
                y0, y1 = rec["rect"][:, q, a], rec["rect"][:, q, a + 1]
                assert np.all((y0 >= 0) & (y0 < y1) & (y1 <= dim))
        rec = fields.draw_records(_ffi.IPP_FIELD_SPLIT, dim, dim, r, rows, 1 << 40, 9)
        ysplit = rec["rect"][:, 0, 3] == dim
        s = np.where(ysplit, rec["rect"][:, 0, 1], rec["rect"][:, 0, 3])
        assert np.all(np.where(ysplit, (s >= np.ceil(dim * 0.33)) & (s <= np.ceil(dim * 0.66)),
                               (s >= np.floor(dim * 0.33)) & (s <= np.ceil(dim * 0.66))))
        assert np.all(np.abs(rec["inside"] - rec["outside"]) > 0.3)


@pytest.mark.parametrize("dim,r", [(20, 5.0), (12, 2.5)])
def test_direct_second_centre_matches_the_rejection_loop(dim, r):
    """The joint law of (first centre, second centre) on each axis: direct draw (draw_records) vs the reference's loop over pairs
    (both axes redrawn until |dy| > r and |dx| > r), on host uniforms.  Every cell of the (c, c2) table within 5 sigma."""
    n = 200_000
    lo = int(r)
    rec = fields.draw_records(_ffi.IPP_FIELD_HOTSPOT, dim, dim, r, np.arange(n), 5, 3)
    rs = np.random.RandomState(1)
    yc = lo + rs.randint(0, dim - lo, n)
    xc = lo + rs.randint(0, dim - lo, n)
    y2, x2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    todo = np.arange(n)
    while len(todo):
        ty, tx = lo + rs.randint(0, dim - lo, len(todo)), lo + rs.randint(0, dim - lo, len(todo))
        ok = (np.abs(ty - yc[todo]) > r) & (np.abs(tx - xc[todo]) > r)
        y2[todo[ok]], x2[todo[ok]] = ty[ok], tx[ok]
        todo = todo[~ok]

    # (a centre is ambiguous from its cluster's bounds at the edges: the tables count the bounds themselves)
    for axis, (c, c2) in enumerate(((yc, y2), (xc, x2))):
        b0 = np.trunc(np.maximum(c - r, 0)).astype(np.int64), np.trunc(np.minimum(c + r, dim)).astype(np.int64)
        b2 = np.trunc(np.maximum(c2 - r, 0)).astype(np.int64), np.trunc(np.minimum(c2 + r, dim)).astype(np.int64)
        brute = np.bincount(((b0[0] * dim + b0[1]) * dim + b2[0]) * dim + b2[1], minlength=dim ** 4)
        R = rec["rect"]
        direct = np.bincount(((R[:, 0, 2 * axis] * dim + R[:, 0, 2 * axis + 1]) * dim + R[:, 1, 2 * axis]) * dim + R[:, 1, 2 * axis + 1],
                             minlength=dim ** 4)
        assert np.array_equal(brute > 0, direct > 0)  # the same support
        assert np.all(np.abs(brute - direct) <= 5 * np.sqrt(brute + direct) + 2)
