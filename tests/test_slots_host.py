"""
CPU tests of the packed slot record (ipp-rl_amd/slots.py: the NumPy definition of the format of ipp_slots_export / ipp_slots_import,
include/ipp_engine.h "Slot export and import") and of the compact ring's archive-slot set (selfplay.archive_slots_in_use):
  * unpack(pack(x)) == x bit for bit for random raw arrays, N = 225 (no multiple of 4) and N = 400, ranks 0, 1 and rank_cap, every
    selection of sections;
  * the offsets are the exclusive scan of the documented record sizes, every part starts on a 16-byte boundary, padding is zero;
  * malformed records are refused; layouts are compared field by field;
  * archive_slots_in_use against a brute-force loop, episode counters below, equal to and above E.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_CAP = 27
PSTRIDE = {225: 112, 400: 208}  # floats per stored column: a multiple of 16


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def random_slot(rs, rank, N, pstride):
    """Raw arrays with every bit pattern in play: NaNs and infinities included."""
    def f32(n):
        return rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)

    return dict(rank=rank, prior=rs.uniform(0.5, 4.0, size=2), colspan=rs.randint(-2 ** 31, 2 ** 31, size=rank).astype(np.int32),
                colrect=rs.randint(-2 ** 31, 2 ** 31, size=rank).astype(np.int32), columns=f32(rank * pstride).reshape(rank, pstride),
                mean=f32(N), diag=f32(N), gt=f32(N))


def documented_bytes(what, rank, N, pstride):
    """The table of include/ipp_engine.h, written out."""
    pad = lambda b: (b + 15) // 16 * 16  # noqa: E731
    size = 32
    if what & 1:
        size += 16 + pad(4 * rank) + pad(4 * rank) + 4 * rank * pstride
    if what & 2:
        size += 3 * pad(4 * N)
    return size


@pytest.mark.parametrize("N", [225, 400])
@pytest.mark.parametrize("what", [1, 2, 3])
def test_round_trip_offsets_and_alignment(N, what):
    from ipp_rl_amd import slots as sl

    ps = PSTRIDE[N]
    rs = np.random.RandomState(100 * N + what)
    ranks = [0, 1, RANK_CAP, 5, 0, RANK_CAP]
    slots = [random_slot(rs, r, N, ps) for r in ranks]
    blob, offsets = sl.pack_slots_host(slots, what, N, ps)
    assert blob.dtype == np.uint8 and offsets.dtype == np.int64 and len(offsets) == len(slots) + 1
    sizes = [documented_bytes(what, r if what & 1 else 0, N, ps) for r in ranks]
    assert offsets.tolist() == [0] + np.cumsum(sizes).tolist() and len(blob) == offsets[-1]
    assert [sl.record_bytes(what, r, N, ps) for r in ranks] == sizes
    covered = np.zeros(len(blob), dtype=bool)
    for s, r, o in zip(slots, ranks, offsets[:-1]):
        r = r if what & 1 else 0
        off = sl.section_offsets(what, r, N, ps)
        assert all((o + v) % 16 == 0 for v in off.values()), off
        h = sl.read_header(blob, o)
        assert h == dict(magic=sl.SLOT_MAGIC, format=sl.SLOT_FORMAT, what=what, rank=r, bytes=off["end"], N=N, pstride=ps)
        covered[o:o + 32] = True
        lens = dict(prior=16, colspan=4 * r, colrect=4 * r, columns=4 * r * ps, mean=4 * N, diag=4 * N, gt=4 * N)
        for name, at in off.items():
            if name in lens:
                assert np.array_equal(blob[o + at:o + at + lens[name]], bits(s[name])), name
                covered[o + at:o + at + lens[name]] = True
    assert not blob[~covered].any()  # (padding is zero)
    back = sl.unpack_slots_host(blob, offsets, what)
    assert len(back) == len(slots)
    for s, b, r in zip(slots, back, ranks):
        assert b["what"] == what and b["N"] == N and b["pstride"] == ps and b["rank"] == (r if what & 1 else 0)
        names = (("prior", "colspan", "colrect", "columns") if what & 1 else ()) + (("mean", "diag", "gt") if what & 2 else ())
        assert set(b) == {"what", "rank", "N", "pstride", *names}
        for name in names:
            assert b[name].dtype == np.asarray(s[name]).dtype and b[name].shape == np.asarray(s[name]).shape, name
            assert np.array_equal(bits(b[name]), bits(s[name])), name
    again, offs2 = sl.pack_slots_host(back, what, N, ps)
    assert np.array_equal(again, blob) and np.array_equal(offs2, offsets)


def test_malformed_records_and_layouts_are_refused():
    from ipp_rl_amd import slots as sl

    N, ps = 225, 112
    rs = np.random.RandomState(7)
    blob, offsets = sl.pack_slots_host([random_slot(rs, 3, N, ps), random_slot(rs, 1, N, ps)], 3, N, ps)
    for w in (0, 4, 7):
        with pytest.raises(ValueError, match="what"):
            sl.pack_slots_host([], w, N, ps)
    with pytest.raises(ValueError, match="what"):
        sl.unpack_slots_host(blob, offsets, 1)
    bad = blob.copy()
    bad[0] ^= 1  # the magic
    with pytest.raises(ValueError, match="magic"):
        sl.unpack_slots_host(bad, offsets)
    bad = blob.copy()
    bad[12] = 2  # the first record's rank: its size no longer fits
    with pytest.raises(ValueError, match="rank 2"):
        sl.unpack_slots_host(bad, offsets)
    with pytest.raises(ValueError, match="offsets"):
        sl.unpack_slots_host(blob, offsets + 8)
    with pytest.raises(ValueError, match="values"):
        sl.pack_slots_host([dict(random_slot(rs, 2, N, ps), colspan=np.zeros(3, np.int32))], 1, N, ps)
    lay = dict(format=1, W=20, H=20, N=400, Npad=448, pw=16, ph=13, pstride=208, window_rows=10, tile_cells=128, prior_kind=0)
    sl.check_layouts(lay, dict(lay))
    with pytest.raises(ValueError, match="window_rows = 12"):
        sl.check_layouts(lay, dict(lay, window_rows=12))
    with pytest.raises(ValueError, match="format version"):
        sl.check_layouts(lay, dict(lay, format=2, W=40))  # (the version is named first)


def test_the_calls_refuse_a_null_engine_without_a_device():
    """The slot unit reports through the library's one error slot, before any device call; the binding's constants are the format's."""
    import ctypes

    from ipp_rl_amd import _ffi
    from ipp_rl_amd import slots as sl

    lib = _ffi.load()
    lay = _ffi.IppSlotLayout()
    assert lib.ipp_slots_layout(None, ctypes.byref(lay)) == -1 and lib.ipp_last_error() == b"ipp_slots_layout: null argument"
    assert lib.ipp_slots_plan(None, None, 0, 3, None, None, None) == -1 and lib.ipp_last_error() == b"ipp_slots_plan: null engine"
    assert lib.ipp_slots_export(None, None, 0, 3, None, None, None) == -1 and lib.ipp_last_error() == b"ipp_slots_export: null engine"
    assert lib.ipp_slots_import(None, None, 0, 3, None, None, None, None) == -1 and lib.ipp_last_error() == b"ipp_slots_import: null engine"
    assert (sl.SLOT_COLUMNS, sl.SLOT_MAPS) == (_ffi.IPP_SLOT_COLUMNS, _ffi.IPP_SLOT_MAPS)
    assert (sl.SLOT_OK, sl.SLOT_BAD_ID, sl.SLOT_RANK, sl.SLOT_BAD_RECORD) == (_ffi.IPP_SLOT_OK, _ffi.IPP_SLOT_BAD_ID, _ffi.IPP_SLOT_RANK,
                                                                            _ffi.IPP_SLOT_BAD_RECORD)
    assert tuple(f[0] for f in _ffi.IppSlotLayout._fields_) == sl.LAYOUT_FIELDS + ("reserved",) and ctypes.sizeof(_ffi.IppSlotLayout) == 48
    header = open(os.path.join(ROOT, "include", "ipp_engine.h")).read()
    for macro, val in (("IPP_SLOT_COLUMNS", sl.SLOT_COLUMNS), ("IPP_SLOT_MAPS", sl.SLOT_MAPS), ("IPP_SLOT_FORMAT", sl.SLOT_FORMAT),
                       ("IPP_SLOT_HEADER_BYTES", sl.SLOT_HEADER_BYTES), ("IPP_SLOT_MAGIC", sl.SLOT_MAGIC), ("IPP_SLOT_RANK", sl.SLOT_RANK),
                       ("IPP_SLOT_BAD_RECORD", sl.SLOT_BAD_RECORD)):
        m = re.search(rf"#define\s+{macro}\s+(0x[0-9a-f]+|\d+)", header)
        assert m and int(m.group(1), 0) == val, macro


def test_archive_slots_in_use_against_a_loop():
    from ipp_rl_amd.planning.mcts_zero.selfplay import archive_slot, archive_slots_in_use

    for B, E, episodes in ((3, 2, [0, 1, 2]), (3, 2, [3, 7, 2]), (4, 5, [0, 4, 5, 6]), (1, 1, [0]), (1, 1, [9]), (2, 3, [2, 100])):
        want = [B + e * E + j for e in range(B) for j in range(E) if j < min(E, episodes[e])]
        got = archive_slots_in_use(np.asarray(episodes), B, E)
        assert got.dtype == np.int64 and got.tolist() == want, (B, E, episodes)
        # ... which are the slots of the last min(E, p) ended episodes of each env
        named = sorted(int(archive_slot(B, E, e, p)) for e in range(B) for p in range(max(0, episodes[e] - E), episodes[e]))
        assert named == want
    with pytest.raises(ValueError, match="episode counters"):
        archive_slots_in_use(np.zeros(2), 3, 2)
