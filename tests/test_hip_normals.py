"""
The device's normals (philox_normal4, csrc/ipp_common.h: Philox4x32-10, then Box-Muller through the hardware log / sin / cos) element by
element against the fp64 restatement of their definition on the host (vec_env.philox_normal4_ref; its Philox words are pinned to the
Random123 known answers in tests/test_normals_host.py): the flat fill, the row-keyed fill (counter = (row id + offset) * ceil(row_len / 4)
+ c // 4, element c % 4, plane p in subsequence subseq0 + p), every high word of counter, subsequence and seed, and the words at which
the fast transcendentals are weakest (u next to 0 and 1, the angle next to the zeros of sine and cosine).

BOUND: |device - fp64 reference| of one normal.  Measured maximum over all the cases of this file on an MI355X: MEASURED = 1.738e-6, in
the 2^20 bulk draws (the RATIO lines print it per case; the extreme words stay below 6e-7).  The bound is twice that, rounded up to a
power of two (other inputs may land on worse roundings of the same instructions): 2^-18 = 3.8e-6.  It has to stay below the project's
parity bar of 1e-5 for whatever feeds a ground truth (tests/test_normals_host.py checks this arithmetic without a GPU).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MEASURED = 1.738e-06
BOUND = 2.0 ** -18
SEED = (0x9E3779B9 << 32) | 5
SUB = (1 << 40) + 9
ROW_IDS = [5, 0, 7, 3, 3]

# Counters of (SEED, SUB) whose Philox words fall into the extreme bins, found by scanning counters 0 .. 2^24 on the host with philox_words
# (the three-quarters bin has one hit there: its other four come from going on to 2^26); test_extreme_words recomputes the words and
# asserts the bins.
EXTREME = {
    "low": [758164, 2584805, 4035594, 12173438, 14290634, 3205438, 10752603, 11994010, 1197679, 14575996],   # some word < 512
    "high": [1825938, 6516079, 15253294, 2467467, 5234116, 6701745, 15220892],                               # some word >= 2^32 - 512
    "quarter": [4626127, 5961157, 13906517, 14358694],                                                       # word 1 within 512 of 2^30
    "half": [1011021, 2444070, 8828454, 13138113],                                                           # ... of 2^31
    "three_quarters": [12480943, 16959586, 18420528, 20568930, 26461088],                                    # ... of 3 2^30
}


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def eng():
    from ipp_rl_amd import EngineConfig, IPPEngine

    e = IPPEngine(EngineConfig(x_dim=10, y_dim=10), capacity=2, state="factor", rank_cap=16)
    yield e
    e.close()


def check(what, dev, ref):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    assert np.all(np.isfinite(dev)), what
    err = float(np.max(np.abs(dev - ref)))
    print(f"RATIO {what}: max |device - fp64| {err:.3e} = {err / BOUND:.3f} of the bound {BOUND:.3e}")
    assert err <= BOUND, (what, err, int(np.argmax(np.abs(dev - ref).ravel())))


def flat_ref(count, seed, sub):
    from ipp_rl_amd.vec_env import philox_normal4_ref

    return philox_normal4_ref(np.arange((count + 3) // 4), sub, seed).ravel()[:count]


def test_fill_normal_high_words(eng):
    """count = 4099: the last counter is partial (3 of its 4 normals).  Seed and subsequence with non-zero high words; then three more
    fills with one high word changed each: the seed's, the subsequence's and the counter's.  A flat fill always starts at counter 0 and
    would need 2^34 elements to reach the counter's high word, so that one goes through the row-keyed fill with row_len 4 (counter = row
    id + offset) and an offset of 2^32; a fourth flat fill strips both other high words at once."""
    count = 4099
    base = host(eng.normal(count, seed=SEED, subsequence=SUB))
    check("fill_normal 4099", base, flat_ref(count, SEED, SUB))
    for what, seed, sub in (("seed high word", SEED ^ (1 << 32), SUB), ("subsequence high word", SEED, SUB ^ (1 << 40)),
                            ("seed and subsequence low words only", SEED & 0xFFFFFFFF, SUB & 0xFFFFFFFF)):
        out = host(eng.normal(count, seed=seed, subsequence=sub))
        assert not np.array_equal(out, base), what
        assert np.max(np.abs(out - base)) > 1.0, what  # (another stream, not a perturbation)
        check(f"fill_normal 4099, {what} changed", out, flat_ref(count, seed, sub))
    # the counter's high word, third of the three: counters q and q + 2^32 through the row-keyed fill with row_len 4 (counter = row id + offset)
    import torch
    from ipp_rl_amd.vec_env import philox_normal_rows_ref

    lo = torch.empty((1, 1025, 4), dtype=torch.float32, device="cuda")
    hi = torch.empty_like(lo)
    eng.normal_rows(lo, 4, SEED, SUB, row_offset=0)
    eng.normal_rows(hi, 4, SEED, SUB, row_offset=1 << 32)
    assert np.array_equal(host(lo).ravel()[:4099], base)
    assert np.max(np.abs(host(hi) - host(lo))) > 1.0
    check("fill_normal_rows, counter high word changed", host(hi), philox_normal_rows_ref(1, range(1025), 4, SEED, SUB, 1 << 32))


@pytest.mark.parametrize("row_len", [1, 4, 9, 10])
def test_fill_normal_rows(eng, row_len):
    """row_len 9 is the measurement-noise row; 10 and 1 end in a partial counter.  Offsets: none, an ordinary one, one that carries
    counter = (row id + offset) * qpr across 2^32 for every row_len with qpr = 3 (row_len 9, 10), and one that puts the counter above 2^40."""
    import torch
    from ipp_rl_amd.vec_env import philox_normal_rows_ref

    ids = torch.tensor(ROW_IDS, dtype=torch.int32, device="cuda")
    for off in (0, 123456789, 1500000000, (1 << 41) + 3):
        out = torch.full((3, 5, row_len), float("nan"), dtype=torch.float32, device="cuda")
        eng.normal_rows(out, row_len, SEED, SUB, row_ids=ids, row_offset=off)
        out = host(out)
        check(f"fill_normal_rows row_len {row_len} offset {off}", out, philox_normal_rows_ref(3, ROW_IDS, row_len, SEED, SUB, off))
        assert np.array_equal(out[:, 3], out[:, 4]) and not np.array_equal(out[:, 0], out[:, 1])  # rows 3 and 4 share an id
        for p in range(3):  # plane p is plane 0 of subsequence SUB + p
            one = torch.empty((5, row_len), dtype=torch.float32, device="cuda")
            eng.normal_rows(one, row_len, SEED, SUB + p, row_ids=ids, row_offset=off)
            assert np.array_equal(host(one), out[p]), (off, p)
    # no row ids: row j is row id j
    out = torch.empty((2, 8, row_len), dtype=torch.float32, device="cuda")
    eng.normal_rows(out, row_len, SEED, SUB, row_offset=1500000000)
    check(f"fill_normal_rows row_len {row_len}, no ids", host(out), philox_normal_rows_ref(2, range(8), row_len, SEED, SUB, 1500000000))


def test_extreme_words(eng):
    """Box-Muller's tails: u0 next to 0 (largest radius) and next to or equal to 1 (radius 0: the log next to its zero), the angle next to
    0, 1/4, 1/2, 3/4 and 1 revolution (the zeros of sine and cosine).  Random sampling does not land there; these counters do."""
    import torch
    from ipp_rl_amd.vec_env import philox_normal_rows_ref, philox_words

    counters = []
    for name, qs in EXTREME.items():
        w = np.stack([x.astype(np.int64) for x in philox_words(np.array(qs, dtype=np.uint64), SUB, SEED)], axis=1)  # [len, 4]
        in_bin = {"low": (w < 512).any(axis=1), "high": (w >= 2 ** 32 - 512).any(axis=1), "quarter": np.abs(w[:, 1] - 2 ** 30) <= 512,
                  "half": np.abs(w[:, 1] - 2 ** 31) <= 512, "three_quarters": np.abs(w[:, 1] - 3 * 2 ** 30) <= 512}[name]
        assert in_bin.all() and max(qs) < 1 << 26, (name, w)
        counters += qs
    wall = np.stack([x.astype(np.int64) for x in philox_words(np.array(counters, dtype=np.uint64), SUB, SEED)], axis=1)
    # every word position is hit at both ends: radius words (0, 2) and angle words (1, 3)
    assert (wall[:, [0, 2]] < 512).any() and (wall[:, [1, 3]] < 512).any()
    assert (wall[:, [0, 2]] >= 2 ** 32 - 512).any() and (wall[:, [1, 3]] >= 2 ** 32 - 512).any()
    ids = torch.tensor(counters, dtype=torch.int32, device="cuda")
    out = torch.full((1, len(counters), 4), float("nan"), dtype=torch.float32, device="cuda")
    eng.normal_rows(out, 4, SEED, SUB, row_ids=ids, row_offset=0)  # row_len 4: one counter per row, counter = row id
    out = host(out)[0]
    ref = philox_normal_rows_ref(1, counters, 4, SEED, SUB)[0]
    for name, qs in EXTREME.items():
        sel = [counters.index(q) for q in qs]
        check(f"extreme words, {name}", out[sel], ref[sel])
    # u0 = 1.0 (float32 rounds a word >= 2^32 - 128 to 2^32): log 1 = 0, both elements of the pair exactly 0
    u = (wall.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    ones = np.argwhere(u[:, [0, 2]] == np.float32(1.0))
    assert len(ones) >= 1
    for row, h in ones:
        assert out[row, 2 * h] == 0.0 and out[row, 2 * h + 1] == 0.0, (counters[row], out[row])
        assert ref[row, 2 * h] == 0.0 and ref[row, 2 * h + 1] == 0.0


def test_bulk(eng):
    count = 1 << 20
    out = host(eng.normal(count, seed=SEED, subsequence=SUB))
    check("fill_normal 2^20", out, flat_ref(count, SEED, SUB))
