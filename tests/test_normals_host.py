"""
CPU tests of the host reference of the device's normals (ipp_rl_amd/vec_env.py: philox_words, philox_normal4_ref,
philox_normal_rows_ref -- what tests/test_hip_normals.py and the drawn-noise case of tests/test_hip_big_grids.py compare the device
with): all four Philox4x32-10 output words against the published Random123 known answers, philox_uniform unchanged bit for bit by
the refactoring, the reference normals' moments and its row-keyed addressing.
"""
import numpy as np


def _frozen_philox_uniform(counter, subsequence, seed):
    """philox_uniform as it was before philox_words was factored out of it (frozen copy: the budget draws must not move)."""
    m32 = np.uint64(0xFFFFFFFF)
    q = np.asarray(counter, dtype=np.int64).astype(np.uint64)
    sub = np.asarray(subsequence, dtype=np.int64).astype(np.uint64)
    q, sub = np.broadcast_arrays(q, sub)
    c = [q & m32, q >> np.uint64(32), sub & m32, sub >> np.uint64(32)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = np.uint64(0xD2511F53) * c[0]
            p1 = np.uint64(0xCD9E8D57) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
            k0 = (k0 + np.uint64(0x9E3779B9)) & m32
            k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return (c[0].astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


# Random123 kat_vectors, philox4x32 10: counter words c0..c3, key words k0 k1 -> output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_words_known_answers():
    from ipp_rl_amd.vec_env import philox_uniform, philox_words

    for c, k, want in KAT:
        counter, sub, seed = c[0] | (c[1] << 32), c[2] | (c[3] << 32), k[0] | (k[1] << 32)
        got = philox_words(counter, sub, seed)
        assert len(got) == 4 and all(w.dtype == np.uint64 for w in got)
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]
        # high counter / subsequence bits as an array, too (the vectorised form the GPU tests use)
        got = philox_words(np.array([counter], dtype=np.uint64), np.array([sub], dtype=np.uint64), seed)
        assert tuple(int(w[0]) for w in got) == want
    # the first word of the first two is what tests/test_budget_host.py asserts of philox_uniform
    assert philox_uniform(0, 0, 0) == (KAT[0][2][0] + 0.5) / 2 ** 32
    assert philox_uniform(-1, -1, 2 ** 64 - 1) == (KAT[1][2][0] + 0.5) / 2 ** 32
    assert tuple(int(w) for w in philox_words(-1, -1, 2 ** 64 - 1)) == KAT[1][2]


def test_philox_uniform_unchanged_bit_for_bit():
    from ipp_rl_amd.vec_env import philox_uniform

    rs = np.random.RandomState(0)
    for seed in (0, 7, (0x9E3779B9 << 32) | 5, 2 ** 64 - 1):
        counter = rs.randint(-2 ** 62, 2 ** 62, size=4000, dtype=np.int64)
        sub = rs.randint(-2 ** 62, 2 ** 62, size=4000, dtype=np.int64)
        assert np.array_equal(philox_uniform(counter, sub, seed), _frozen_philox_uniform(counter, sub, seed))
        # broadcast forms of start_budget: ids against one stream, Python ints
        assert np.array_equal(philox_uniform(np.arange(1000), (1 << 42) + 3, seed), _frozen_philox_uniform(np.arange(1000), (1 << 42) + 3, seed))
        assert philox_uniform(5, 9, seed) == _frozen_philox_uniform(5, 9, seed)


def test_reference_normals_are_standard_and_keyed():
    from ipp_rl_amd.vec_env import philox_normal4_ref, philox_words

    n = 1 << 18  # x 4 = 2^20 draws
    x = philox_normal4_ref(np.arange(n), 2, 5)
    assert x.shape == (n, 4) and x.dtype == np.float64 and np.all(np.isfinite(x))
    flat = x.ravel()
    # standard errors at 2^20 draws: mean 1e-3, std 7e-4, kurtosis 4.8e-3
    assert abs(flat.mean()) < 5e-3 and abs(flat.std() - 1.0) < 5e-3 and abs(np.mean(flat ** 4) - 3.0) < 0.03
    for e in range(4):  # ... and of every element on its own (a pair that reused a word would still be standard as a whole)
        assert abs(x[:, e].mean()) < 1e-2 and abs(x[:, e].std() - 1.0) < 1e-2
    c = np.corrcoef(x.T)
    assert np.max(np.abs(c - np.eye(4))) < 1e-2
    # the definition, element by element, on one counter with high words everywhere
    q, sub, seed = (3 << 40) + 17, (1 << 40) + 9, (0x9E3779B9 << 32) | 5
    w = [int(v) for v in philox_words(q, sub, seed)]
    u = [float(np.float32(np.float32(v) + np.float32(0.5)) * np.float32(2.0 ** -32)) for v in w]
    want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
            np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])]
    assert np.allclose(philox_normal4_ref(q, sub, seed), want, rtol=0, atol=1e-15)
    # every high word is part of the key
    base = philox_normal4_ref(np.arange(8), sub, seed)
    assert not np.array_equal(philox_normal4_ref(np.arange(8) + (1 << 32), sub, seed), base)
    assert not np.array_equal(philox_normal4_ref(np.arange(8), sub ^ (1 << 40), seed), base)
    assert not np.array_equal(philox_normal4_ref(np.arange(8), sub, seed ^ (1 << 32)), base)
    # a word of 2^32 - 1 rounds to u = 1 in float32: radius exactly 0
    assert float(np.float32(np.float32(2 ** 32 - 1) + np.float32(0.5)) * np.float32(2.0 ** -32)) == 1.0


def test_row_keyed_addressing():
    from ipp_rl_amd.vec_env import philox_normal4_ref, philox_normal_rows_ref

    seed, sub = (0x9E3779B9 << 32) | 5, (1 << 40) + 9
    ids = [5, 0, 7, 3, 3]
    for row_len in (1, 4, 9, 10):
        qpr = (row_len + 3) // 4
        for off in (0, 123456789, 1500000000, 1 << 41):
            out = philox_normal_rows_ref(3, ids, row_len, seed, sub, off)
            assert out.shape == (3, 5, row_len)
            assert np.array_equal(out[:, 3], out[:, 4]) and not np.array_equal(out[:, 0], out[:, 1])
            for p in range(3):
                for j, rid in enumerate(ids):
                    for c in (0, row_len - 1):
                        want = philox_normal4_ref((rid + off) * qpr + c // 4, sub + p, seed)[c % 4]
                        assert out[p, j, c] == want
    # row_len 9, offset 1.5e9: the counter (not the row id) crosses 2^32
    assert (7 + 1500000000) < 2 ** 32 <= (7 + 1500000000) * 3


def test_device_bound_is_twice_the_measurement_and_below_the_bar():
    """The constants of tests/test_hip_normals.py: BOUND is 2 x MEASURED rounded up to a power of two, at most the 1e-5 parity bar."""
    from tests.test_hip_normals import BOUND, MEASURED

    assert MEASURED > 0.0 and 2.0 * MEASURED <= BOUND < 4.0 * MEASURED and BOUND <= 1e-5
    assert np.log2(BOUND) == round(np.log2(BOUND))
