"""
GPU parity on grids beyond the golden fixtures' 50x50: the oracle's factor form (P = P0 - U U^T, fp64, pinned
against the dense restatement and the golden vectors in tests/test_oracle_golden.py) scales to N = 14 400, so the
large-grid code paths can be checked cell for cell:
  * N > 12 288: no prior table in LDS (direct sqrt/exp in the base term),
  * many tiles per env, windowed column spans, every streaming kernel (fused, workgroup, wave, exact),
  * GRF: every generator launch_grf can pick (GRF_CASES), impulse orientation, cluster radii, noise drawn in the generator.
"""
import numpy as np
import pytest

from oracle import ipp_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5
UAV = {"max_v": 2.0, "max_a": 2.0}


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make(dim, window_rows, tile_threads, capacity, rank_cap=72):
    from ipp_rl_amd import EngineConfig, IPPEngine

    cfg = EngineConfig(x_dim=dim, y_dim=dim)
    eng = IPPEngine(cfg, capacity=capacity, state="factor", rank_cap=rank_cap, window_rows=window_rows,
                    tile_threads=tile_threads, fixed_prior=window_rows < 0)
    ocfg = orc.OracleConfig(x_dim=dim, y_dim=dim, resolution=cfg.resolution, coeff_a=cfg.coeff_a, coeff_b=cfg.coeff_b)
    return eng, cfg, ocfg


@pytest.mark.parametrize("dim,window_rows,tile_threads", [
    (64, 12, 256), (64, 12, 128), (64, 12, 64), (64, 0, 0),
    (120, 12, 256), (120, 12, 128), (120, 12, 64), (120, 0, 0), (120, 1000, 256),
    (200, 12, 256), (200, 0, 0),  # BASELINE configs[4] grid size
    (100, -1, 256), (100, 0, 0),  # BASELINE configs[2] grid size, whole 16-step episodes (bench window / exact mode)
])
def test_factor_step_vs_oracle_factor_form(dim, window_rows, tile_threads):
    """B envs x 6 steps (100x100: a whole 16-step episode of configs[2]) with clustered revisits (so that stored columns
    are streamed on the footprint tiles), all altitude classes, border footprints; reward / mean / diag against the fp64
    factor-form oracle."""
    B, steps = 3, (16 if dim == 100 else 6)
    eng, cfg, ocfg = make(dim, window_rows, tile_threads, B, rank_cap=9 * steps + 18)
    rs = np.random.RandomState(100 + dim)
    gts = rs.uniform(0.0, 1.0, size=(B, dim, dim))
    eng.reset(gt=gts)
    fss = [orc.factor_reset(ocfg) for _ in range(B)]
    prev = np.tile(np.array([2.0, 2.0, 14.0]), (B, 1))
    res = cfg.resolution
    centres = rs.randint(3, dim - 3, size=(B, 2))
    centres[0] = (0, dim - 1)  # env 0 works in a corner: clipped footprints
    worst = 0.0
    for t in range(steps):
        acts = np.empty((B, 3))
        for b in range(B):
            col = np.clip(centres[b, 0] + rs.randint(-2, 3), 0, dim - 1)
            row = np.clip(centres[b, 1] + rs.randint(-2, 3), 0, dim - 1)
            acts[b] = (res * col + 0.5 * res, res * row + 0.5 * res, [5.0, 8.0, 12.0, 14.0, 9.0, 14.0][(t + b) % 6])
        eps = rs.normal(size=(B, 9))
        reward, status = eng.step(acts, prev, meas_noise=eps)
        assert int(status.abs().sum()) == 0
        for b in range(B):
            fs = fss[b]
            m = orc.num_measurements(orc.project_fov(ocfg, acts[b]), orc.resolution_factor(acts[b]))
            z = orc.observe(ocfg, gts[b], acts[b], eps[b, :m])
            mask = orc.adaptive_mask(fs.mean, fs.diag, 0.4, 0.0)
            diag_before = fs.diag.copy()
            orc.factor_step(ocfg, fs, acts[b], z=z)
            want = orc.reward_from_diags(diag_before, fs.diag, acts[b], prev[b], UAV, mask)
            worst = max(worst, abs(float(reward[b]) - want))
            assert abs(float(reward[b]) - want) < TOL, (t, b, float(reward[b]), want)
        prev = acts
    for b in range(B):
        assert np.max(np.abs(host(eng.read_mean(b)).ravel() - fss[b].mean)) < TOL
        assert np.max(np.abs(host(eng.read_diag(b)).ravel() - fss[b].diag)) < TOL
        assert eng.rank(b) == fss[b].U.shape[1]
    print(f"[{dim}x{dim}, window {window_rows}, T={tile_threads}] worst reward error {worst:.2e}")


# Which generator launch_grf (csrc/ipp_engine.hip) picks, derived from its dispatch; TT = ceil(n / 16), np = 16 TT the padded size.
#   default engine, even n <= 128: k_grf_hartley<TT, NW> (NW = 8 for TT 5..7, else 4); n = 50 / 100: k_grf_fft<5> / <10> instead;
#   even 130 <= n <= 256: k_grf_dft, 1024 threads, XB = 4 columns per thread if n % 4 == 0 else 2, rows per thread
#     = ceil(n / (1024 / (n / XB))): <10,4,1024> (rows <= 10), <16,4,1024>, <20,2,1024> (rows <= 20), <32,2,1024>;
#   n = 258 and odd n: k_grf_conv<5 if n <= 64 else 8, tables in LDS if 12 n^2 <= 120 KiB>.
#   IPP_GRF_FFT=0: n = 50 / 100 take the GEMM form with the contracted K: k_grf_hartley<4,4,13> / <7,8,25> (KS = ceil(n / 4) < 4 TT).
#   IPP_GRF_HARTLEY=0: even n <= 128 run k_grf_dft; n <= 100: 256 threads, white noise in LDS (WLDS), rows = ceil(n / (256 / (n / XB))):
#     XB = 4 -> <10,4,256,true>; XB = 2: rows <= 10 -> <10,2,256,true>, else <20,2,256,true>.
DEFAULT, NO_FFT, NO_HARTLEY = {}, {"IPP_GRF_FFT": "0"}, {"IPP_GRF_HARTLEY": "0"}


def expected_generator(n, switches):
    """(kind, param) ipp_grf_generator must report: the family the comments of GRF_CASES derive, and its TT or grf_kc."""
    from ipp_rl_amd import _ffi

    if n % 2 or n > 256:
        return _ffi.IPP_GRF_GEN_CONV, 0
    if n > 128 or switches == NO_HARTLEY:
        budget, fixed = (32768 if n <= 64 else 65536), (4 * n * n if n <= 100 else 0) + 16 * n + 256
        return _ffi.IPP_GRF_GEN_DFT, max(1, min(n // 2 + 1, (budget - fixed) // (40 * n)))
    return (_ffi.IPP_GRF_GEN_FFT if n in (50, 100) and switches == DEFAULT else _ffi.IPP_GRF_GEN_HARTLEY), (n + 15) // 16

GRF_CASES = [
    (4, DEFAULT),     # k_grf_hartley<1,4>, smallest accepted even size (np 16)
    (10, DEFAULT),    # k_grf_hartley<1,4>
    (16, DEFAULT),    # k_grf_hartley<1,4>, n = np: no zero padding
    (18, DEFAULT),    # k_grf_hartley<2,4>
    (32, DEFAULT),    # k_grf_hartley<2,4>, no padding
    (36, DEFAULT),    # k_grf_hartley<3,4>
    (50, DEFAULT),    # k_grf_fft<5, float>
    (64, DEFAULT),    # k_grf_hartley<4,4>, no padding
    (74, DEFAULT),    # k_grf_hartley<5,8>
    (82, DEFAULT),    # k_grf_hartley<6,8>
    (96, DEFAULT),    # k_grf_hartley<6,8>, no padding
    (98, DEFAULT),    # k_grf_hartley<7,8>
    (100, DEFAULT),   # k_grf_fft<10, float>
    (114, DEFAULT),   # k_grf_hartley<8,4>
    (120, DEFAULT),   # k_grf_hartley<8,4>
    (128, DEFAULT),   # k_grf_hartley<8,4>, no padding, last Hartley size
    (130, DEFAULT),   # first size of the DFT: XB 2, 1024 / 65 = 15 row groups, 9 rows -> k_grf_dft<20,2,1024,false>
    (150, DEFAULT),   # XB 2, 13 row groups, 12 rows -> k_grf_dft<20,2,1024,false>
    (200, DEFAULT),   # XB 4, 20 row groups, 10 rows -> k_grf_dft<10,4,1024,false>
    (254, DEFAULT),   # XB 2, 8 row groups, 32 rows -> k_grf_dft<32,2,1024,false>
    (256, DEFAULT),   # XB 4, 16 row groups, 16 rows -> k_grf_dft<16,4,1024,false>
    (258, DEFAULT),   # k_grf_conv<8, false> (799 KB of tables)
    (15, DEFAULT),    # k_grf_conv<5, true>
    (99, DEFAULT),    # k_grf_conv<8, true> (odd, n > 64, 115 KB of tables); <5, false> is unreachable: n <= 64 always fits LDS
    (50, NO_FFT),     # k_grf_hartley<4,4,13>
    (100, NO_FFT),    # k_grf_hartley<7,8,25>
    (36, NO_HARTLEY),   # XB 4 -> k_grf_dft<10,4,256,true>
    (50, NO_HARTLEY),   # XB 2, 256 / 25 = 10 row groups, 5 rows -> k_grf_dft<10,2,256,true>
    (54, NO_HARTLEY),   # XB 2, 256 / 27 = 9 row groups, 6 rows -> k_grf_dft<10,2,256,true>
    (98, NO_HARTLEY),   # XB 2, 256 / 49 = 5 row groups, 20 rows -> k_grf_dft<20,2,256,true>; grf_kc = 6 of 50 spectrum rows: 9 k-chunks
    (100, NO_HARTLEY),  # XB 4 -> k_grf_dft<10,4,256,true>, grf_kc = 5
    (128, NO_HARTLEY),  # XB 4, 1024 / 32 = 32 row groups, 4 rows -> k_grf_dft<10,4,1024,false>
]


def grf_engine(monkeypatch, n, switches, capacity=3, cluster_radius=5.0):
    from ipp_rl_amd import EngineConfig, IPPEngine

    for k, v in switches.items():  # (read once, at creation; monkeypatch restores them when the test ends)
        monkeypatch.setenv(k, v)
    eng = IPPEngine(EngineConfig(x_dim=n, y_dim=n, cluster_radius=cluster_radius), capacity=capacity, state="factor", rank_cap=16)
    assert eng.grf_generator() == expected_generator(n, switches), (n, switches, eng.grf_generator())  # the switch was seen
    return eng


def check_fields(eng, white, radius=5.0):
    n = white.shape[-1]
    out = host(eng.generate_grf(white)).reshape(len(white), n, n)
    for k in range(len(white)):
        ref = orc.grf_from_white_noise(white[k], radius)
        assert np.max(np.abs(out[k] - ref)) < TOL, (n, k, np.max(np.abs(out[k] - ref)))
        assert out[k].min() == 0.0 and abs(out[k].max() - 1.0) < 1e-6
    return out


@pytest.mark.parametrize("n,switches", GRF_CASES, ids=[str(n) + "".join(f"-{k}={v}" for k, v in sw.items()) for n, sw in GRF_CASES])
def test_grf_sizes_vs_oracle(monkeypatch, n, switches):
    """Every instantiation launch_grf can pick, at least once (GRF_CASES says which case runs which): the fast Hartley transforms
    (n = 50 / 100), the fp64 GEMM form for every TT = 1 .. 8 with and without zero padding and, under IPP_GRF_FFT=0, with the contracted
    K of n = 50 / 100; the half-spectrum DFT kernel in its four 1024-thread forms and, under IPP_GRF_HARTLEY=0, its three 256-thread
    forms; n = 258 and odd n (the reference's amplitude table loses its last row / column there, ground_truths.py:8-11): the
    circular-convolution kernel.  All against numpy's FFT path."""
    import torch

    eng = grf_engine(monkeypatch, n, switches)
    rs = np.random.RandomState(n)
    white = rs.normal(size=(3, n, n))
    check_fields(eng, white)
    eng.reset(env_ids=[1], white_noise=white[2][None])
    assert np.max(np.abs(host(eng.read_gt(1)) - orc.grf_from_white_noise(white[2], 5.0))) < TOL
    if n in (50, 100):  # the switch was seen: only the fast Hartley path draws its own noise
        out = torch.empty((1, n * n), dtype=torch.float32, device="cuda")
        assert eng.generate_grf_rows(1, 3, 1 << 40, out) is (switches == DEFAULT)
    eng.close()


@pytest.mark.parametrize("n", [50, 64, 150, 15])
def test_grf_impulse_orientation(monkeypatch, n):
    """One generator of every family (fast Hartley, GEMM, DFT, convolution) on white noise that is 1 at (row 3, column n - 2), -1 at
    (0, 1) and 0 elsewhere: the field is the difference of two shifted copies of the convolution kernel, so an output that is
    transposed or mirrored (the GEMM forms store every product transposed) is wrong by O(1), not by a rounding."""
    eng = grf_engine(monkeypatch, n, DEFAULT)
    white = np.zeros((2, n, n))
    white[0, 3, n - 2], white[0, 0, 1] = 1.0, -1.0
    white[1, n - 2, 3], white[1, 1, 0] = 1.0, -1.0  # its transpose, as another field of the same launch
    out = check_fields(eng, white)
    ref = orc.grf_from_white_noise(white[0], 5.0)
    for wrong in (ref.T, ref[::-1], ref[:, ::-1], np.roll(ref[::-1, ::-1], 1, axis=(0, 1))):  # (the case can tell them apart)
        assert np.max(np.abs(wrong - ref)) > 0.1
    assert np.max(np.abs(out[1] - out[0].T)) < TOL
    eng.close()


@pytest.mark.parametrize("radius", [1.5, 3.0])
@pytest.mark.parametrize("n", [50, 64, 150, 15])
def test_grf_cluster_radius(monkeypatch, n, radius):
    """The amplitude tables of every family are built from the engine's cluster_radius, not from the default 5.0."""
    eng = grf_engine(monkeypatch, n, DEFAULT, cluster_radius=radius)
    white = np.random.RandomState(1000 + n).normal(size=(3, n, n))
    out = check_fields(eng, white, radius)
    assert np.max(np.abs(out[0] - orc.grf_from_white_noise(white[0], 5.0))) > 0.05  # (another field than the default radius gives)
    eng.close()


@pytest.mark.parametrize("n", [50, 100])
def test_grf_drawn_noise_vs_host_reference(monkeypatch, n):
    """ipp_generate_grf_rows (white noise drawn inside the fast Hartley generator) against the host: the white noise rebuilt with
    philox_normal4_ref and the row-keyed addressing (row_len = n^2), pushed through the oracle.  The existing bit-for-bit test
    (test_hip_sharding.py) compares two users of the same device function; this one closes the loop to the definition.  The offset
    carries counter = (row id + offset) * n^2 / 4 across 2^32."""
    import torch
    from ipp_rl_amd.vec_env import philox_normal_rows_ref

    eng = grf_engine(monkeypatch, n, DEFAULT, capacity=8)
    N, seed, sub, row_ids = n * n, (0x9E3779B9 << 32) | 77, (1 << 40) + 9, [5, 0, 7, 3, 3]
    ids = torch.tensor(row_ids, dtype=torch.int32, device="cuda")
    for off in (0, 7000000):
        assert off == 0 or (off * (N // 4) > 2 ** 32 and off < 2 ** 32)
        out = torch.empty((5, N), dtype=torch.float32, device="cuda")
        assert eng.generate_grf_rows(5, seed, sub, out, row_ids=ids, row_offset=off) is True
        out = host(out).reshape(5, n, n)
        white = philox_normal_rows_ref(1, row_ids, N, seed, sub, off)[0].reshape(5, n, n)
        worst = 0.0
        for k in range(5):
            err = np.max(np.abs(out[k] - orc.grf_from_white_noise(white[k], 5.0)))
            worst = max(worst, err)
            assert err < TOL, (n, off, k, err)
        print(f"RATIO drawn-noise field {n}x{n} offset {off}: max |device - oracle of the fp64 normals| {worst:.3e} (TOL {TOL:.0e})")
        assert np.array_equal(out[3], out[4]) and not np.array_equal(out[0], out[1])
    eng.close()
