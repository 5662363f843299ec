"""
GPU tests of grf_rows="all" (ipp_set_grf_rows): every Gaussian-random-field generator family draws its own white noise -- the
GEMM-Hartley kernels and the 256-thread DFT kernels into the LDS array they stage it in, the 1024-thread DFT kernels into the field's
own destination -- from the one noise definition of csrc/k_grf_noise.h.  The grids are the smallest and the boundary shapes of each
family (which kernel a grid runs: the table above GRF_CASES in tests/test_hip_big_grids.py):
  default             34, 48, 128          k_grf_hartley TT = 3 padded, TT = 3 unpadded, TT = 8 (the largest)
  default             130, 132, 254, 256   the four 1024-thread k_grf_dft forms
  IPP_GRF_HARTLEY=0   36, 50, 98           the three 256-thread k_grf_dft forms
  IPP_GRF_FFT=0       50                   the contracted-K k_grf_hartley form
  default             50                   k_grf_fft itself, as a regression
The bar against the definition is the one of tests/test_hip_big_grids.py: 1e-5 of the normalised field against numpy's fp64 FFT path.
"""
import numpy as np
import pytest

from oracle import ipp_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEFAULT, NO_FFT, NO_HARTLEY = {}, {"IPP_GRF_FFT": "0"}, {"IPP_GRF_HARTLEY": "0"}
CASES = [(34, DEFAULT), (48, DEFAULT), (128, DEFAULT), (130, DEFAULT), (132, DEFAULT), (254, DEFAULT), (256, DEFAULT),
         (36, NO_HARTLEY), (50, NO_HARTLEY), (98, NO_HARTLEY), (50, NO_FFT), (50, DEFAULT)]
IDS = [str(n) + "".join(f"-{k}={v}" for k, v in sw.items()) for n, sw in CASES]
SEED, SUB = (0x9E3779B9 << 32) | 77, (1 << 40) + 9
ROW_IDS = [5, 0, -1, 3, 3]


def host(t):
    return t.detach().cpu().numpy()


def engine(monkeypatch, n, switches, grf_rows="all", **kw):
    from ipp_rl_amd import EngineConfig, IPPEngine, _ffi

    for k, v in switches.items():  # (read once, at creation; monkeypatch restores them when the test ends)
        monkeypatch.setenv(k, v)
    args = dict(capacity=8, state="factor", rank_cap=16)
    args.update(kw)
    eng = IPPEngine(EngineConfig(x_dim=n, y_dim=n), grf_rows=grf_rows, **args)
    assert eng.grf_rows == grf_rows
    if switches == NO_HARTLEY or n > 128:
        family = _ffi.IPP_GRF_GEN_DFT
    else:
        family = _ffi.IPP_GRF_GEN_FFT if (n in (50, 100) and switches == DEFAULT) else _ffi.IPP_GRF_GEN_HARTLEY
    assert eng.grf_generator()[0] == family, (n, switches, eng.grf_generator())  # the switch was seen
    return eng


def two_call_fields(eng, N, seed, sub, row_ids, off):
    """The route every grid has: ipp_fill_normal_rows into a buffer, ipp_generate_grf from it."""
    import torch

    white = torch.empty((len(row_ids), N), dtype=torch.float32, device="cuda")
    eng.normal_rows(white, N, seed, sub, row_ids=row_ids, row_offset=off)
    return eng.generate_grf(white)


def carry_offset(N):
    """A row offset that carries counter = (row id + offset) * N / 4 across 2^32 (as test_grf_drawn_noise_vs_host_reference chooses it)."""
    off = 2 ** 32 // (N // 4) + 12345
    assert off * (N // 4) > 2 ** 32 and off < 2 ** 32
    return off


@pytest.mark.parametrize("n,switches", CASES, ids=IDS)
def test_rows_equal_the_two_call_path_and_the_definition(monkeypatch, n, switches):
    import torch
    from ipp_rl_amd.vec_env import philox_normal_rows_ref

    eng = engine(monkeypatch, n, switches)
    N = n * n
    ids = torch.tensor(ROW_IDS, dtype=torch.int32, device="cuda")
    live = [0, 1, 3, 4]
    for off in (0, carry_offset(N)):
        out = torch.full((5, N), -1.0, dtype=torch.float32, device="cuda")
        assert eng.generate_grf_rows(5, SEED, SUB, out, row_ids=ids, row_offset=off) is True
        want = two_call_fields(eng, N, SEED, SUB, ids, off)
        torch.cuda.synchronize()
        out, want = host(out), host(want)
        # 1. bit-identity with the two-call path; the skipped row is untouched
        for k in live:
            assert np.array_equal(out[k], want[k]), (n, off, k, np.max(np.abs(out[k] - want[k])))
        assert np.all(out[2] == -1.0)
        assert np.array_equal(out[3], out[4]) and not np.array_equal(out[0], out[1])
        # 2. closed to the definition: the fp64 normals of the host reference through numpy's FFT path
        white = philox_normal_rows_ref(1, [ROW_IDS[k] for k in live], N, SEED, SUB, off)[0].reshape(len(live), n, n)
        worst = 0.0
        for j, k in enumerate(live):
            err = float(np.max(np.abs(out[k].astype(np.float64).reshape(n, n) - orc.grf_from_white_noise(white[j], 5.0))))
            worst = max(worst, err)
            assert err < TOL, (n, off, k, err)
        print(f"RATIO drawn-noise field {n}x{n} {switches} offset {off}: max |device - oracle of the fp64 normals| {worst:.3e} (TOL {TOL:.0e})")
    eng.close()


@pytest.mark.parametrize("n,switches", CASES, ids=IDS)
def test_groups_equal_plain_calls(monkeypatch, n, switches):
    import torch

    eng = engine(monkeypatch, n, switches)
    N = n * n
    ids = torch.tensor([4, 1, 6, -1, 2, 2], dtype=torch.int32, device="cuda")
    groups = [0, 3, 7]
    out = torch.full((6, N), -1.0, dtype=torch.float32, device="cuda")
    assert eng.generate_grf_rows(6, SEED, SUB, out, row_ids=ids, row_offset=11, group_rows=2, group_subsequence=groups) is True
    want = torch.full((6, N), -1.0, dtype=torch.float32, device="cuda")
    for g, gs in enumerate(groups):
        assert eng.generate_grf_rows(2, SEED, SUB + gs, want[2 * g:2 * g + 2], row_ids=ids[2 * g:2 * g + 2].contiguous(), row_offset=11) is True
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bool((out[3] == -1.0).all()) and not torch.equal(out[4], out[1])
    # (row id 2 in group 2 is another field than it would be in group 0: the group's subsequence is part of the key)
    one = torch.empty((1, N), dtype=torch.float32, device="cuda")
    assert eng.generate_grf_rows(1, SEED, SUB, one, row_ids=ids[4:5].contiguous(), row_offset=11) is True
    assert not torch.equal(one[0], out[4])
    eng.close()


@pytest.mark.parametrize("n,switches", CASES, ids=IDS)
def test_default_is_off(monkeypatch, n, switches):
    import torch

    eng = engine(monkeypatch, n, switches, grf_rows=None)
    N = n * n
    ids = torch.tensor(ROW_IDS, dtype=torch.int32, device="cuda")
    out = torch.full((5, N), -1.0, dtype=torch.float32, device="cuda")
    served = n in (50, 100) and switches == DEFAULT  # k_grf_fft draws its own noise with or without the switch
    assert eng.generate_grf_rows(5, SEED, SUB, out, row_ids=ids) is served
    refill = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    episode = torch.zeros(8, dtype=torch.int64, device="cuda")
    if not served:
        from ipp_rl_amd import _ffi

        assert eng.generate_fields_rows(_ffi.IPP_FIELD_GRF, 5, SEED, SUB, out, row_ids=ids) is False
        assert eng.generate_fields_refill(_ffi.IPP_FIELD_GRF, 2, refill, episode, SEED, SUB) is False
        torch.cuda.synchronize()
        assert bool((out == -1.0).all())  # no output byte changed
    eng.close()


@pytest.mark.parametrize("n,switches", [(40, DEFAULT), (132, DEFAULT), (40, NO_HARTLEY)], ids=["40", "132", "40-IPP_GRF_HARTLEY=0"])
def test_alternate_plane_and_flip(monkeypatch, n, switches):
    """Fields staged with out=None for env slots {0, 2} of four, then a step with a folded reset of all four: the staged envs carry
    exactly those fields, the others are poisoned as an unstaged flip is (tests/test_hip_autoreset.py)."""
    import torch

    B, N = 4, n * n
    eng = engine(monkeypatch, n, switches, capacity=B, rank_cap=90, window_rows=-1, fixed_prior=True)
    assert int(eng.info.fused_step) == 1 and int(eng.info.patch_layout) == 1
    rs = np.random.RandomState(3)
    eng.reset(white_noise=rs.normal(size=(B, n, n)))
    before = [host(eng.read_gt(e)).copy() for e in range(B)]
    prev = torch.tensor([2.0, 2.0, 14.0], dtype=torch.float64, device="cuda").repeat(B, 1)
    staged = torch.tensor([0, -1, 2], dtype=torch.int32, device="cuda")
    assert eng.generate_grf_rows(3, 11, 1 << 40, None, row_ids=staged, row_offset=5) is True
    want = host(two_call_fields(eng, N, 11, 1 << 40, staged, 5))
    for e in range(B):  # staging leaves every CURRENT plane alone
        assert np.array_equal(host(eng.read_gt(e)), before[e]), e
    src = torch.arange(B, dtype=torch.int32, device="cuda")
    res = eng.cfg.resolution
    acts = np.stack([res * rs.randint(0, n, B) + 0.5 * res, res * rs.randint(0, n, B) + 0.5 * res, rs.randint(5, 15, B).astype(float)], axis=1)
    r, st = eng.step(acts, prev, meas_noise=rs.normal(size=(B, 9)), reset_src=src, reset_gt=None, init_action=(2.0, 2.0, 14.0), update_prev=True)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and bool(torch.isfinite(r).all())  # the step itself ran before the resets
    for e, k in ((0, 0), (2, 2)):
        assert np.array_equal(host(eng.read_gt(e)).reshape(-1), want[k]), e
        assert bool(torch.isfinite(eng.read_diag(e)).all()) and bool(torch.isfinite(eng.read_mean(e)).all()), e
    for e in (1, 3):
        assert bool(torch.isnan(eng.read_mean(e)).all()) and bool(torch.isnan(eng.read_diag(e)).all()), e
    eng.close()


@pytest.mark.parametrize("n", [35, 258])
def test_refused_grids_name_the_rule(n):
    from ipp_rl_amd import EngineConfig, IPPEngine

    with pytest.raises(ValueError, match=r"even square grids of 4 \.\. 256"):
        IPPEngine(EngineConfig(x_dim=n, y_dim=n), capacity=2, state="factor", rank_cap=16, grf_rows="all")
    eng = IPPEngine(EngineConfig(x_dim=n, y_dim=n), capacity=2, state="factor", rank_cap=16)  # (the grid itself builds)
    assert eng.grf_rows is None
    eng.close()
