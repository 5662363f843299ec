"""
CPU tests of tests/mcts_noise_ref.py, the fp64 restatement of the device tree search's Dirichlet-noise stream (csrc/k_mcts.h:
mc_mix, mc_u01, mc_gamma, the noisy branch of k_mcts_expand).  They tie the restatement to the mathematics, not to the kernel: the
published splitmix64 sequence, the law of the gamma draws (below and above shape 1, and at the shape of the aggregated `rest`
draw), the Beta marginal of one action's share of the noise.  The last test checks, for every key the device comparison
(tests/test_hip_mcts_expand.py) uses, that no acceptance test of the sampler is decided by less than 1e-9: a rounding difference
in the device's log / pow / cos then cannot flip an accept, and that comparison is deterministic.
"""
import math

import numpy as np
import pytest

from tests.mcts_noise_ref import (NOISE_CASES, NOISE_EPS, case_roots, gamma_ref, mix64, noise_keys, noisy_priors_ref, prior_of,
                                  seed64_of, u01)

KS_P = 1e-3
A20, K20 = 800, 162  # 20x20 cells x 2 altitudes; the row width (most candidates of a position) at max_valid_action_distance 11.5


def test_splitmix64_known_answers():
    """The first two outputs of splitmix64 from state 0 (Vigna's reference implementation; the test vectors of java.util.SplittableRandom
    ports): output n is mix64 of n increments of the golden-ratio constant."""
    assert mix64(0) == 0xE220A8397B1DCDAF
    assert mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert u01(0) == 2.0 ** -54 and u01((1 << 64) - 1) == 1.0 - 2.0 ** -54  # never 0 or 1: log(u) and u^(1/shape) stay finite


@pytest.mark.parametrize("shape", [0.3, 0.64, 1.0, 2.5, 0.3 * (A20 - K20)])
def test_gamma_draws_follow_the_gamma_law(shape):
    """Kolmogorov-Smirnov against Gamma(shape, 1) over 20000 fixed keys (the keys are fixed: the outcome is deterministic)."""
    from scipy import stats

    keys = [mix64(0xC0FFEE + 977 * i) for i in range(20000)]
    draws = np.array([gamma_ref(shape, key)[0] for key in keys])
    res = stats.kstest(draws, stats.gamma(shape).cdf)
    print(f"shape {shape:g}: KS D {res.statistic:.4f} p {res.pvalue:.3f}; mean {draws.mean():.4f}")
    assert res.pvalue > KS_P


def test_noise_shares_are_beta():
    """Dirichlet(alpha) over A actions: one action's share is Beta(alpha, (A - 1) alpha), the K valid actions' shares together are
    Beta(K alpha, (A - K) alpha).  Both recovered from the noisy root priors of 4000 root numbers (A = 800, K = 162, alpha = 0.3).  A
    wrong shape of the aggregated `rest` draw moves the total: drawn with alpha A, the single share still passes at 4000 samples
    (p = 2e-3, its law is that skewed), the valid actions' total does not (its mean moves by 1.3 standard deviations)."""
    from scipy import stats

    A, K, alpha, eps = A20, K20, 0.3, NOISE_EPS
    one, total = [], []
    for root in range(4000):
        ps = noisy_priors_ref(5, root, K, A, alpha, eps)
        shares = (ps * ((1 - eps) * K / A + eps) - (1 - eps) / A) / eps
        one.append(shares[root % K])
        total.append(math.fsum(shares))
    res_one = stats.kstest(np.array(one), stats.beta(alpha, (A - 1) * alpha).cdf)
    res_tot = stats.kstest(np.array(total), stats.beta(K * alpha, (A - K) * alpha).cdf)
    print(f"one action: KS D {res_one.statistic:.4f} p {res_one.pvalue:.3f}, mean share x A {np.mean(one) * A:.3f}; "
          f"valid total: KS D {res_tot.statistic:.4f} p {res_tot.pvalue:.3f}, mean {np.mean(total):.4f} (K / A = {K / A:.4f})")
    assert res_one.pvalue > KS_P and res_tot.pvalue > KS_P


def test_given_priors_take_the_place_of_the_uniform_ones():
    """The two closed forms agree where they must: given priors that are all 1/A are the uniform case, and without noise weight the
    result is the plain normalisation over the valid set."""
    A, K = A20, 37
    a = noisy_priors_ref(3, 2, K, A, 0.64, NOISE_EPS)
    b = noisy_priors_ref(3, 2, K, A, 0.64, NOISE_EPS, prior=np.full(K, 1.0 / A))
    assert np.max(np.abs(a / b - 1)) < 1e-15
    p = prior_of(np.arange(100, 100 + K))
    assert np.max(np.abs(noisy_priors_ref(3, 2, K, A, 0.64, 0.0, prior=p) - p / p.sum())) < 1e-16
    assert np.all(a > 0) and a.sum() < 1.0  # (the mass that lands on invalid actions stays there)


def test_acceptance_margins_of_every_key_of_the_device_comparison():
    """Every draw of every root of the device cases: accepted or rejected by more than 1e-9 in every round, within 32 rounds."""
    worst, most, n = math.inf, 0, 0
    for name, case in NOISE_CASES.items():
        _, valid = case_roots(case["dim"], case["R"], case["max_dist"])
        A = 2 * case["dim"] ** 2
        assert all(len(v) > 0 for v in valid)
        for alpha in case["alphas"]:
            for j, vi in enumerate(valid):
                K = len(vi)
                nkey, keys = noise_keys(case["seed"], j, K)
                for shape, key in [(alpha, k) for k in keys] + [(alpha * (A - K), nkey)]:
                    _, margin, rounds = gamma_ref(shape, key)
                    assert margin > 1e-9 and rounds <= 32, (name, alpha, j, hex(key), margin, rounds)
                    worst, most, n = min(worst, margin), max(most, rounds), n + 1
    print(f"{n} draws: smallest acceptance margin {worst:.3e}, most rounds {most}")
    assert seed64_of(0) == 12345
