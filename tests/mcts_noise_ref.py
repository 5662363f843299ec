"""
fp64 restatement of the device tree search's Dirichlet-noise stream (csrc/k_mcts.h: mc_mix, mc_u01, mc_gamma and the noisy branch
of k_mcts_expand) in plain Python: integers masked to 64 bits, `math` for the rest, no torch.  tests/test_mcts_noise_host.py ties it
to the mathematics (splitmix64 known answers, the law of the gamma draws, the Beta marginal of a noise share);
tests/test_hip_mcts_expand.py compares the device's root priors with it value by value.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
TWO_PI = 6.283185307179586


def mix64(x):
    """mc_mix: one splitmix64 step (increment, then the finaliser)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def u01(h):
    """mc_u01: the top 53 bits as a uniform in (0, 1), never 0 or 1."""
    return (float(h >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def gamma_ref(shape, key):
    """mc_gamma: Marsaglia-Tsang Gamma(shape, 1) from the counter-based stream of `key` (shape < 1 through the u^(1/shape) boost).
    Returns (draw, margin, rounds): margin = the smallest |log(u3) - rhs| over the rounds that reached the acceptance test (inf when
    none did), rounds = the number of rounds used (65 when all 64 were rejected and the device returns boost * d)."""
    key &= M64
    boost = 1.0
    if shape < 1.0:
        boost = math.pow(u01(mix64(key ^ 0xA5A5A5A5)), 1.0 / shape)
        shape += 1.0
    dd = shape - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * dd)
    margin = math.inf
    c = 0
    for it in range(64):
        u1, u2, u3 = u01(mix64((key + c + 1) & M64)), u01(mix64((key + c + 2) & M64)), u01(mix64((key + c + 3) & M64))
        c += 3
        x = math.sqrt(-2.0 * math.log(u1)) * math.cos(TWO_PI * u2)  # Box-Muller
        t = 1.0 + cc * x
        if t <= 0.0:
            continue
        v = t * t * t
        lhs, rhs = math.log(u3), 0.5 * x * x + dd - dd * v + dd * math.log(v)
        margin = min(margin, abs(lhs - rhs))
        if lhs < rhs:
            return boost * dd * v, margin, it + 1
    return boost * dd, margin, 65


def seed64_of(seed):
    """The seed DeviceMCTS._expand hands to ipp_mcts_expand for DeviceMCTS(seed=seed)."""
    return (seed * 0x9E3779B97F4A7C15 + 12345) & M64


def noise_keys(seed, root_number, K):
    """(key of the aggregated `rest` draw, keys of the K per-action draws) of a root: root_number is the root's number in the whole
    search (its position among the roots of get_policy, whatever the groups)."""
    nkey = mix64(seed64_of(seed) ^ ((root_number & 0xFFFFFFFF) << 24))
    return nkey, [(nkey + ((k + 1) << 32)) & M64 for k in range(K)]


def noisy_priors_ref(seed, root_number, K, A, alpha, eps, prior=None, with_margin=False):
    """Root priors of the first simulation on the K valid actions (k_mcts_expand's noisy branch): Dirichlet(alpha) over all A actions
    looked at on the valid ones -- independent Gamma(alpha) draws for those, one Gamma((A - K) alpha) draw for the total of the rest --
    mixed with weight eps into the uniform prior 1/A (prior=None) or the given unnormalised priors on the valid set, and normalised
    over ALL actions.  With with_margin: (priors, smallest acceptance margin of any draw, most rounds of any draw)."""
    nkey, keys = noise_keys(seed, root_number, K)
    draws = [gamma_ref(alpha, key) for key in keys]
    rest = gamma_ref(alpha * (A - K), nkey) if A > K else (0.0, math.inf, 0)
    g = np.array([d[0] for d in draws], dtype=np.float64)
    gtot = math.fsum(g) + rest[0]
    if prior is None:
        p0, psum = np.full(K, 1.0 / A), float(K) / A
    else:
        p0 = np.asarray(prior, dtype=np.float64)[:K]
        psum = math.fsum(p0)
    ps = ((1 - eps) * p0 + eps * g / gtot) / ((1 - eps) * psum + eps)
    if with_margin:
        return ps, min([d[1] for d in draws] + [rest[1]]), max([d[2] for d in draws] + [rest[2]])
    return ps


# ---------------------------------------------------------------------------------------------------------------------
# The cases of the device comparison (tests/test_hip_mcts_expand.py), here so that the CPU test can check the acceptance margin of
# every key they use: name -> (grid, roots, max_valid_action_distance, alphas, priors given, groups, seed of DeviceMCTS).
NOISE_EPS = 0.25
NOISE_CASES = {
    "a": dict(dim=20, R=16, max_dist=11.5, alphas=(0.3, 1.0, 2.5), given=False, groups=1, seed=11),
    "b": dict(dim=20, R=16, max_dist=19.5, alphas=(0.3,), given=False, groups=1, seed=12),
    "c": dict(dim=20, R=16, max_dist=11.5, alphas=(0.64,), given=True, groups=1, seed=13),
    "d": dict(dim=50, R=37, max_dist=11.5, alphas=(0.3,), given=False, groups=2, seed=14),
}
ROOT_BUDGET = 60.0
ALTITUDES = (8.0, 14.0)


def prior_of(idx):
    """The prior function of the device-against-host comparisons: small integers (every summation order gives the same total, so
    device and NumPy priors are bit-identical), 0 on the -1 padding."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.where(idx >= 0, 1.0 + (idx * 7919) % 13, 0.0).astype(np.float64)


def case_roots(dim, R, max_dist, resolution=4.0):
    """(positions [R, 3], valid action indices per root) of the roots of tests/test_hip_mcts.py::_search_setup: the waypoints of its
    third step, the valid sets by mcts.py:148-158 over every cell centre at the two altitudes (action index = level N + x_dim col +
    row, planning/common/actions.py)."""
    rs = np.random.RandomState(10_000 + 2)  # vec_env.cell_centre_actions(cfg, 2, 0, R, R, ALTITUDES)
    col, row, lev = rs.randint(0, dim, R), rs.randint(0, dim, R), rs.randint(0, len(ALTITUDES), R)
    pos = np.stack([resolution * col + 0.5 * resolution, resolution * row + 0.5 * resolution, np.asarray(ALTITUDES)[lev]], axis=1)
    c, r = np.meshgrid(np.arange(dim), np.arange(dim), indexing="ij")
    cells = np.stack([resolution * c.ravel() + 0.5 * resolution, resolution * r.ravel() + 0.5 * resolution], axis=1)
    actions = np.concatenate([np.concatenate([cells, np.full((dim * dim, 1), a)], axis=1) for a in ALTITUDES])
    valid = []
    for p in pos:
        d = np.sqrt(((actions - p) ** 2).sum(axis=1))
        valid.append(np.nonzero((d > 0) & (d <= ROOT_BUDGET) & (d < max_dist))[0])
    return pos, valid
