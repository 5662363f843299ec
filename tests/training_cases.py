"""
The training cases shared by the generator of tests/golden/training.npz (tests/golden/gen_training_golden.py) and the tests
(test_training_host.py, test_hip_train_kernels.py, test_hip_trainer.py): the loss minibatches with their row kinds, the SGD vectors,
the hyper-parameters and the dummy samples of the end-to-end run.  Everything is drawn from NumPy's legacy RandomState stream.
"""
import os
from functools import lru_cache

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training.npz")

# (n, A) of the loss kernel's tests; the fixture records the reference on those with A <= 257
LOSS_SHAPES = ((1, 1), (2, 63), (3, 64), (3, 65), (5, 257), (4, 1025), (2, 20011), (96, 200))
GOLDEN_LOSS_SHAPES = tuple(s for s in LOSS_SHAPES if s[1] <= 257)
# row r of a minibatch is of kind ROW_KINDS[r] while there are kinds left, then "random": the kinds that catch a wrong kernel first
ROW_KINDS = ("shift_not_mask", "all_masked", "one_valid", "all_valid", "one_hot_target", "mass_0.7", "weight_0", "span_80")
COEFFS = dict(policy=1.0, value=0.7, reward=1.3)
ENTROPY_COEFFS = (0.0, 0.2)


def loss_case(n, A, seed=0):
    """Inputs of one minibatch, float32 / uint8 / float64 as ipp_pvnet_loss takes them (reward and target_reward always drawn: a test
    without reward leaves them out)."""
    rs = np.random.RandomState([991, n, A, seed])
    z = rs.normal(0.0, 2.0, size=(n, A))
    m = (rs.random_sample((n, A)) < 0.5).astype(np.uint8)
    t = rs.random_sample((n, A))
    w = rs.uniform(0.2, 1.0, size=n)
    kinds = []
    for r in range(n):
        kind = ROW_KINDS[r] if r < len(ROW_KINDS) else "random"
        kinds.append(kind)
        m[r, rs.randint(A)] = 1  # (a random row has a valid action)
        if kind == "shift_not_mask":  # valid logits at -2000 against invalid ones at 0: the shifted invalid actions carry the softmax
            if A > 1:
                m[r, rs.randint(A)] = 1
                m[r, (int(np.argmax(m[r])) + 1) % A] = 0
            z[r] = np.where(m[r] == 1, -2000.0 + z[r], z[r])
        elif kind == "all_masked":
            m[r] = 0
        elif kind == "one_valid":
            m[r] = 0
            m[r, rs.randint(A)] = 1
        elif kind == "all_valid":
            m[r] = 1
        elif kind == "span_80":
            z[r] = rs.permutation(np.linspace(-80.0, 80.0, A)) if A > 1 else 80.0
        elif kind == "weight_0":
            w[r] = 0.0
        valid = m[r] == 1
        if kind == "one_hot_target":
            t[r] = 0.0
            t[r, np.nonzero(valid)[0][rs.randint(valid.sum())]] = 1.0
        elif kind == "mass_0.7" and valid.any() and (~valid).any():
            t[r, valid] *= 0.7 / t[r, valid].sum()
            t[r, ~valid] *= 0.3 / t[r, ~valid].sum()
        elif valid.any():
            t[r, ~valid] = 0.0
            t[r] /= t[r].sum()
            if kind == "mass_0.7":
                t[r] *= 0.7
    return dict(kinds=kinds, logits=z.astype(np.float32), target_policy=t.astype(np.float32), valid_msk=m,
                value=rs.uniform(0.1, 2.0, size=n).astype(np.float32), reward=rs.uniform(0.0, 1.0, size=n).astype(np.float32),
                target_value=rs.uniform(0.1, 2.0, size=n), target_reward=rs.uniform(0.05, 1.0, size=n), weights=w)


SGD_SIZES = (1, 255, 256, 257, 65537, 200003)
# (name, gradient scale, lr, momentum, weight_decay, max_norm): the norm below and above max_norm, zero gradients, wd = 0, mu = 0
SGD_CASES = (("below", 1e-3, 0.05, 0.9, 3e-5, 10.0), ("above", 3.0, 0.05, 0.9, 3e-5, 1.0), ("zero_grad", 0.0, 0.05, 0.9, 3e-5, 1.0),
             ("no_decay", 3.0, 0.02, 0.85, 0.0, 1.0), ("no_momentum", 3.0, 0.02, 0.0, 3e-5, 1.0))
SGD_STEPS = 3


def sgd_case(N, scale, seed=0):
    """(params [N], the gradients of SGD_STEPS consecutive steps [SGD_STEPS, N]) as float32."""
    rs = np.random.RandomState([992, N % 65521, seed])
    return rs.normal(0.0, 0.5, size=N).astype(np.float32), (scale * rs.normal(0.0, 1.0, size=(SGD_STEPS, N))).astype(np.float32)


# ---- the end-to-end run: pvnet case "b" (tests/pvnet_cases.py), 24 dummy samples, batch 8, 2 epochs
E2E_CASE, E2E_SAMPLES, E2E_SEED = "b", 24, 4242
E2E_TRAIN = dict(batch_size=8, num_augmented_samples=0, num_epochs=2, learning_rate=0.002, max_learning_rate=0.02, weight_decay=3e-5,
                 momentum=0.9, max_grad_norm=2.0, policy_loss_coeff=1.0, value_loss_coeff=1.0, reward_loss_coeff=1.0,
                 reconstruction_loss_coeff=1.0, entropy_regularization_coeff=0.01, replay_alpha=0.75, replay_beta0=0.4, use_per=False,
                 log_network_parameters=False)


def e2e_params(use_per=False):
    from tests import pvnet_cases as pc

    hp, md = pc.params(E2E_CASE)
    hp = dict(hp, **E2E_TRAIN)
    hp["use_per"] = bool(use_per)
    return hp, md


def e2e_samples():
    """The dummy training samples, as the reference pickles them: (input_feature_planes, policy, value, reward, valid_actions_msk)."""
    from tests import pvnet_cases as pc

    c = pc.CONFIGS[E2E_CASE]
    A = c["side"] ** 2 * c["levels"]
    rs = np.random.RandomState([E2E_SEED, 1])
    out = []
    for _ in range(E2E_SAMPLES):
        planes = rs.random_sample((c["input_channels"], c["side"], c["side"])).astype(np.float32)
        msk = (rs.random_sample(A) < 0.3).astype(np.float64)
        msk[rs.randint(A)] = 1.0
        pol = rs.random_sample(A) * msk
        pol /= pol.sum()
        out.append((planes, pol.astype(np.float32), float(rs.uniform(0.2, 1.5)), float(rs.uniform(0.0, 0.5)), msk))
    return out


def e2e_batch(ids, index, weights, weight_dtype, device="cpu"):
    """The 7-tuple of ReplayBuffer.sample for the dummy samples `ids`: states f32, policies f32, values f64, rewards f64, mask u8,
    indices i64, weights."""
    import torch

    s = e2e_samples()
    rows = [s[i] for i in ids]
    b = (torch.from_numpy(np.stack([r[0] for r in rows])), torch.from_numpy(np.stack([r[1] for r in rows])),
         torch.tensor([r[2] for r in rows], dtype=torch.float64), torch.tensor([r[3] for r in rows], dtype=torch.float64),
         torch.from_numpy(np.stack([r[4] for r in rows]).astype(np.uint8)), torch.from_numpy(np.asarray(index, dtype=np.int64)),
         torch.from_numpy(np.asarray(weights)).to(weight_dtype))
    return tuple(t.to(device) for t in b)


@lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))
