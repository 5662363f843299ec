"""
The policy-value network cases of tests/golden/pvnet.npz, shared by the generator (tests/golden/gen_pvnet_golden.py) and the tests
(test_pvnet_host.py, test_hip_pvnet.py): the three configurations, and the DRAWS of their weights and planes.

A network's weights are not stored in the fixture: configuration (c) alone has 1.5 MB of them, above what one committed file may hold.
The fixture records the state_dict as names, shapes, a seed and a CRC-32 per tensor, and draw_state_dict() reproduces the tensors
from NumPy's legacy RandomState stream (frozen by NumPy's compatibility policy): the CRCs prove that the tensors a test rebuilds are,
bit for bit, the ones the reference ran with.  Planes are drawn the same way (U(0, 1), float32).
"""
import json
import os
import zlib
from functools import lru_cache

import numpy as np

KMAX = 37
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvnet.npz")
# the smallest configurations at which a class of mistake still shows:
#   a: the reference's full default schedule down to 1x1 pixels, a batch above one 64-row tile, an input channel count that is no multiple of anything
#   b: odd side, the plain residual path with its biased 1x1 identity convs, two altitude levels
#   c: a channel count that is no multiple of 32
CONFIGS = {
    "a": dict(side=20, input_channels=5, channels=32, pooled=8, blocks=10, separable=True, mixing=True, silu=True, heads=(3, 3), levels=1, n=70, seed=101),
    "b": dict(side=13, input_channels=7, channels=16, pooled=4, blocks=4, separable=False, mixing=False, silu=False, heads=(2, 1), levels=2, n=5, seed=202),
    "c": dict(side=9, input_channels=3, channels=48, pooled=16, blocks=7, separable=True, mixing=True, silu=True, heads=(1, 2), levels=1, n=5, seed=303),
}
TAP_ROWS = (0, 1, 2, 3, 31, 32, 62, 63, 64, 65, 68, 69)  # the samples of (a) whose block outputs the fixture keeps


def params(name):
    """(hyper_params, meta_data) of a configuration, in the reference's vocabulary."""
    c = CONFIGS[name]
    hp = dict(input_channels=c["input_channels"], num_channels=c["channels"], dropout=0.0, use_silu=c["silu"], num_encoder_res_blocks=c["blocks"],
              use_separable_conv_layers=c["separable"], use_global_context_mixing=c["mixing"], num_global_pooling_channels=c["pooled"],
              num_policy_head_conv_bn_blocks=c["heads"][0], num_value_head_conv_bn_blocks=c["heads"][1], mask_policy_head=True,
              use_reward_target=False, use_autoencoder=False)
    md = dict(num_grid_cells=c["side"] ** 2, min_altitude=8.0, max_altitude=8.0 + 6.0 * (c["levels"] - 1), altitude_spacing=6.0)
    return hp, md


def draw_state_dict(names, shapes, seed):
    """name -> ndarray: BatchNorm statistics and affines away from the identity (so that folding is exercised), conv / linear weights
    N(0, 1 / fan_in), biases N(0, 0.1^2).  One RandomState per tensor, seeded by (seed, position)."""
    names = list(names)
    out = {}
    for i, (name, shape) in enumerate(zip(names, shapes)):
        rs = np.random.RandomState([int(seed), i])
        shape = tuple(int(s) for s in shape)
        stem, leaf = name.rsplit(".", 1)
        is_bn = (stem + ".running_mean") in names
        if leaf == "num_batches_tracked":
            v = np.zeros(shape, dtype=np.int64)
        elif leaf == "running_var" or (is_bn and leaf == "weight"):
            v = rs.uniform(0.5, 1.5, size=shape)
        elif leaf == "running_mean" or (is_bn and leaf == "bias"):
            v = rs.normal(0.0, 0.2, size=shape)
        elif len(shape) >= 2:
            v = rs.normal(0.0, 1.0, size=shape) / np.sqrt(float(np.prod(shape[1:])))
        else:
            v = rs.normal(0.0, 0.1, size=shape)
        out[name] = v if v.dtype == np.int64 else v.astype(np.float32)
    return out


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def draw_planes(name):
    c = CONFIGS[name]
    return np.random.RandomState([c["seed"], 7777]).random_sample((c["n"], c["input_channels"], c["side"], c["side"])).astype(np.float32)


def draw_valid_idx(name):
    """Ascending valid sets, -1 padded: row 0 has one action, row 1 all KMAX, row 2 none."""
    c = CONFIGS[name]
    A = c["side"] ** 2 * c["levels"]
    rs = np.random.RandomState([c["seed"], 8888])
    idx = np.full((c["n"], KMAX), -1, dtype=np.int32)
    for r in range(c["n"]):
        K = {0: 1, 1: KMAX, 2: 0}.get(r, int(rs.randint(2, KMAX)))
        idx[r, :K] = np.sort(rs.choice(A, size=K, replace=False))
    return idx


@lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@lru_cache(maxsize=None)
def case(name):
    """Everything of one configuration, read once and shared (treat as read-only): params, the state_dict as torch tensors (CRC-checked),
    planes, valid_idx and the recorded outputs with d32 = max |ref32 - ref64| per output."""
    import torch

    fx = fixture()
    names = json.loads(str(fx[f"{name}_keys"]))
    shapes = json.loads(str(fx[f"{name}_shapes"]))
    sd = draw_state_dict(names, shapes, int(fx[f"{name}_seed"]))
    assert [crc(sd[k]) for k in names] == [int(v) for v in fx[f"{name}_crc"]], "the redrawn weights are not the recorded ones"
    planes, idx = draw_planes(name), fx[f"{name}_valid_idx"]
    assert crc(planes) == int(fx[f"{name}_planes_crc"])
    hp, md = params(name)
    out = dict(name=name, hp=hp, md=md, cfg=CONFIGS[name], keys=names, state_dict={k: torch.from_numpy(v.copy()) for k, v in sd.items()},
               planes=planes, valid_idx=idx)
    for k in ("prior32", "value32", "prior64", "value64"):
        out[k] = fx[f"{name}_{k}"]
    out["d32_prior"] = float(np.max(np.abs(out["prior32"] - out["prior64"])))
    out["d32_value"] = float(np.max(np.abs(out["value32"] - out["value64"])))
    if name == "a":
        out["tap_names"] = json.loads(str(fx["a_tap_names"]))
        out["taps64"] = [fx[f"a_tap64_{i}"] for i in range(len(out["tap_names"]))]
        out["tap_d32"] = [float(v) for v in fx["a_tap_d32"]]
    return out
