"""
The policy-value network cases of tests/golden/pvnet.npz (a, b, c) and tests/golden/pvnet_edges.npz (d, e, f, g), shared by the
generator (tests/golden/gen_pvnet_golden.py) and the tests (test_pvnet_host.py, test_hip_pvnet.py): the configurations, and the DRAWS
of their weights and planes.

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

KMAX = 37  # of a, b and c; a configuration's own is kmax(name)
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(_GOLDEN, "pvnet.npz")
EDGE_FIXTURE = os.path.join(_GOLDEN, "pvnet_edges.npz")
# the smallest configurations at which a class of mistake still shows:
#   a: the reference's full default schedule down to 1x1 pixels, a batch above one 64-row tile, an input channel count that is no multiple of anything
#   b: odd side, the plain residual path with its biased 1x1 identity convs, two altitude levels
#   c: a channel count that is no multiple of 32
CONFIGS = {
    "a": dict(side=20, input_channels=5, channels=32, pooled=8, blocks=10, separable=True, mixing=True, silu=True, heads=(3, 3), levels=1, n=70, seed=101),
    "b": dict(side=13, input_channels=7, channels=16, pooled=4, blocks=4, separable=False, mixing=False, silu=False, heads=(2, 1), levels=2, n=5, seed=202),
    "c": dict(side=9, input_channels=3, channels=48, pooled=16, blocks=7, separable=True, mixing=True, silu=True, heads=(1, 2), levels=1, n=5, seed=303),
}
# ... and past one 64-channel tile of k_pv_conv, one pixel at the head pools and one pass of the 256-thread loops of k_pv_heads and
# k_pv_mix ("Policy-value network", has the table of which configuration reaches which edge; test_pvnet_host.py asserts it):
#   d: 72 channels: two output-channel tiles, the second 8 columns wide; no K a multiple of 32; a 3x3 map at the head pools; G = 24
#   e: the shipped network's channel, input and pooled counts: two full tiles, every K a multiple of 32, a 2x2 map at the head pools
#   f: 264 channels: five tiles, a head pool over >= 256 channels, 260 context channels in the mix, three altitude levels
#   g: 136 channels: a head pool over 129..255 channels, three tiles, the last 8 columns wide
# kmax = 300: the policy head's loops over the slots run a second pass.  `seed` is where the generator STARTS: it keeps the first seed
# at which a float32 NumPy run of the plan lies within 2 d32 of ref64 (gen_pvnet_golden.py), and the fixture's {x}_seed is the one kept.
EDGE_CONFIGS = {
    "d": dict(side=24, input_channels=5, channels=72, pooled=24, blocks=3, separable=True, mixing=True, silu=True, heads=(2, 2), levels=1, n=8, seed=404, kmax=300),
    "e": dict(side=32, input_channels=16, channels=128, pooled=32, blocks=4, separable=True, mixing=True, silu=True, heads=(2, 2), levels=1, n=8, seed=505, kmax=300),
    "f": dict(side=12, input_channels=3, channels=264, pooled=4, blocks=4, separable=False, mixing=True, silu=False, heads=(2, 1), levels=3, n=8, seed=606, kmax=300),
    "g": dict(side=12, input_channels=4, channels=136, pooled=8, blocks=2, separable=False, mixing=False, silu=False, heads=(1, 1), levels=3, n=8, seed=707, kmax=300),
}
EDGE_NAMES = tuple(EDGE_CONFIGS)
CONFIGS.update(EDGE_CONFIGS)
TAP_ROWS = (0, 1, 2, 3, 31, 32, 62, 63, 64, 65, 68, 69)  # the samples of (a) whose block outputs the fixture keeps
EDGE_TAP_ROWS = (0, 7)  # ... and of d, e, f and g


def kmax(name):
    return CONFIGS[name].get("kmax", KMAX)


def tap_rows(name):
    return EDGE_TAP_ROWS if name in EDGE_CONFIGS else TAP_ROWS


def block_names(name):
    """The top-level blocks of a configuration in call order, as build_plan names them."""
    c = CONFIGS[name]
    return (["encoder.down_sample_block"] + [f"encoder.block{i}" for i in range(c["blocks"])]
            + [f"policy_head.block{i}" for i in range(c["heads"][0])] + [f"value_head.block{i}" for i in range(c["heads"][1])])


def recorded_taps(name):
    """The blocks whose outputs the fixture keeps: all of a and d; of e, f and g the last encoder block and the last block of each head
    trunk (maps of at most 3x3, which separate a wrong encoder from a wrong head); none of b and c."""
    c = CONFIGS[name]
    if name in ("a", "d"):
        return block_names(name)
    if name not in EDGE_CONFIGS:
        return []
    return [f"encoder.block{c['blocks'] - 1}", f"policy_head.block{c['heads'][0] - 1}", f"value_head.block{c['heads'][1] - 1}"]


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


def draw_planes(name, seed=None):
    c = CONFIGS[name]
    return np.random.RandomState([c["seed"] if seed is None else int(seed), 7777]).random_sample((c["n"], c["input_channels"], c["side"], c["side"])).astype(np.float32)


def draw_valid_idx(name, seed=None):
    """Ascending valid sets, -1 padded: row 0 has one action, row 1 all kmax, row 2 none; the others 2..kmax-1 (a, b, c) or 257..kmax-1
    (the edge configurations: past one pass of 256 threads)."""
    c = CONFIGS[name]
    A, km = c["side"] ** 2 * c["levels"], kmax(name)
    rs = np.random.RandomState([c["seed"] if seed is None else int(seed), 8888])
    idx = np.full((c["n"], km), -1, dtype=np.int32)
    for r in range(c["n"]):
        K = {0: 1, 1: km, 2: 0}.get(r, int(rs.randint(257 if name in EDGE_CONFIGS else 2, km)))
        idx[r, :K] = np.sort(rs.choice(A, size=K, replace=False))
    return idx


@lru_cache(maxsize=None)
def fixture(name="a"):
    """The arrays of the file that holds configuration `name`."""
    return dict(np.load(EDGE_FIXTURE if name in EDGE_CONFIGS else FIXTURE))


@lru_cache(maxsize=None)
def case(name):
    """Everything of one configuration, read once and shared (treat as read-only): params, the state_dict as torch tensors (CRC-checked),
    planes, valid_idx and the recorded outputs with d32 = max |ref32 - ref64| per output."""
    import torch

    fx = fixture(name)
    names = json.loads(str(fx[f"{name}_keys"]))
    shapes = json.loads(str(fx[f"{name}_shapes"]))
    seed = int(fx[f"{name}_seed"])
    sd = draw_state_dict(names, shapes, seed)
    assert [crc(sd[k]) for k in names] == [int(v) for v in fx[f"{name}_crc"]], "the redrawn weights are not the recorded ones"
    planes, idx = draw_planes(name, seed), fx[f"{name}_valid_idx"]
    assert crc(planes) == int(fx[f"{name}_planes_crc"]) and np.array_equal(idx, draw_valid_idx(name, seed))
    hp, md = params(name)
    out = dict(name=name, hp=hp, md=md, cfg=CONFIGS[name], kmax=kmax(name), seed=seed, keys=names, state_dict={k: torch.from_numpy(v.copy()) for k, v in sd.items()},
               planes=planes, valid_idx=idx)
    for k in ("prior32", "value32", "prior64", "value64"):
        out[k] = fx[f"{name}_{k}"]
    out["d32_prior"] = float(np.max(np.abs(out["prior32"] - out["prior64"])))
    out["d32_value"] = float(np.max(np.abs(out["value32"] - out["value64"])))
    out["tap_names"], out["taps64"], out["tap_d32"], out["tap_rows"] = [], [], [], tap_rows(name)
    if f"{name}_tap_names" in fx:
        out["tap_names"] = json.loads(str(fx[f"{name}_tap_names"]))
        out["taps64"] = [fx[f"{name}_tap64_{i}"] for i in range(len(out["tap_names"]))]
        out["tap_d32"] = [float(v) for v in fx[f"{name}_tap_d32"]]
    assert out["tap_names"] == recorded_taps(name)
    return out
