#!/usr/bin/env python
"""
Generate tests/golden/pvnet.npz by IMPORTING the reference's PolicyValueNetwork (planning/mcts_zero/networks/policy_value_networks.py)
and recording what it computes in eval mode for the three configurations of tests/pvnet_cases.py.

    python tests/golden/gen_pvnet_golden.py REFERENCE_CHECKOUT          (or IPP_REFERENCE=REFERENCE_CHECKOUT)

Per configuration x in (a, b, c) the fixture holds numbers and names only:
    {x}_keys, {x}_shapes   the reference's state_dict keys (in order) and tensor shapes, as JSON
    {x}_seed, {x}_crc      the seed of tests/pvnet_cases.py draw_state_dict and the CRC-32 of every tensor the reference was loaded with
    {x}_planes_crc         CRC-32 of the planes (draw_planes: U(0, 1), float32)
    {x}_valid_idx          random ascending valid sets, kmax = 37, -1 padded: one row with K = 1, one with K = kmax, one with K = 0
    {x}_prior32, _value32  exp(log_policy) gathered on the valid sets and v^2 + 2 v from the float32 run (what predict() returns)
    {x}_prior64, _value64  the same from the .double() run
and for (a): a_tap_names, a_tap64_{i} (the .double() output of every top-level block, samples TAP_ROWS) and a_tap_d32 (the largest
|float32 run - double run| of that block on those samples).

The weights themselves are NOT stored: every tensor of the state_dict (BatchNorm running statistics and affines included, drawn away
from the identity so that folding is exercised) comes from draw_state_dict's seeded stream, is loaded into the reference network with
strict=True, and is pinned by its CRC.  Stored as float32, configuration (c) alone would be 1.5 MB, more than a committed file may
hold; with the draws the fixture stays below 1 MB at the issue's sizes ((a) keeps C = 32, G = 8), and the block outputs of (a) are
kept for twelve of its seventy samples, on both sides of the 64-row tile edge.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import pvnet_cases as pc  # noqa: E402


def run(net, planes, idx, A, dtype, blocks):
    import torch

    n = planes.shape[0]
    mask = np.zeros((n, A))
    for r in range(n):
        mask[r, idx[r][idx[r] >= 0]] = 1.0
    taps = []
    hooks = [m.register_forward_hook(lambda mod, i, o: taps.append(o.detach().double().numpy().copy())) for m in blocks]
    with torch.no_grad():
        log_policy, value, _, _ = net.to(dtype)(torch.from_numpy(planes).to(dtype), torch.from_numpy(mask).to(dtype))
    for h in hooks:
        h.remove()
    policy = torch.exp(log_policy).double().numpy()
    prior = np.zeros((n, pc.KMAX))
    for r in range(n):
        ids = idx[r][idx[r] >= 0]
        prior[r, :len(ids)] = policy[r, ids]
    v = value.double().numpy().reshape(n)
    return prior, v * v + 2 * v, taps


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IPP_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("usage: gen_pvnet_golden.py REFERENCE_CHECKOUT (the fixture can only be generated next to the reference)")
    sys.path.insert(1, ref)
    import torch
    from planning.mcts_zero.networks.policy_value_networks import PolicyValueNetwork

    out = {}
    for name, c in pc.CONFIGS.items():
        hp, md = pc.params(name)
        torch.manual_seed(c["seed"])
        net = PolicyValueNetwork(hp, md).cpu().eval()
        ref_sd = net.state_dict()
        keys, shapes = list(ref_sd.keys()), [list(v.shape) for v in ref_sd.values()]
        sd = pc.draw_state_dict(keys, shapes, c["seed"])
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        planes, idx = pc.draw_planes(name), pc.draw_valid_idx(name)
        assert (idx[0] >= 0).sum() == 1 and (idx[1] >= 0).sum() == pc.KMAX and (idx[2] >= 0).sum() == 0
        # top-level blocks in call order: the stem and the (shared) encoder blocks, then the policy trunk's, then the value trunk's
        enc = net.encoder
        blocks = [enc.down_sample_block, enc.residual_block_s1, enc.residual_block_s2, enc.separable_residual_block_s1,
                  enc.separable_residual_block_s2, enc.mix_global_context_s1, enc.mix_global_context_s2]
        for head in (net.policy_head, net.value_head):
            blocks += [head.mix_global_context, head.conv_bn_block]
        p32, v32, t32 = run(net, planes, idx, net.num_actions, torch.float32, blocks)
        p64, v64, t64 = run(net, planes, idx, net.num_actions, torch.float64, blocks)
        assert np.isfinite(p64).all() and np.isfinite(v64).all()
        out.update({f"{name}_keys": np.array(json.dumps(keys)), f"{name}_shapes": np.array(json.dumps(shapes)), f"{name}_seed": np.int64(c["seed"]),
                    f"{name}_crc": np.array([pc.crc(sd[k]) for k in keys], dtype=np.int64), f"{name}_planes_crc": np.int64(pc.crc(planes)),
                    f"{name}_valid_idx": idx, f"{name}_prior32": p32, f"{name}_value32": v32, f"{name}_prior64": p64, f"{name}_value64": v64})
        print(name, "d32 prior %.3g value %.3g" % (np.abs(p32 - p64).max(), np.abs(v32 - v64).max()), "value range", v64.min(), v64.max())
        if name == "a":
            tap_names = (["encoder.down_sample_block"] + [f"encoder.block{i}" for i in range(c["blocks"])]
                         + [f"policy_head.block{i}" for i in range(c["heads"][0])] + [f"value_head.block{i}" for i in range(c["heads"][1])])
            assert len(tap_names) == len(t64) == len(t32)
            rows = list(pc.TAP_ROWS)
            out["a_tap_names"] = np.array(json.dumps(tap_names))
            out["a_tap_d32"] = np.array([np.abs(a[rows] - b[rows]).max() for a, b in zip(t32, t64)])
            for i, t in enumerate(t64):
                out[f"a_tap64_{i}"] = t[rows]
    path = os.path.join(ROOT, "tests", "golden", "pvnet.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
