#!/usr/bin/env python3
"""
Timing of ipp_feature_planes (one launch per batch): written bytes / time against the HBM peak.

Cases: 1024 requests x H = 3 on 10x10 (search leaves: current state + two prefixes), 4096 histories x H = 3 on 10x10 (env
training samples), 256 requests x H = 3 on 20x20 (the two-pass form: the plane does not fit LDS).  Position mode with the cost
plane (C = 16), adaptive.  Exact factor engines after 8 steps.

Usage:  python tools/plane_bench.py [--iters 50]        (results: profiles/plane_bench.txt)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E spec (6.29 TB/s measured with a float4 copy)


def case(n, dim, H, iters):
    import torch

    from ipp_rl_amd import EngineConfig, IPPEngine
    from ipp_rl_amd.feature_planes import PlaneSpec, make_entry, pack_entries

    B = min(n, 1024)
    eng = IPPEngine(EngineConfig(x_dim=dim, y_dim=dim), capacity=B, state="factor", rank_cap=96, score_scratch=True, device="cuda:0")
    rs = np.random.RandomState(0)
    eng.reset(white_noise=rs.normal(size=(B, dim, dim)))
    prev = np.tile([2.0, 2.0, 14.0], (B, 1))
    ranks = []
    for _ in range(8):
        ranks.append(eng.ranks().cpu().numpy()[:B].copy())
        c = rs.randint(0, dim, size=(B, 2))
        a = np.stack([4.0 * c[:, 0] + 2.0, 4.0 * c[:, 1] + 2.0, rs.choice([8.0, 14.0], size=B)], axis=1)
        eng.step(a, prev, meas_noise=rs.normal(size=(B, 9)))
        prev = a
    spec = PlaneSpec(H, use_costs=True, min_altitude=8.0, max_altitude=14.0)
    recs = pack_entries([[make_entry(i % B, prev[i % B], 0.9)] + [make_entry(i % B, prev[i % B], 0.8, rank=int(ranks[-k][i % B])) for k in range(1, H)]
                         for i in range(n)], H)
    mask_env = np.arange(n) % B
    out = eng.feature_planes(recs, spec, mask_env=mask_env)
    ent = eng._keep_planes[0]
    me = eng._keep_planes[1]
    for _ in range(3):
        eng.feature_planes(ent, spec, mask_env=me, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        eng.feature_planes(ent, spec, mask_env=me, out=out)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / iters
    nbytes = out.numel() * 4
    assert bool(torch.isfinite(out).all())
    eng.close()
    return ms, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch

    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'case':<34} {'ms':>8} {'MB written':>11} {'GB/s':>8} {'% HBM peak':>11}")
    for label, n, dim, H in (("1024 leaves x H=3, 10x10", 1024, 10, 3), ("4096 histories x H=3, 10x10", 4096, 10, 3),
                             ("256 requests x H=3, 20x20", 256, 20, 3)):
        ms, nbytes = case(n, dim, H, args.iters)
        gbs = nbytes / (ms * 1e-3) / 1e9
        print(f"{label:<34} {ms:8.3f} {nbytes / 1e6:11.1f} {gbs:8.0f} {100 * gbs * 1e9 / HBM_PEAK:10.1f}%")


if __name__ == "__main__":
    main()
