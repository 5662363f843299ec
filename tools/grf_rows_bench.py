#!/usr/bin/env python3
"""
Gaussian random fields with the white noise drawn in the generator (grf_rows="all", ipp_set_grf_rows) against the two-call path on
the same engine, per grid:fields pair:
  (a) rows       generate_grf_rows(fields, seed, subsequence, out)                 one launch, no noise array
  (b) two calls  normal_rows(white, N, seed, subsequence) + generate_grf(white)    what every grid could do before; the yardstick
Both produce the same fields bit for bit (tests/test_hip_grf_rows_all.py).  Per pair: a warm-up, then 5 timed windows of --reps calls
for each route, alternating; the median window and the spread (min .. max) are printed in ms per call.

usage: python tools/grf_rows_bench.py [--reps 10] [grid:fields ...]      default 40:2048 64:2048 128:512 200:102 256:64
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipp_rl_amd import EngineConfig, IPPEngine, _ffi  # noqa: E402

FAMILY = {_ffi.IPP_GRF_GEN_CONV: "conv", _ffi.IPP_GRF_GEN_DFT: "k_grf_dft", _ffi.IPP_GRF_GEN_HARTLEY: "k_grf_hartley", _ffi.IPP_GRF_GEN_FFT: "k_grf_fft"}
WINDOWS = 5


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("specs", nargs="*", default=["40:2048", "64:2048", "128:512", "200:102", "256:64"])
    a = ap.parse_args()
    for spec in a.specs:
        n, fields = (int(x) for x in spec.split(":"))
        eng = IPPEngine(EngineConfig(x_dim=n, y_dim=n), capacity=fields, state="factor", rank_cap=16, window_rows=0, grf_rows="all")
        N = n * n
        white = torch.empty((fields, N), dtype=torch.float32, device="cuda")
        out = torch.empty_like(white)

        def rows():
            if not eng.generate_grf_rows(fields, 3, 1 << 40, out):
                raise RuntimeError("generate_grf_rows answered False under grf_rows='all'")

        def two_calls():
            eng.normal_rows(white, N, 3, 1 << 40)
            eng.generate_grf(white, out=out)

        for fn in (rows, two_calls):
            window(fn, 3)
        ta, tb = [], []
        for _ in range(WINDOWS):
            ta.append(window(rows, a.reps))
            tb.append(window(two_calls, a.reps))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        verdict = "rows slower than the two calls by more than the spread" if ma - mb > spread else \
            ("rows faster by more than the spread" if mb - ma > spread else "within the spread")
        kind, param = eng.grf_generator()
        print(f"[{n}x{n}, {fields} fields, {FAMILY[kind]} ({param})] rows {ma:.4f} ms ({min(ta):.4f} .. {max(ta):.4f})   "
              f"fill + generate {mb:.4f} ms ({min(tb):.4f} .. {max(tb):.4f})   rows / two calls {ma / mb:.3f}: {verdict}")
        eng.close()


if __name__ == "__main__":
    main()
