"""Shared by the GPU tests of ipp_baseline_act on bare arrays: one launch from host arrays, everything read back."""
import ctypes as C

import numpy as np

RES, DTB, ALT_LO, ALT_HI, SPACING, STEP_SIZE, NUM_WAYPOINTS, SLOPE = 4, 4, 8, 14, 3, 8, 40, 10  # tests/golden/gen_golden_baselines.py
MAX_V, MAX_A = 2.0, 2.0


def baseline_launch(kind, prev, budget, episode=None, cursor=None, seen=None, decision=None, start=None, table=None, levels=None,
                    uniforms=None, grid=10, adaptive=False, flight=False, step_size=STEP_SIZE, low=None, high=None, seed=0, row_offset=0):
    """One ipp_baseline_act launch; returns a dict of host arrays: action, has, budget, cursor, seen, decision, start."""
    import torch
    from ipp_rl_amd import _ffi

    dev = torch.device("cuda:0")
    n = len(budget)

    def t(x, dtype, default):
        return torch.as_tensor(np.ascontiguousarray(default if x is None else x), dtype=dtype, device=dev)

    prev_t = t(prev, torch.float64, None)
    bud = t(budget, torch.float64, None)
    epi = t(episode, torch.int64, np.zeros(n))
    cur = t(cursor, torch.int32, np.zeros(n))
    sn = t(seen, torch.int64, np.zeros(n))
    dec = t(decision, torch.int64, np.zeros(n))
    st = t(start, torch.float64, np.full(n, -1.0))
    action = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
    has = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    keep = [torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev) if x is not None else None for x in (table, levels, uniforms)]
    d = _ffi.IppBaseline()
    d.n, d.kind, d.device = n, kind, 0
    d.table_len = 0 if table is None else len(table)
    d.grid_w = d.grid_h = grid
    d.n_levels = 0 if levels is None else len(levels)
    d.adaptive, d.use_flight_time = int(adaptive), int(flight)
    d.resolution, d.step_size, d.max_v, d.max_a = float(RES), float(step_size), MAX_V, MAX_A
    for c in range(3):
        d.low[c], d.high[c] = (0.0 if low is None else float(low[c])), (0.0 if high is None else float(high[c]))
    d.seed, d.row_offset = seed, row_offset
    d.table, d.levels, d.uniforms = [x.data_ptr() if x is not None else None for x in keep]
    d.prev, d.budget, d.episode = prev_t.data_ptr(), bud.data_ptr(), epi.data_ptr()
    d.cursor, d.seen_episode, d.decision, d.start_budget = cur.data_ptr(), sn.data_ptr(), dec.data_ptr(), st.data_ptr()
    d.action, d.has = action.data_ptr(), has.data_ptr()
    _ffi.check(_ffi.load().ipp_baseline_act(C.byref(d), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    return dict(action=action.cpu().numpy(), has=has.cpu().numpy(), budget=bud.cpu().numpy(), cursor=cur.cpu().numpy(), seen=sn.cpu().numpy(),
                decision=dec.cpu().numpy(), start=st.cpu().numpy())
