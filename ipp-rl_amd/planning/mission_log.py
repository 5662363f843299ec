"""
Metric curves per env and the planner comparison on the device (the reference's experiments/experiments.py:178-236: every mission type on
the same maps, the map metrics after every executed waypoint -- Mission.eval, planning/missions.py:176-203 -- against the cumulative flight
time, np.interp onto one axis, mean and spread per planner).

MissionLog(env, capacity) sits behind ANY batched planner: record() after every env step appends (cumulative flight time, ipp_metrics) for
the envs that executed a waypoint (ipp_curve_record), curves() resamples and reduces (ipp_curve_resample / ipp_curve_reduce,
csrc/k_curves.h).  Between the first record() and curves() nothing is read from the device; curves() reads ONE number, the largest
flight time, to size the axis as experiments.py:227-228 does.

An env's curve is that of ONE mission: once the env's ledger reports `done`, its later steps are not recorded (reset() starts over).
"""
import ctypes as C
from typing import Dict, Optional

import numpy as np

from .. import _ffi
from .vec_baselines import curve_axis

VALUES, POINT = _ffi.IPP_CURVE_VALUES, _ffi.IPP_CURVE_POINT
METRIC_NAMES = ("rmse", "masked_rmse", "wrmse", "mll", "wmll", "trace", "masked_trace", "uncertainty_difference")  # ipp_metrics' order


class MissionLog:
    def __init__(self, env, capacity: int):
        """env: a VecIPPEnv (parts == 1).  capacity: points per env, the step-0 point included; a point beyond it is dropped and sets
        the env's overflow flag."""
        if not hasattr(env, "engine") or not hasattr(env, "prev"):
            raise TypeError("env must be a VecIPPEnv")
        if int(capacity) < 1:
            raise ValueError("capacity < 1")
        torch = env.torch
        self.env, self.torch, self.capacity = env, torch, int(capacity)
        B, dev = env.num_envs, env.device
        self.log = torch.zeros((B, self.capacity, POINT), dtype=torch.float64, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.ended = torch.zeros(B, dtype=torch.bool, device=dev)
        self.metrics = torch.zeros((B, VALUES), dtype=torch.float32, device=dev)
        self._max_x = torch.zeros(1, dtype=torch.float64, device=dev)
        self.started = False

    def reset(self):
        self.count.zero_(); self.overflow.zero_(); self.ended.zero_()
        self.started = False

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.env.device).cuda_stream)

    def record(self, prev_before=None, actions=None, executed=None, first: bool = False):
        """After an env step: one point for every env with executed[e] that has not ended before this step -- time += flight time from
        prev_before[e] to actions[e], values = the env's metrics now.  first=True: the step-0 point (time 0) of every env, before the
        first step.  All arguments are device tensors; nothing is read back."""
        env, torch = self.env, self.torch
        if getattr(env, "parts", 1) > 1:
            env.wait()
        B = env.num_envs
        if first:
            a = p = ex = None
        else:
            a = actions.to(device=env.device, dtype=torch.float64).contiguous()
            p = prev_before.to(device=env.device, dtype=torch.float64).contiguous()
            ex = (executed.to(device=env.device).bool() & ~self.ended).to(torch.uint8)
            if tuple(a.shape) != (B, 3) or tuple(p.shape) != (B, 3) or tuple(ex.shape) != (B,):
                raise ValueError("record: actions and prev_before [B, 3], executed [B]")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        _ffi.check(_ffi.load().ipp_curve_record(env.engine._h, ptr(self.metrics), ptr(a), ptr(p), ptr(ex), B, 1 if first else 0,
                                                float(env.cfg.max_v), float(env.cfg.max_a), ptr(self.log), ptr(self.count),
                                                ptr(self.overflow), self.capacity, env.device.index or 0, self._stream()))
        if not first and getattr(env, "budget_mode", False):
            self.ended |= env.done.bool()
        self.started = True

    def curves(self, budget: float) -> Dict:
        """The comparison curves on the axis of experiments.py:227-228 -- max_x = min(largest flight time, budget), G = int(ceil(max_x))
        points of np.linspace(0, max_x, G): dict(axis [G], per_env [B, G, 8], mean [G, 8], sd [G, 8] (ddof = 1), overflow [B], max_x_all).
        Device tensors but for max_x_all, the one number read from the device."""
        env, torch = self.env, self.torch
        lib, B, dev = _ffi.load(), env.num_envs, env.device.index or 0
        _ffi.check(lib.ipp_curve_extent(self.log.data_ptr(), self.count.data_ptr(), B, self.capacity, self._max_x.data_ptr(), dev, self._stream()))
        max_x_all = float(self._max_x.item())
        max_x, G = curve_axis(max_x_all, budget)
        per_env = torch.empty((B, G, VALUES), dtype=torch.float64, device=env.device)
        mean = torch.empty((G, VALUES), dtype=torch.float64, device=env.device)
        sd = torch.empty_like(mean)
        _ffi.check(lib.ipp_curve_resample(self.log.data_ptr(), self.count.data_ptr(), B, self.capacity, max_x, G, per_env.data_ptr(), dev,
                                          self._stream()))
        _ffi.check(lib.ipp_curve_reduce(per_env.data_ptr(), B, G, mean.data_ptr(), sd.data_ptr(), dev, self._stream()))
        axis = torch.as_tensor(np.linspace(0, max_x, G), device=env.device)
        return dict(axis=axis, per_env=per_env, mean=mean, sd=sd, overflow=self.overflow.clone(), max_x_all=max_x_all)


def compare(planners: Dict, steps: int, budget: float, capacity: Optional[int] = None) -> Dict:
    """"Which planner wins on this scenario" for a batch: for every named planner (any object with .env, a budget-mode VecIPPEnv with
    parts == 1, and act() -> (actions, has)) reset its env (the planner's own reset() where it has one), run `steps` decisions and env
    steps with a MissionLog behind them, and collect curves(budget).  The steps run without the in-launch reset (auto_reset=False): the
    metrics of an episode's last waypoint are those of the map it was flown on, and an ended env idles with budget 0.  No plotting."""
    out = {}
    for name, planner in planners.items():
        env = planner.env
        (planner.reset if hasattr(planner, "reset") else env.reset)()
        log = MissionLog(env, int(capacity) if capacity else int(steps) + 1)
        log.record(first=True)
        for _ in range(int(steps)):
            prev_before = env.prev.clone()
            actions, has = planner.act()
            env.step(actions, auto_reset=False)
            log.record(prev_before, actions, has)
        out[name] = log.curves(budget)
    return out
