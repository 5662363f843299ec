"""
Ground-truth kinds of the reference (sensor.simulation.type, constants.py:74-89) and the fp64 NumPy copy of the device's hotspot and
split fields (csrc/k_fields.h).

A hotspot or split field is two values and at most two half-open rectangles {y0, y1, x0, x1} (y0 >= y1: empty), the engine's
ipp_field_record: cell (y, x) = inside if it lies in rect[0] or rect[1], else outside.

  * hotspot (simulations/simulations.py:56-90): outside = low, inside = high, rect[0] / rect[1] = the two clusters
  * split   (simulations/simulations.py:99-123): outside = second, inside = first, rect[0] = the first part, rect[1] empty

Device draws (ipp_generate_field_groups / ipp_generate_field_refill) take the Philox uniforms u_k = philox_uniform(row * 8 + k,
subsequence, seed) of a field's row (the GLOBAL env id) in the reference's draw order; draw_records() is their host copy, and the tests
hold the device to it bit for bit.  hotspot_record_numpy / split_record_numpy instead draw from NumPy's legacy global stream with the
reference's own calls (the drop-in HotspotRandomField / SplitRandomField).
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi

KINDS = {"gaussian_random_field": _ffi.IPP_FIELD_GRF, "hotspot_random_field": _ffi.IPP_FIELD_HOTSPOT,
         "split_random_field": _ffi.IPP_FIELD_SPLIT}
NAMES = {v: k for k, v in KINDS.items()}

# the engine's ipp_field_record (include/ipp_engine.h), 48 bytes
RECORD_DTYPE = np.dtype([("inside", "<f8"), ("outside", "<f8"), ("rect", "<i4", (2, 4))])


def field_kind(simulation: str) -> int:
    """IPP_FIELD_* of a sensor.simulation.type; ValueError for the kinds the engine does not generate."""
    if simulation == "temperature_data_field":
        raise ValueError("temperature_data_field is not supported: it needs the reference's temperature dataset (a file under "
                         "DATASETS_DIR that the reference does not ship) plus imageio and cv2 to read and resize it")
    if simulation not in KINDS:
        raise ValueError(f"unknown sensor.simulation.type {simulation!r}: one of {sorted(KINDS)} (or temperature_data_field)")
    return KINDS[simulation]


def _second_centre_bounds(c0, r: float, lo: int, dim: int):
    """Admissible second centres {c in [lo, dim) : |c - c0| > r}: the integers in [lo, left_end] and in [right_beg, dim)."""
    c0 = np.asarray(c0, dtype=np.float64)
    left_end = np.ceil(c0 - r).astype(np.int64) - 1
    right_beg = np.maximum(np.floor(c0 + r).astype(np.int64) + 1, lo)
    nl = np.maximum(0, left_end - lo + 1)
    nr = np.maximum(0, dim - right_beg)
    return nl, right_beg, nr


def check_hotspot(y_dim: int, x_dim: int, r: float) -> None:
    """ValueError where the reference's hotspot generator cannot run: trunc(r) >= a grid dimension (its randint raises), r < 0, or a
    first centre that leaves no second centre more than r away on an axis (its rejection loop, simulations/simulations.py:71-86, never
    ends), e.g. 10 x 10 with r = 5."""
    r = float(r)
    if not (r >= 0.0) or math.isinf(r):
        raise ValueError(f"hotspot_random_field: cluster_radius {r} must be finite and >= 0")
    for dim, axis in ((int(y_dim), "y_dim"), (int(x_dim), "x_dim")):
        lo = int(r)
        if lo >= dim:
            raise ValueError(f"hotspot_random_field: cluster_radius {r} >= {axis} = {dim} (the reference's randint(r, {dim}) raises)")
        nl, _, nr = _second_centre_bounds(np.arange(lo, dim), r, lo, dim)
        if np.any(nl + nr == 0):
            raise ValueError(f"hotspot_random_field: {axis} = {dim} with cluster_radius {r}: a first cluster centre can leave no second "
                             f"centre more than r away (the reference's rejection loop never ends)")


def _randint(lo, hi, u):
    """randint(lo, hi) from one uniform: lo + min(floor(u (hi - lo)), hi - lo - 1)."""
    span = np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64)
    return lo + np.minimum(np.floor(u * span.astype(np.float64)).astype(np.int64), span - 1)


def _cluster(c, r: float, dim: int):
    """int(max(c - r, 0)), int(min(c + r, dim)) in fp64 (simulations/simulations.py:63-66)."""
    c = np.asarray(c, dtype=np.float64)
    return np.trunc(np.maximum(c - r, 0.0)).astype(np.int32), np.trunc(np.minimum(c + r, float(dim))).astype(np.int32)


def draw_records(kind: int, y_dim: int, x_dim: int, cluster_radius: float, rows, subsequence, seed: int) -> np.ndarray:
    """Host copy of the device draws: the records of the fields of global row ids `rows` with the given subsequence(s) (broadcast)."""
    from .vec_env import philox_uniform

    rows = np.asarray(rows, dtype=np.int64)
    sub = np.broadcast_to(np.asarray(subsequence, dtype=np.int64), rows.shape)
    u = [philox_uniform(rows * 8 + k, sub, seed) for k in range(6)]
    H, W, r = int(y_dim), int(x_dim), float(cluster_radius)
    out = np.zeros(rows.shape, dtype=RECORD_DTYPE)
    if kind == _ffi.IPP_FIELD_HOTSPOT:
        check_hotspot(H, W, r)
        lo = int(r)
        high = 0.7 + (1.0 - 0.7) * u[0]
        low = 0.0 + (0.3 - 0.0) * u[1]
        yc, xc = _randint(lo, H, u[2]), _randint(lo, W, u[3])
        centres2 = []
        for c0, dim, uu in ((yc, H, u[4]), (xc, W, u[5])):
            nl, rb, nr = _second_centre_bounds(c0, r, lo, dim)
            j = _randint(0, nl + nr, uu)
            centres2.append(np.where(j < nl, lo + j, rb + (j - nl)))
        out["inside"], out["outside"] = high, low
        for q, (cy, cx) in enumerate(((yc, xc), tuple(centres2))):
            out["rect"][..., q, 0], out["rect"][..., q, 1] = _cluster(cy, r, H)
            out["rect"][..., q, 2], out["rect"][..., q, 3] = _cluster(cx, r, W)
    elif kind == _ffi.IPP_FIELD_SPLIT:
        high = 0.65 + (1.0 - 0.65) * u[0]
        low = 0.0 + (0.35 - 0.0) * u[1]
        swap, ysplit = u[2] > 0.5, u[3] > 0.5
        out["inside"] = np.where(swap, low, high)
        out["outside"] = np.where(swap, high, low)
        sy = _randint(int(np.ceil(H * 0.33)), int(np.ceil(H * 0.66)) + 1, u[4])
        sx = _randint(int(np.floor(W * 0.33)), int(np.ceil(W * 0.66)) + 1, u[4])
        out["rect"][..., 0, 1] = np.where(ysplit, sy, H)
        out["rect"][..., 0, 3] = np.where(ysplit, W, sx)
    else:
        raise ValueError(f"draw_records: field kind {kind} has no record (hotspot = {_ffi.IPP_FIELD_HOTSPOT}, split = {_ffi.IPP_FIELD_SPLIT})")
    return out


def fill(records, y_dim: int, x_dim: int) -> np.ndarray:
    """The fields of `records` as fp64 maps [..., y_dim, x_dim] (float32() of them is what the device writes)."""
    rec = np.asarray(records, dtype=RECORD_DTYPE)
    y = np.arange(int(y_dim))[:, None]
    x = np.arange(int(x_dim))[None, :]
    flat = rec.reshape(-1)
    out = np.empty((len(flat), int(y_dim), int(x_dim)))
    for i, f in enumerate(flat):
        inside = np.zeros((int(y_dim), int(x_dim)), dtype=bool)
        for y0, y1, x0, x1 in f["rect"]:
            inside |= (y >= y0) & (y < y1) & (x >= x0) & (x < x1)
        out[i] = np.where(inside, f["inside"], f["outside"])
    return out.reshape(rec.shape + (int(y_dim), int(x_dim)))


def hotspot_record_numpy(y_dim: int, x_dim: int, cluster_radius) -> np.ndarray:
    """The reference's HotspotRandomField.create_ground_truth_map (simulations/simulations.py:56-90) as a record: the same NumPy legacy
    stream calls in the same order, rejection loop included, so a seeded run consumes the stream exactly as the reference does.
    ValueError (before any draw) where the reference would loop forever or raise."""
    check_hotspot(y_dim, x_dim, cluster_radius)
    r = cluster_radius
    high = np.random.uniform(low=0.7, high=1)
    low = np.random.uniform(low=0.0, high=0.3)
    yc = np.random.randint(low=r, high=y_dim)
    xc = np.random.randint(low=r, high=x_dim)
    while True:
        yc2 = np.random.randint(low=r, high=y_dim)
        xc2 = np.random.randint(low=r, high=x_dim)
        if np.abs(yc2 - yc) <= r or np.abs(xc2 - xc) <= r:
            continue
        break
    rec = np.zeros((), dtype=RECORD_DTYPE)
    rec["inside"], rec["outside"] = high, low
    for q, (cy, cx) in enumerate(((yc, xc), (yc2, xc2))):
        rec["rect"][q] = (int(max(cy - r, 0)), int(min(cy + r, y_dim)), int(max(cx - r, 0)), int(min(cx + r, x_dim)))
    return rec


def split_record_numpy(y_dim: int, x_dim: int) -> np.ndarray:
    """The reference's SplitRandomField.create_ground_truth_map (simulations/simulations.py:99-123) as a record, drawn with its calls."""
    high = np.random.uniform(low=0.65, high=1)
    low = np.random.uniform(low=0.0, high=0.35)
    first, second = high, low
    if np.random.rand() > 0.5:
        first, second = low, high
    rec = np.zeros((), dtype=RECORD_DTYPE)
    rec["inside"], rec["outside"] = first, second
    if np.random.rand() > 0.5:
        s = np.random.randint(low=np.ceil(y_dim * 0.33), high=np.ceil(y_dim * 0.66) + 1)
        rec["rect"][0] = (0, s, 0, x_dim)
    else:
        s = np.random.randint(low=np.floor(x_dim * 0.33), high=np.ceil(x_dim * 0.66) + 1)
        rec["rect"][0] = (0, y_dim, 0, s)
    return rec
