"""
The packed slot record of ipp_slots_export / ipp_slots_import (include/ipp_engine.h, "Slot export and import"; csrc/k_slots.h) in NumPy:
the CPU-testable definition of the format.  No device, no library.

A record = header (32 bytes) + the sections `what` selects, in this order; every part starts on a 16-byte boundary, padding is zero:

    header    uint32 magic, uint32 format, uint32 what, int32 rank r (0 without SLOT_COLUMNS), uint64 record bytes, int32 N, int32 pstride
    SLOT_COLUMNS   prior (2 float64) | colspan int32[r] | colrect int32[r] | columns float32[r][pstride]
    SLOT_MAPS      mean float32[N] | diag float32[N] | gt float32[N]

A slot is a dict of raw arrays: rank (int), prior (2 float64), colspan, colrect (int32 [rank]), columns (float32 [rank, pstride]), mean,
diag, gt (float32 [N]).  pack_slots_host writes the records of a list of slots back to back, unpack_slots_host reads them again, bit for
bit.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SLOT_COLUMNS, SLOT_MAPS = 1, 2
SLOT_FORMAT = 1
SLOT_MAGIC = 0x4C535049  # "IPSL"
SLOT_HEADER_BYTES = 32
SLOT_OK, SLOT_BAD_ID, SLOT_RANK, SLOT_BAD_RECORD = 0, 1, 2, 3
LAYOUT_FIELDS = ("format", "W", "H", "N", "Npad", "pw", "ph", "pstride", "window_rows", "tile_cells", "prior_kind")
_HEADER = np.dtype([("magic", "<u4"), ("format", "<u4"), ("what", "<u4"), ("rank", "<i4"), ("bytes", "<u8"), ("N", "<i4"), ("pstride", "<i4")])
assert _HEADER.itemsize == SLOT_HEADER_BYTES


def pad16(nbytes: int) -> int:
    return (int(nbytes) + 15) & ~15


def check_what(what: int) -> int:
    what = int(what)
    if what == 0 or what & ~(SLOT_COLUMNS | SLOT_MAPS):
        raise ValueError(f"what = {what:#x} selects no section or an unknown one")
    return what


def section_offsets(what: int, rank: int, n_cells: int, pstride: int) -> Dict[str, int]:
    """Byte offset of every part of a record from its start, and "end" = the record's bytes."""
    what, r = check_what(what), int(rank)
    out = {"header": 0}
    at = SLOT_HEADER_BYTES
    if what & SLOT_COLUMNS:
        out["prior"] = at
        at += 16
        out["colspan"] = at
        at += pad16(4 * r)
        out["colrect"] = at
        at += pad16(4 * r)
        out["columns"] = at
        at += 4 * r * int(pstride)
    if what & SLOT_MAPS:
        for name in ("mean", "diag", "gt"):
            out[name] = at
            at += pad16(4 * int(n_cells))
    out["end"] = at
    return out


def record_bytes(what: int, rank: int, n_cells: int, pstride: int) -> int:
    """Bytes of one record (ipp_slots_plan scans these): rank counts only with SLOT_COLUMNS."""
    return section_offsets(what, rank if int(what) & SLOT_COLUMNS else 0, n_cells, pstride)["end"]


def pack_slots_host(slots: Sequence[Dict], what: int, n_cells: int, pstride: int) -> Tuple[np.ndarray, np.ndarray]:
    """(blob uint8, offsets int64 [n + 1]) of the slots' records, as ipp_slots_plan + ipp_slots_export write them."""
    what, N, ps = check_what(what), int(n_cells), int(pstride)
    cols = bool(what & SLOT_COLUMNS)
    ranks = [int(s["rank"]) if cols else 0 for s in slots]
    sizes = [record_bytes(what, r, N, ps) for r in ranks]
    offsets = np.zeros(len(slots) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.asarray(sizes, dtype=np.int64))
    blob = np.zeros(int(offsets[-1]), dtype=np.uint8)

    def put(at, arr, dtype, count):
        a = np.ascontiguousarray(arr, dtype=dtype).reshape(-1)
        if a.size != count:
            raise ValueError(f"{a.size} values where the record holds {count}")
        blob[at:at + a.nbytes] = a.view(np.uint8)

    for s, r, o, size in zip(slots, ranks, offsets[:-1], sizes):
        o = int(o)
        off = section_offsets(what, r, N, ps)
        head = np.zeros(1, dtype=_HEADER)
        head["magic"], head["format"], head["what"], head["rank"] = SLOT_MAGIC, SLOT_FORMAT, what, r
        head["bytes"], head["N"], head["pstride"] = size, N, ps
        blob[o:o + SLOT_HEADER_BYTES] = head.view(np.uint8)
        if cols:
            put(o + off["prior"], s["prior"], "<f8", 2)
            put(o + off["colspan"], s["colspan"], "<i4", r)
            put(o + off["colrect"], s["colrect"], "<i4", r)
            put(o + off["columns"], s["columns"], "<f4", r * ps)
        if what & SLOT_MAPS:
            for name in ("mean", "diag", "gt"):
                put(o + off[name], s[name], "<f4", N)
    return blob, offsets


def read_header(blob: np.ndarray, offset: int) -> Dict[str, int]:
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    h = b[int(offset):int(offset) + SLOT_HEADER_BYTES].view(_HEADER)[0]
    return {k: int(h[k]) for k in _HEADER.names}


def unpack_slots_host(blob, offsets, what: Optional[int] = None) -> List[Dict]:
    """The slots of a blob: per record a dict with what, rank, N, pstride and the raw arrays of its sections (copies).  A record whose
    header is not this format's, whose size is not its rank's or which does not end at the next offset raises ValueError; what (if
    given) has to be every record's."""
    b = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    out = []
    for i in range(len(offs) - 1):
        o, end = int(offs[i]), int(offs[i + 1])
        if o % 16 or end < o + SLOT_HEADER_BYTES or end > b.size:
            raise ValueError(f"record {i}: offsets {o} .. {end} are not a record's inside a blob of {b.size} bytes")
        h = read_header(b, o)
        if h["magic"] != SLOT_MAGIC or h["format"] != SLOT_FORMAT:
            raise ValueError(f"record {i}: magic {h['magic']:#x}, format {h['format']}: not a slot record of format {SLOT_FORMAT}")
        if h["what"] == 0 and h["bytes"] == SLOT_HEADER_BYTES == end - o:  # (the export of an id outside the engine)
            out.append(dict(what=0, rank=0, N=h["N"], pstride=h["pstride"]))
            continue
        if what is not None and h["what"] != int(what):
            raise ValueError(f"record {i}: what = {h['what']:#x}, expected {int(what):#x}")
        w, r, N, ps = check_what(h["what"]), h["rank"], h["N"], h["pstride"]
        if r < 0 or h["bytes"] != end - o or h["bytes"] != record_bytes(w, r, N, ps):
            raise ValueError(f"record {i}: {h['bytes']} bytes in the header, {end - o} between its offsets, {record_bytes(w, max(r, 0), N, ps)} for rank {r}")
        off = section_offsets(w, r, N, ps)
        get = lambda name, dtype, count: b[o + off[name]:o + off[name] + count * np.dtype(dtype).itemsize].view(dtype).copy()  # noqa: E731
        s = dict(what=w, rank=r, N=N, pstride=ps)
        if w & SLOT_COLUMNS:
            s["prior"] = get("prior", "<f8", 2)
            s["colspan"], s["colrect"] = get("colspan", "<i4", r), get("colrect", "<i4", r)
            s["columns"] = get("columns", "<f4", r * ps).reshape(r, ps)
        if w & SLOT_MAPS:
            for name in ("mean", "diag", "gt"):
                s[name] = get(name, "<f4", N)
        out.append(s)
    return out


def check_layouts(mine: Dict, theirs: Dict):
    """ValueError naming the first fingerprint field (the format version first) in which two layouts differ."""
    for k in LAYOUT_FIELDS:
        if k not in theirs:
            raise ValueError(f"the packed slots' layout has no field {k!r}")
        if int(mine[k]) != int(theirs[k]):
            what = "format version" if k == "format" else f"layout field {k}"
            raise ValueError(f"packed slots of another {what}: {k} = {int(theirs[k])}, this engine has {int(mine[k])}")
