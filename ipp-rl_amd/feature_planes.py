"""
Host side of the batched NN input feature planes (ipp_feature_planes, include/ipp_engine.h): the plane spec, the entry
record and its packing.

A request is one history of ``spec.history`` entries, newest first, like ``EpisodeHistory.states`` of
planning/common/features.py.  An entry names a state instead of holding it: an env slot, how many of its factor columns
(``rank``, -1 = all: the slot's current state; a smaller rank is an earlier state of the same episode) and a tree path
below it, plus the waypoint and the normalised budget pushed with it.  Entries live on the device as int32 [n, H, 18]
(72 bytes each, the C struct); ``entry_tensor`` packs host records, ``ENTRY_WORDS`` / ``POS_F64`` / ``BUDGET_F64`` let
device code fill them with torch ops.
"""
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import _ffi

TREE_DEPTH = 6
ENTRY_DTYPE = np.dtype([("root_env", np.int32), ("rank", np.int32), ("path", np.int32, (TREE_DEPTH,)), ("valid", np.int32),
                        ("reserved", np.int32), ("position", np.float64, (3,)), ("budget", np.float64)], align=True)
ENTRY_WORDS = ENTRY_DTYPE.itemsize // 4  # 18 int32 words per entry
PATH_W, VALID_W = 2, 8                   # int32 word of path[0] / valid
POS_F64, BUDGET_F64 = 5, 8               # float64 word of position[0] / budget
assert ENTRY_DTYPE.itemsize == 72 and ENTRY_DTYPE.fields["position"][1] == 8 * POS_F64 and ENTRY_DTYPE.fields["budget"][1] == 8 * BUDGET_F64


@dataclass(frozen=True)
class PlaneSpec:
    """generate_input_feature_planes' options: use_fov = min / max altitude None (FoV mode), use_costs =
    use_action_costs_input (position mode only), adaptive = adaptive_info given, use_flight_time = uav_specifications given."""
    history: int
    use_fov: bool = False
    use_costs: bool = False
    adaptive: bool = True
    use_flight_time: bool = True
    min_altitude: float = 0.0
    max_altitude: float = 0.0

    def __post_init__(self):
        if int(self.history) < 1 or int(self.history) > 64:
            raise ValueError(f"history = {self.history} outside [1, 64]")
        if not self.use_fov and not (np.isfinite(self.min_altitude) and np.isfinite(self.max_altitude) and self.max_altitude != self.min_altitude):
            raise ValueError("position mode needs finite min_altitude != max_altitude (use_fov=True for the FoV planes)")

    @property
    def per_entry(self) -> int:
        return 3 if self.use_fov else 5

    @property
    def channels(self) -> int:
        """C: 3H (FoV), 5H (position), 5H + 1 (position with the cost plane)."""
        return self.per_entry * self.history + (1 if self.use_costs and not self.use_fov else 0)

    def channel_names(self):
        per = ["state", "fov", "budget"] if self.use_fov else ["state", "x", "y", "z", "budget"]
        names = [f"{p}[{h}]" for h in range(self.history) for p in per]
        return names + (["cost"] if self.channels > len(names) else [])

    @classmethod
    def from_params(cls, hyper_params: Dict, meta_data: Dict, adaptive: bool = True, use_flight_time: bool = True) -> "PlaneSpec":
        """The spec the reference's MCTS / episode generator use (mcts.py:184-197, episode_generators.py:170-182)."""
        fov = bool(hyper_params["use_fov_input"])
        return cls(history=int(hyper_params["input_history_length"]), use_fov=fov,
                   use_costs=bool(hyper_params.get("use_action_costs_input", False)), adaptive=adaptive, use_flight_time=use_flight_time,
                   min_altitude=0.0 if fov else float(meta_data["min_altitude"]), max_altitude=0.0 if fov else float(meta_data["max_altitude"]))

    def to_c(self) -> "_ffi.IppPlaneSpec":
        return _ffi.IppPlaneSpec(history=int(self.history), use_fov=int(bool(self.use_fov)), use_costs=int(bool(self.use_costs)),
                                 adaptive=int(bool(self.adaptive)), use_flight_time=int(bool(self.use_flight_time)), reserved=0,
                                 min_altitude=float(self.min_altitude), max_altitude=float(self.max_altitude))


def make_entry(root_env: int, position, budget: float, rank: int = -1, path: Optional[Sequence[int]] = None) -> np.ndarray:
    """One valid entry (a 0-d record of ENTRY_DTYPE)."""
    e = np.zeros((), dtype=ENTRY_DTYPE)
    p = [] if path is None else [int(x) for x in path if int(x) >= 0]
    if len(p) > TREE_DEPTH:
        raise ValueError(f"path of {len(p)} nodes > {TREE_DEPTH}")
    e["root_env"], e["rank"], e["valid"] = int(root_env), int(rank), 1
    e["path"] = p + [-1] * (TREE_DEPTH - len(p))
    e["position"] = np.asarray(position, dtype=np.float64).reshape(3)
    e["budget"] = float(budget)
    return e


def pack_entries(histories: Sequence[Sequence[np.ndarray]], history: int) -> np.ndarray:
    """[n, H] records from n histories of make_entry records, newest first; shorter histories are zero padded."""
    out = np.zeros((len(histories), history), dtype=ENTRY_DTYPE)
    for i, h in enumerate(histories):
        if len(h) > history:
            raise ValueError(f"history {i} has {len(h)} entries > H = {history}")
        for j, e in enumerate(h):
            out[i, j] = e
    out["path"][out["valid"] == 0] = -1
    return out


def entry_tensor(records: np.ndarray, device):
    """ENTRY_DTYPE records [n, H] -> device int32 [n, H, 18]."""
    import torch

    arr = np.ascontiguousarray(records, dtype=ENTRY_DTYPE)
    words = arr.view(np.int32).reshape(arr.shape + (ENTRY_WORDS,))
    return torch.as_tensor(words.copy(), device=device)


def entry_records(t) -> np.ndarray:
    """device int32 [n, H, 18] -> ENTRY_DTYPE records [n, H] (host)."""
    words = np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int32, copy=False))
    return words.reshape(-1, ENTRY_WORDS).view(ENTRY_DTYPE).reshape(words.shape[:-1])


def empty_entries(n: int, history: int, device):
    """All-padding device entries [n, H, 18] (path -1)."""
    import torch

    t = torch.zeros((n, history, ENTRY_WORDS), dtype=torch.int32, device=device)
    t[:, :, PATH_W:PATH_W + TREE_DEPTH] = -1
    return t


def check_entries(entries, history: int):
    if str(entries.dtype) != "torch.int32" or entries.dim() != 3 or entries.shape[1] != history or entries.shape[2] != ENTRY_WORDS:
        raise ValueError(f"entries must be int32 [n, {history}, {ENTRY_WORDS}], got {tuple(entries.shape)} {entries.dtype}")

