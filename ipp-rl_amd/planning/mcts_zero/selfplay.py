"""
SelfPlay: the reference's self-play loop (planning/mcts_zero/episode_generators.py:102-184 -- there one EpisodeGenerator per episode and
CPU worker, mcts_zero_mission.py:71-83) for a whole batch of budget-mode envs on one device, and ReplayBuffer: its training samples
(input_feature_planes, policy, value, reward, valid_actions_msk) kept in device memory and served as minibatches like
replay_buffers.py:58-101 serves the bz2 pickles.

One SelfPlay.step() is one iteration of the reference's episode loop for every env:

    planes    VecIPPEnv.feature_planes of each env's history (the pushed states of this episode, masked with the PRE-step mean: what
              adaptive_info_history[i] holds, :133) straight into the env's ring row                                   (ipp_feature_planes)
    search    DeviceMCTS on the env slots as roots, root depth 0 (:121-128); the read-out on the device (ipp_mcts_policy) for every
              action count, at temperature_scale and, where a temperature-0 step can occur, at 1 (its arg-max)
    record    temperature 0: one-hot arg-max (mcts.py:134-138); the action by the inverse CDF of the policy (np.random.choice, :135);
              the sparse policy and valid set into the row; a root without a policy ends its episode (:130-131)  (ipp_selfplay_record)
    step      VecIPPEnv.step: the fused budget step, episode ends and resets in the same launch (:137-150)
    commit    the rewards; for every episode that ended its windowed value targets (:158-164), the rows become sampleable; the next
              episode's first waypoint (sample_init_action, :51)                                                     (ipp_selfplay_commit)

Nothing in the loop reads the device from the host beyond the search's one count read-back per wave of simulations.

Draws (include/ipp_engine.h, IPP_SP_*_STREAM): the loop's own draws are Philox4x32-10 uniforms keyed on (seed, global env id, episode,
depth); the search's draws (Dirichlet noise, random tie breaks: k_mcts.h hashes) are keyed on env_id_offset + root; so N shards with
contiguous env_id_offset produce the samples of one process.  Minibatch draws are keyed on the buffer's draw count and the draw index.  Ring: S step slots of B rows, the sample of env e at step t in row
(t mod S) B + e; S > max_episode_steps keeps every row of a running episode.  Replay minibatches: ReplayBuffer.sample (uniform,
ExperienceReplayBuffer) and ReplayBuffer.prioritized (PrioritizedExperienceReplayBuffer, replay_buffers.py:104-141: priorities, their
prefix sums, the draws, the importance-sampling weights and the priority updates all in device memory; a trainer's use_per selects it,
the episode loop has no use for the switch and check_args refuses it).

Iterations of the learn loop (mcts_zero_mission.py:305-362: `num_episodes` episodes per worker and iteration, their samples under
train_data/iter_{i}; ReplayBuffer(self_play_iteration, window_size), replay_buffers.py:34-46): SelfPlay.begin_iteration / step_iteration /
run_iteration commit with ipp_selfplay_commit_iter -- every env keeps `episodes_per_env` episodes per iteration, their rows tagged with
the iteration in ReplayBuffer.iter, later episodes are played out and dropped -- and read the iteration's totals record
(ipp_selfplay_iter_totals) from pinned memory, the step's one new read.  ReplayBuffer.window(lo, hi) serves a Trainer the rows of
iterations lo .. hi (planning/mcts_zero/learn.py).

The compact ring (planes="compact"; csrc/k_replay_compact.h): a row's planes are a function of its episode's factor columns, a few scalars
per history entry and the mean at record time, so the row keeps those (ipp_replay_record_compact, where `planes` is above), an ended
episode's columns are copied once into a spare engine slot between `step` and `commit` (ipp_selfplay_archive: the predicate is read on the
device) and a minibatch builds the planes of its rows (ipp_replay_compact_planes).  Same draws, same seven outputs; bit-identical to the
dense ring with interval_factor = 0, and with interval_factor != 0 the newest state's mask takes the densified diagonal of its column
prefix where the dense ring takes the slot's incrementally stored one (two fp32 evaluations of the same P_ii).

Divergences from the reference (INTEGRATION.md "Batched self-play"): a temperature-0 sample stores the real valid-action mask where the
reference stores the visit counts (mcts.py:138); no tree reuse between steps, no per-episode shuffled priors; the draws are counter-based,
not NumPy's global stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional

import numpy as np

from ... import _ffi
from ...vec_env import VecIPPEnv, philox_uniform

PENDING, COMMITTED = 1, 2
ACTION_STREAM, INIT_STREAM, TIE_STREAM = _ffi.IPP_SP_ACTION_STREAM, _ffi.IPP_SP_INIT_STREAM, _ffi.IPP_SP_TIE_STREAM
ARGMAX_STREAM, REPLAY_STREAM = _ffi.IPP_SP_ARGMAX_STREAM, _ffi.IPP_REPLAY_STREAM
MAX_DEPTH = 1 << 20  # (the depth is the low 20 bits of a step draw's counter)
MAX_KMAX = 2048      # widest valid set a ring row holds (csrc/k_selfplay.h kSpMaxK)


# ---------------------------------------------------------------------------------------------------- host restatements
def step_counter(global_env_ids, depth) -> np.ndarray:
    """Philox counter of an env's per-step draws: (global env id << 20) + depth."""
    return (np.asarray(global_env_ids, dtype=np.int64) << 20) + np.asarray(depth, dtype=np.int64)


def step_uniform(stream: int, seed: int, global_env_ids, episode, depth) -> np.ndarray:
    """The uniform an env draws at (episode, depth) from `stream` (ACTION_STREAM, TIE_STREAM, ARGMAX_STREAM)."""
    return philox_uniform(step_counter(global_env_ids, depth), stream + np.asarray(episode, dtype=np.int64), seed)


def init_action_index(seed: int, global_env_ids, episode, num_actions: int) -> np.ndarray:
    """First waypoint (action index) of an episode: sample_init_action (episode_generators.py:60-62) from INIT_STREAM."""
    u = philox_uniform(np.asarray(global_env_ids, dtype=np.int64), INIT_STREAM + np.asarray(episode, dtype=np.int64), seed)
    return np.minimum((u * num_actions).astype(np.int64), num_actions - 1)


def inverse_cdf(policy, u: float) -> int:
    """np.random.choice(len(policy), p=policy) at the uniform u: the first index whose normalised cumulative sum exceeds u."""
    cdf = np.cumsum(np.asarray(policy, dtype=np.float64))
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, u, side="right"))


def value_targets(rewards, gamma: float, horizon: int):
    """(targets, total_episode_value) of one episode: value_i = scale_value_target(sum_{j=i}^{min(i+horizon,T)-1} gamma^j r_j) with the
    ABSOLUTE step j as exponent, the reference's own form (episode_generators.py:158-164; a discount relative to i would be gamma^(j-i))."""
    r = [float(x) for x in rewards]
    T = len(r)
    out = np.empty(T)
    for i in range(T):
        v = 0.0
        for j in range(i, min(i + horizon, T)):
            v += gamma ** j * r[j]
        out[i] = np.sqrt(1 + v) - 1
    tot = 0.0
    for j in range(T):
        tot += gamma ** j * r[j]
    return out, tot


def replay_draws(n: int, copies: int, seed: int, draw: int, committed_rows: np.ndarray):
    """Rows and shift offsets of minibatch number `draw` (ipp_replay_gather): draw i picks committed_rows[floor(u_i total)] (ascending
    row order), copy c >= 1 is shifted by (i, j) in [0, 8]^2, copy 0 is (4, 4) = unshifted."""
    sub = REPLAY_STREAM + int(draw)
    total = len(committed_rows)
    u = philox_uniform(np.arange(n, dtype=np.int64), sub, seed)
    pick = np.minimum((u * total).astype(np.int64), total - 1)
    rows = np.asarray(committed_rows, dtype=np.int64)[pick]
    offs = np.full((copies, 2), 4, dtype=np.int64)
    for c in range(1, copies):
        for w in range(2):
            uo = philox_uniform((1 << 32) + 2 * c + w, sub, seed)
            offs[c, w] = min(int(uo * 9.0), 8)
    return rows, offs


def per_uniforms(n: int, seed: int, draw: int) -> np.ndarray:
    """The n uniforms of minibatch number `draw`, prioritised or uniform: counter i of subsequence REPLAY_STREAM + draw."""
    return philox_uniform(np.arange(n, dtype=np.int64), REPLAY_STREAM + int(draw), seed)


def per_mass(priorities, committed, alpha: float) -> np.ndarray:
    """priorities ** alpha (replay_buffers.py:126) on the rows that are committed and hold a finite positive priority, 0 elsewhere."""
    p = np.asarray(priorities, dtype=np.float64)
    ok = np.asarray(committed, dtype=bool) & np.isfinite(p) & (p > 0)
    mass = np.zeros(p.shape)
    mass[ok] = p[ok] ** float(alpha)
    return mass


def per_probabilities(mass) -> np.ndarray:
    """`probabilities /= probabilities.sum()` (:127)."""
    mass = np.asarray(mass, dtype=np.float64)
    return mass / mass.sum()


def per_rows(mass, u) -> np.ndarray:
    """np.random.choice(len(mass), p=probabilities) (:129) at the uniforms u: cdf = cumsum(p), cdf /= cdf[-1], cdf.searchsorted(u,
    side="right"); past the last row with mass (rounding): that row; no mass at all: -1."""
    mass, u = np.asarray(mass, dtype=np.float64), np.atleast_1d(np.asarray(u, dtype=np.float64))
    if not mass.sum() > 0:
        return np.full(u.shape, -1, dtype=np.int64)
    cdf = np.cumsum(per_probabilities(mass))
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, u, side="right"), np.nonzero(mass > 0)[0][-1]).astype(np.int64)


def per_weights(mass, rows, committed_count: int, beta: float) -> np.ndarray:
    """(probabilities[rows] * L) ** -beta over its maximum, float32 (:135-136); NaN for a row of -1."""
    rows = np.asarray(rows, dtype=np.int64)
    if np.any(rows < 0):
        return np.full(rows.shape, np.nan, dtype=np.float32)
    w = (per_probabilities(mass)[rows] * committed_count) ** (-float(beta))
    return np.array(w / w.max(), dtype=np.float32)


def per_beta_step(beta: float, beta0: float, total_steps: int) -> float:
    """PrioritizedExperienceReplayBuffer.step (:122-123)."""
    return float(np.minimum(beta + (1 - beta0) / total_steps, 1))


def per_update(priorities, indices, values) -> np.ndarray:
    """`self.priorities[indices] = priorities` (:140-141) on a copy: the last occurrence of a repeated index wins, -1 is skipped."""
    out = np.array(priorities, dtype=np.float64)
    idx, val = np.asarray(indices, dtype=np.int64).reshape(-1), np.asarray(values, dtype=np.float64).reshape(-1)
    for i, v in zip(idx, val):  # (in order, so that the last one stays)
        if 0 <= i < len(out):
            out[i] = v
    return out


def shift_planes(states: np.ndarray, offset) -> np.ndarray:
    """ReplicationPad2d(4) followed by the crop at (i, j) of the original size (RandomCrop with one offset for the whole 4-D batch)."""
    i, j = int(offset[0]), int(offset[1])
    h, w = states.shape[-2:]
    pad = np.pad(states, [(0, 0)] * (states.ndim - 2) + [(4, 4), (4, 4)], mode="edge")
    return pad[..., i:i + h, j:j + w]


def commit_iter_host(state: Dict, step: int, it: Dict) -> Dict:
    """ipp_selfplay_commit_iter on NumPy arrays.  state: the ring and env fields in front of the commit (B, S, A, gamma, horizon,
    random_init, seed, row_offset; reward, forced, done, ep_len, episode, depth, actions, prev, r_reward, r_value, r_flags); it:
    iteration, episode_cap, iter_episodes, r_iter, examples, value_sum.  Returns what the call leaves: r_reward, r_value, r_flags, ep_len,
    prev, episode_value (NaN: nothing ended), forced, tie_u and iter_episodes, r_iter, examples, value_sum.  An episode that ends is
    kept while the env has fewer than episode_cap ended episodes in this iteration: targets, tag, then the committed flag, examples += T,
    value_sum += total_episode_value; past the cap its rows get flag 0 and nothing else; either way it counts (T = 0 too)."""
    B, S, A = int(state["B"]), int(state["S"]), int(state["A"])
    out = {k: np.array(state[k]) for k in ("r_reward", "r_value", "r_flags", "ep_len", "prev")}
    out.update(iter_episodes=np.array(it["iter_episodes"], dtype=np.int32), r_iter=np.array(it["r_iter"], dtype=np.int32),
               examples=np.array(it["examples"], dtype=np.int64), value_sum=np.array(it["value_sum"], dtype=np.float64))
    out["episode_value"] = np.full(B, np.nan)
    out["forced"] = np.zeros(B, np.uint8)
    gid = np.arange(B, dtype=np.int64) + int(state["row_offset"])
    cap, iteration = int(it["episode_cap"]), int(it["iteration"])
    for e in range(B):
        forced = bool(state["forced"][e])
        if not forced:
            out["r_reward"][(step % S) * B + e] = float(state["reward"][e])
        if not (forced or state["done"][e]):
            continue
        T = int(state["ep_len"][e])
        t_last = step - 1 if forced else step
        rows = np.array([((t_last - (T - 1 - j)) % S) * B + e for j in range(T)], dtype=np.int64)
        vals, tot = value_targets(out["r_reward"][rows], state["gamma"], state["horizon"])
        if out["iter_episodes"][e] < cap:
            out["r_value"][rows], out["r_iter"][rows], out["r_flags"][rows] = vals, iteration, COMMITTED
            out["examples"][e] += T
            out["value_sum"][e] += tot
        else:
            out["r_flags"][rows] = 0
        out["iter_episodes"][e] += 1
        out["episode_value"][e], out["ep_len"][e] = tot, 0
        if state["random_init"]:
            out["prev"][e] = state["actions"][int(init_action_index(state["seed"], gid[e], int(state["episode"][e]), A))]
    out["tie_u"] = step_uniform(TIE_STREAM, state["seed"], gid, state["episode"], state["depth"])
    return out


def scan_order_sum(values) -> float:
    """The fp64 sum of ipp_selfplay_iter_totals, in its order (that of ipp_replay_mass's scan of the tile sums): chunks of 256 values in
    ascending order, zeros behind the last; in a chunk each wave of 64 runs a shuffle scan (for o = 1, 2, .. 32: v[l] += v[l - o]) whose
    last lane holds the wave's sum, the four wave sums are added in wave order to 0, and the chunks' totals in chunk order to 0."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    carry = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, len(v), 256):
            chunk = np.zeros(256)
            chunk[:len(v[c0:c0 + 256])] = v[c0:c0 + 256]
            tot = np.float64(0.0)
            for w in range(4):
                x = chunk[64 * w:64 * w + 64].copy()
                o = 1
                while o < 64:
                    x[o:] = x[o:] + x[:-o]  # (the right-hand side is evaluated before the assignment: every lane adds the old value)
                    o *= 2
                tot = tot + x[63]
            carry = carry + tot
    return float(carry)


def iter_totals_host(iter_episodes, examples, value_sum, episode_cap: int) -> Dict:
    """ipp_selfplay_iter_totals: episodes_kept = sum min(iter_episodes, cap), envs_at_cap = #(iter_episodes >= cap), examples = the sum
    of the kept rows, value_sum = scan_order_sum of the envs' value sums."""
    n = np.asarray(iter_episodes, dtype=np.int64)
    return dict(episodes_kept=int(np.minimum(n, int(episode_cap)).sum()), envs_at_cap=int((n >= int(episode_cap)).sum()),
                examples=int(np.asarray(examples, dtype=np.int64).sum()), value_sum=scan_order_sum(value_sum))


def window_rows_host(flags, r_iter, lo: int, hi: int) -> np.ndarray:
    """Ascending ring rows of the off-policy window [lo, hi] (ReplayBuffer(self_play_iteration, window_size), replay_buffers.py:34-46):
    committed and tagged with an iteration inside it.  ipp_replay_priority_reset_window gives these L rows 1 / L and every other row 0."""
    f, t = np.asarray(flags), np.asarray(r_iter, dtype=np.int64)
    return np.nonzero((f == COMMITTED) & (t >= int(lo)) & (t <= int(hi)))[0].astype(np.int64)


def check_args(hyper_params: Dict, meta_data: Dict, num_envs: int, capacity: Optional[int], episode_priors: Optional[str] = None):
    """What SelfPlay cannot run, refused before anything touches the device.  Returns (slots S, max_episode_steps).
    episode_priors: None (a true hyper_params["shuffle_prior_cov"] raises) or "device" (it selects the env's device-drawn per-episode
    priors, VecIPPEnv(shuffle_prior_cov="device"))."""
    if episode_priors is not None and episode_priors != "device":
        raise ValueError(f"episode_priors = {episode_priors!r}: None or 'device'")
    if meta_data.get("initial_budget") is None:
        raise ValueError("self-play runs budget-mode episodes: meta_data['initial_budget'] is needed")
    if not hyper_params.get("reset_mcts_each_step", True):
        raise ValueError("reset_mcts_each_step=False (tree reuse across steps) is not supported")
    if hyper_params.get("use_per", False):
        raise ValueError("use_per=True is the trainer's switch, not the episode loop's: it is not supported here; draw prioritised "
                         "minibatches with SelfPlay.replay.prioritized(...) (ReplayBuffer.prioritized)")
    if hyper_params.get("shuffle_prior_cov", False) and episode_priors is None:
        raise ValueError("shuffle_prior_cov=True (per-episode shuffled priors) needs the opt-in episode_priors='device': the priors are then "
                         "drawn per episode from the device's Philox streams (vec_env.start_prior) -- the reference's distribution, "
                         "U(0.8, 1.2) x nominal, but not the values of NumPy's global stream")
    steps = int(meta_data.get("max_episode_steps", hyper_params.get("max_episode_steps", 0)))
    if steps < 1 or steps >= MAX_DEPTH:
        raise ValueError(f"max_episode_steps = {steps} outside [1, 2^20)")
    B = int(num_envs)
    if B < 1:
        raise ValueError("num_envs must be >= 1")
    cap = int(capacity) if capacity is not None else B * (steps + 1)
    if cap % B:
        raise ValueError(f"capacity {cap} is not a multiple of num_envs {B} (the ring holds S step slots of num_envs rows)")
    S = cap // B
    if S < steps + 1:
        raise ValueError(f"capacity {cap} = {S} step slots of {B} rows: at least max_episode_steps + 1 = {steps + 1} slots are needed")
    return S, steps


def check_replay_mode(planes, archive_episodes, slots: int) -> int:
    """The ring's plane mode: True (dense planes), False (none) or "compact" (entries + mean per row, the planes built when a minibatch
    is drawn).  Returns E, the episodes archived per env in compact mode (archive_episodes; None: the ring's step slots S, with which
    nothing is ever evicted), 0 in the other modes.  Refused before anything touches a device."""
    if not any(planes is m for m in (True, False)) and planes != "compact":
        raise ValueError(f"planes = {planes!r}: True, False or 'compact'")
    if archive_episodes is not None and int(archive_episodes) < 1:
        raise ValueError(f"archive_episodes = {archive_episodes} < 1")
    if planes != "compact":
        return 0
    return int(slots) if archive_episodes is None else int(archive_episodes)


def archive_slot(num_envs: int, archive_episodes: int, env, episode):
    """Engine slot that archives episode `episode` (the count of the env's episodes that ended before it) of env `env`: the spare
    slots follow the env slots, E per env (ipp_replay_compact, include/ipp_engine.h)."""
    return int(num_envs) + np.asarray(env, dtype=np.int64) * int(archive_episodes) + np.asarray(episode, dtype=np.int64) % int(archive_episodes)


def archive_slots_in_use(episodes, num_envs: int, archive_episodes: int) -> np.ndarray:
    """Ascending engine slots of a compact ring that hold an archived episode: slot num_envs + e E + j does iff j < min(E, episodes[e])
    (env e has archived episodes[e] episodes, episode p into place p mod E).  What a ring's state_dict exports, from one read of
    `episodes`."""
    epi = np.asarray(episodes, dtype=np.int64).reshape(-1)
    B, E = int(num_envs), int(archive_episodes)
    if len(epi) != B:
        raise ValueError(f"{len(epi)} episode counters for {B} envs")
    j = np.arange(E, dtype=np.int64)[None, :]
    used = j < np.minimum(epi, E)[:, None]
    slots = B + np.arange(B, dtype=np.int64)[:, None] * E + j
    return slots[used].astype(np.int64)


def eviction_host(trace, slots: int, archive_episodes: int):
    """ipp_selfplay_archive's eviction and the ring's committed rows on a host trace of ONE env: trace[t] = (episode tag of the env's
    running episode at step t, recorded: the step left a sample, ended: the episode ended in step t).  Row t mod S takes the sample of
    step t (flag pending, tag = the episode; a step without a sample clears the row).  When episode p ends, the rows still flagged and
    tagged p - E lose their flag and are counted, then the rows of episode p become committed.  Returns (flags [S] uint8, tags [S]
    int64, evicted)."""
    S, E = int(slots), int(archive_episodes)
    flags, tags = np.zeros(S, dtype=np.uint8), np.full(S, -1, dtype=np.int64)
    evicted = 0
    for t, (p, recorded, ended) in enumerate(trace):
        s = t % S
        flags[s] = PENDING if recorded else 0
        tags[s] = int(p)
        if ended:
            old = (flags != 0) & (tags == int(p) - E)
            evicted += int(old.sum())
            flags[old] = 0
            flags[(flags == PENDING) & (tags == int(p))] = COMMITTED
    return flags, tags, evicted


# ---------------------------------------------------------------------------------------------------- replay buffer
class ReplayBuffer:
    """The samples of a SelfPlay batch in device memory: S x B rows of planes [C, N, N] fp32 (channels > 0), sparse policy (fp32 on the
    kmax slots of the root's valid set), valid set (int32, -1 padded), value target, reward (fp64) and a flag (1 pending, 2 committed).
    sample() draws from the committed rows only.
    compact=(H, E): no planes tensor (self.planes is None).  A row keeps its H history entries (ipp_plane_entry, 72 bytes each), the
    env's mean at record time [N] fp32 and its episode tag; the columns of an ended episode live once in a spare engine slot (E per
    env), and sample() builds the planes of the drawn rows with one ipp_feature_planes call (ipp_replay_compact_planes).  `evicted`
    counts the rows that lost their flag because their episode's archive slot was reused (never with E >= S)."""

    def __init__(self, owner: "SelfPlay", slots: int, num_envs: int, kmax: int, num_actions: int, channels: int, side: int, seed: int,
                 device, compact=None):
        import torch

        self.torch = torch
        self.slots, self.num_envs, self.kmax, self.num_actions = int(slots), int(num_envs), int(kmax), int(num_actions)
        self.channels, self.side, self.seed = int(channels), int(side), int(seed)
        cap = self.capacity = self.slots * self.num_envs
        e = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        self.planes = None
        self.compact = None
        if compact is not None:
            from ...feature_planes import empty_entries

            H, E = int(compact[0]), int(compact[1])
            self.history, self.archive_episodes = H, E
            self.entries = empty_entries(cap, H, device)                      # [cap, H, 18] int32 = ipp_plane_entry records
            self.mean = e((cap, self.side), torch.float32)
            self.episode_tag = torch.full((cap,), -1, dtype=torch.int64, device=device)
            self.episodes = e((self.num_envs,), torch.int64)                  # episodes of env e archived so far = its running episode's tag
            self.last_rank = e((self.num_envs,), torch.int32)
            self._evicted = e((1,), torch.int64)
            self.compact = _ffi.IppReplayCompact(history=H, archive_episodes=E, r_entries=self.entries.data_ptr(), r_mean=self.mean.data_ptr(),
                                                 r_episode=self.episode_tag.data_ptr(), episodes=self.episodes.data_ptr(),
                                                 last_rank=self.last_rank.data_ptr(), evicted=self._evicted.data_ptr())
        elif self.channels:
            need = cap * self.channels * self.side * self.side * 4
            total = torch.cuda.get_device_properties(device).total_memory
            if need > total // 2:
                raise ValueError(f"ring planes need {need / 2**30:.1f} GiB ({cap} rows of {self.channels} x {self.side}^2 floats): "
                                 f"lower the capacity or pass planes=False")
            self.planes = torch.empty((cap, self.channels, self.side, self.side), dtype=torch.float32, device=device)
        self.policy = e((cap, self.kmax), torch.float32)
        self.idx = torch.full((cap, self.kmax), -1, dtype=torch.int32, device=device)
        self.value = e((cap,), torch.float64)
        self.reward = e((cap,), torch.float64)
        self.flags = e((cap,), torch.uint8)
        self.iter = torch.full((cap,), -1, dtype=torch.int32, device=device)  # self-play iteration a committed row came from (-1: none)
        self._owner = owner
        self.draws = 0
        self.last_offsets = None
        self.timing = None  # list of (start, end) events around each gather launch while profiling

    def __len__(self) -> int:
        """Committed rows (reads the device)."""
        return int((self.flags == COMMITTED).sum().item())

    def nbytes(self) -> int:
        """Device bytes of the ring, in every mode: the rows' arrays (planes or entries + mean + tag; policy, valid set, value, reward,
        flag, iteration) and, in compact mode, the per-env archive bookkeeping.  The archived columns live in the engine's spare slots."""
        ts = [self.planes, self.policy, self.idx, self.value, self.reward, self.flags, self.iter]
        if self.compact is not None:
            ts += [self.entries, self.mean, self.episode_tag, self.episodes, self.last_rank, self._evicted]
        return int(sum(t.numel() * t.element_size() for t in ts if t is not None))

    @property
    def evicted(self) -> int:
        """Rows that lost their flag because the archive slot of their episode was reused (compact mode; reads the device)."""
        return int(self._evicted.item()) if self.compact is not None else 0

    # ------------------------------------------------------------------ persistence
    _ROW_ARRAYS = ("policy", "idx", "value", "reward", "flags", "iter")
    _COMPACT_ARRAYS = ("entries", "mean", "episode_tag", "episodes", "last_rank")

    def geometry(self) -> Dict:
        """What two rings have to share to exchange a state_dict."""
        c = self.compact is not None
        return dict(slots=self.slots, num_envs=self.num_envs, kmax=self.kmax, num_actions=self.num_actions, side=self.side,
                    history=self.history if c else 0, E=self.archive_episodes if c else 0, compact=bool(c))

    def state_dict(self) -> Dict:
        """Everything of a compact or planes=False ring a later process needs to go on sampling it: the row arrays (compact: entries,
        mean, episode tag; policy, idx, value, reward, flags, iter), the archive bookkeeping (episodes, last_rank, evicted), the draw
        count, the loop's step counter (the ring position), the geometry and, for a compact ring, the columns of exactly the archive
        slots that hold an episode (IPPEngine.export_slots, columns only; archive_slots_in_use from one read of `episodes`).  Tensors
        stay on the device.  The running episodes are not part of it: load_state_dict drops their pending rows.  A dense-planes ring
        raises ValueError."""
        if self.planes is not None:
            raise ValueError(f"a dense-planes ring is not persisted: its planes alone are {self.planes.numel() * 4 / 2**30:.2f} GiB "
                             f"({self.capacity} rows of {self.channels} x {self.side}^2 floats); use planes='compact'")
        sd = dict(geometry=self.geometry(), draws=int(self.draws), step=int(self._owner.t))
        for name in self._ROW_ARRAYS:
            sd[name] = getattr(self, name).clone()
        if self.compact is not None:
            for name in self._COMPACT_ARRAYS:
                sd[name] = getattr(self, name).clone()
            sd["evicted"] = self._evicted.clone()
            used = archive_slots_in_use(self.episodes.cpu().numpy(), self.num_envs, self.archive_episodes)
            sd["archive_slots"] = self.torch.as_tensor(used, dtype=self.torch.int64)
            sd["archive"] = self._owner.env.engine.export_slots(used, columns=True, maps=False)
        return sd

    def load_state_dict(self, sd: Dict):
        """state_dict of a ring of the same geometry (ValueError names a mismatch), from any device or the host: the arrays, the archive
        slots into the owner's engine (IPPEngine.import_slots: ValueError for another slot layout), the draw count and the step counter.
        Every PENDING row becomes 0: the running episodes are not part of a checkpoint."""
        torch = self.torch
        if self.planes is not None:
            raise ValueError("a dense-planes ring is not persisted; use planes='compact'")
        mine, theirs = self.geometry(), dict(sd["geometry"])
        for k, v in mine.items():
            if k not in theirs or theirs[k] != v:
                raise ValueError(f"replay state of another ring: {k} = {theirs.get(k)!r}, this ring has {v!r}")
        names = self._ROW_ARRAYS + (self._COMPACT_ARRAYS if self.compact is not None else ())
        for name in names:
            dst, src = getattr(self, name), sd[name]
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"replay state: {name} is {tuple(src.shape)} {src.dtype}, this ring has {tuple(dst.shape)} {dst.dtype}")
        if self.compact is not None:
            used = archive_slots_in_use(sd["episodes"].cpu().numpy(), self.num_envs, self.archive_episodes)
            if not np.array_equal(used, sd["archive_slots"].cpu().numpy()):
                raise ValueError("replay state: the exported archive slots are not those its episode counters name")
            self._owner.env.engine.import_slots(used, sd["archive"], check=True)
            self._evicted.copy_(sd["evicted"].to(self._evicted.device))
        for name in names:
            getattr(self, name).copy_(sd[name].to(self.flags.device))
        self.flags[self.flags == PENDING] = 0
        self.draws = int(sd["draws"])
        self._owner.t = int(sd["step"])

    def _compact_planes(self, n: int, copies: int, index, offsets, states):
        """states [n copies, C, N, N] of a minibatch drawn with channels = 0 (ipp_replay_compact_planes)."""
        torch, own = self.torch, self._owner
        dev = self.flags.device
        ent = torch.empty((n, self.history, self.entries.shape[2]), dtype=torch.int32, device=dev)
        mean = torch.empty((n, self.side), dtype=torch.float32, device=dev)
        cs = own.spec.to_c()
        _ffi.check(own._lib.ipp_replay_compact_planes(own.env.engine._h, C.byref(own._sp), C.byref(self.compact), C.byref(cs), n, copies,
                                                      index.data_ptr(), offsets.data_ptr() if offsets is not None else None,
                                                      ent.data_ptr(), mean.data_ptr(), states.data_ptr(), own.env.engine.stream))

    def gather_rows(self, rows):
        """(states, policies, values, rewards, valid_actions_msk) of the given ring rows, unshifted (ipp_replay_gather_rows; a row outside
        the ring: NaN).  In compact mode only committed rows have planes: a running episode has no archive yet."""
        torch, own = self.torch, self._owner
        dev = self.flags.device
        index = torch.as_tensor(rows, device=dev).to(torch.int64).reshape(-1).contiguous()
        n = int(index.numel())
        states = torch.empty((n, self.channels, self.side, self.side), dtype=torch.float32, device=dev) if self.channels else None
        pol = torch.empty((n, self.num_actions), dtype=torch.float32, device=dev)
        msk = torch.empty((n, self.num_actions), dtype=torch.uint8, device=dev)
        val = torch.empty((n,), dtype=torch.float64, device=dev)
        rew = torch.empty((n,), dtype=torch.float64, device=dev)
        gc = self.channels if self.planes is not None else 0
        _ffi.check(own._lib.ipp_replay_gather_rows(C.byref(own._sp), n, gc, self.side, self.planes.data_ptr() if gc else None,
                                                   index.data_ptr(), states.data_ptr() if gc else None, pol.data_ptr(), msk.data_ptr(),
                                                   val.data_ptr(), rew.data_ptr(), own.env.engine.stream))
        if self.compact is not None:
            self._compact_planes(n, 1, index, None, states)
        return states, pol, val, rew, msk

    def committed_rows(self):
        """Device int64 indices of the committed rows, ascending."""
        return self.torch.nonzero(self.flags == COMMITTED).reshape(-1)

    def window(self, lo: int, hi: int) -> "ReplayWindow":
        """The rows of self-play iterations lo .. hi (ReplayBuffer(self_play_iteration, window_size), replay_buffers.py:34-46): a view
        with the members a Trainer uses (len, sample, prioritized).  A ring that never saw an iteration has an empty window."""
        return ReplayWindow(self, lo, hi)

    def prioritized(self, batch_size: int = 32, alpha: float = 0.75, beta0: float = 0.5, num_epochs: int = 3) -> "PrioritizedReplay":
        """PrioritizedExperienceReplayBuffer (replay_buffers.py:104-141) over the rows committed now; reads their count from the device
        once, as the reference reads len(self.data_file_paths)."""
        return PrioritizedReplay(self, batch_size, alpha, beta0, num_epochs)

    def sample(self, batch_size: int, num_augmented_samples: int = 0, check_empty: bool = True):
        """(states [b (k+1), C, N, N] f32, policies [b (k+1), A] f32, values f64, rewards f64, valid_actions_msk [b (k+1), A] u8,
        indices i64 (ring rows), weights (ones, f64)) -- ExperienceReplayBuffer.sample with augment_random_crop: b = max(1, batch_size //
        (k + 1)) rows drawn uniformly with replacement from the committed rows, originals first, then k shifted copies.  states is None
        without planes.  check_empty reads the committed count from the device and raises on an empty buffer (else the rows are -1 / NaN)."""
        return self._sample(self.flags == COMMITTED, batch_size, num_augmented_samples, check_empty,
                            "the replay buffer holds no committed sample yet (no episode has ended)")

    def _sample(self, sampleable, batch_size: int, num_augmented_samples: int, check_empty: bool, empty: str):
        """sample() over the rows of the device mask `sampleable`."""
        torch = self.torch
        k = int(num_augmented_samples)
        if k < 0:
            raise ValueError("num_augmented_samples must be >= 0")
        n = max(1, int(batch_size) // (k + 1))
        copies = k + 1
        cum = torch.cumsum(sampleable.to(torch.int32), 0, dtype=torch.int32)
        if check_empty and int(cum[-1].item()) == 0:
            raise ValueError(empty)
        dev, rows = self.flags.device, n * copies
        states = torch.empty((rows, self.channels, self.side, self.side), dtype=torch.float32, device=dev) if self.channels else None
        pol = torch.empty((rows, self.num_actions), dtype=torch.float32, device=dev)
        msk = torch.empty((rows, self.num_actions), dtype=torch.uint8, device=dev)
        val = torch.empty((rows,), dtype=torch.float64, device=dev)
        rew = torch.empty((rows,), dtype=torch.float64, device=dev)
        index = torch.empty((rows,), dtype=torch.int64, device=dev)
        offs = torch.empty((copies, 2), dtype=torch.int32, device=dev)
        own = self._owner
        if self.timing is not None:  # (events around the gather kernel alone: tools/selfplay_bench.py)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        gc = self.channels if self.planes is not None else 0  # (compact: the row draw alone, then the planes of the drawn rows)
        _ffi.check(own._lib.ipp_replay_gather(C.byref(own._sp), n, copies, gc, self.side,
                                              self.planes.data_ptr() if gc else None, cum.data_ptr(), C.c_uint64(self.seed),
                                              C.c_uint64(REPLAY_STREAM + self.draws), states.data_ptr() if gc else None,
                                              pol.data_ptr(), msk.data_ptr(), val.data_ptr(), rew.data_ptr(), index.data_ptr(), offs.data_ptr(),
                                              own.env.engine.stream))
        if self.compact is not None:
            self._compact_planes(n, copies, index, offs, states)
        if self.timing is not None:
            ev[1].record()
            self.timing.append(ev)
        self.draws += 1
        self.last_offsets = offs
        return states, pol, val, rew, msk, index, torch.ones((rows,), dtype=torch.float64, device=dev)


class ReplayWindow:
    """The off-policy window of a ring: its rows that are committed and tagged with a self-play iteration in [lo, hi].  What a Trainer
    uses of a ReplayBuffer, on those rows only; the minibatch draws share the ring's draw count."""

    def __init__(self, ring: ReplayBuffer, lo: int, hi: int):
        self.ring, self.lo, self.hi = ring, int(lo), int(hi)
        if self.lo > self.hi:
            raise ValueError(f"window [{lo}, {hi}]: lo > hi")

    def mask(self):
        r = self.ring
        return (r.flags == COMMITTED) & (r.iter >= self.lo) & (r.iter <= self.hi)

    def __len__(self) -> int:
        """Rows in the window (one read of the device)."""
        return int(self.mask().sum().item())

    def rows(self):
        """Device int64 indices of the window's rows, ascending."""
        return self.ring.torch.nonzero(self.mask()).reshape(-1)

    def sample(self, batch_size: int, num_augmented_samples: int = 0, check_empty: bool = True):
        """ReplayBuffer.sample drawn from the window's rows."""
        return self.ring._sample(self.mask(), batch_size, num_augmented_samples, check_empty,
                                 f"no committed sample of self-play iterations {self.lo} .. {self.hi} is in the ring")

    def prioritized(self, batch_size: int = 32, alpha: float = 0.75, beta0: float = 0.5, num_epochs: int = 3) -> "PrioritizedReplay":
        """ReplayBuffer.prioritized over the window's rows (ipp_replay_priority_reset_window): every other row has no mass."""
        return PrioritizedReplay(self.ring, batch_size, alpha, beta0, num_epochs, window=(self.lo, self.hi))


class PrioritizedReplay:
    """PrioritizedExperienceReplayBuffer (replay_buffers.py:104-141) on the ring of a ReplayBuffer: rows drawn in proportion to
    priority ** alpha, importance-sampling weights (P L) ** -beta over their maximum, priorities written back by update(), beta raised by
    step().  Construction fixes the sampled set: the L rows committed then start at priority 1 / L, every other row at 0, so rows
    committed later are not drawn (the reference's file list is fixed too) and a row that a later record re-opens drops out.  The
    minibatch draws share the ring's draw count with ReplayBuffer.sample.  After construction nothing here reads the device from the host."""

    def __init__(self, ring: ReplayBuffer, batch_size: int = 32, alpha: float = 0.75, beta0: float = 0.5, num_epochs: int = 3,
                 window=None):
        """window: (lo, hi) restricts the sampled set to the committed rows of those self-play iterations (ReplayBuffer.window)."""
        torch = self.torch = ring.torch
        self.ring = ring
        self.alpha, self.beta0, self.beta = float(alpha), float(beta0), float(beta0)
        if not (0.0 <= self.alpha < float("inf")) or not (0.0 <= self.beta0 <= 1.0):
            raise ValueError(f"alpha = {alpha} outside [0, inf) or beta0 = {beta0} outside [0, 1]")
        self.sample_size = max(1, int(batch_size))  # (no augmented copies under PER, :114)
        dev, cap = ring.flags.device, ring.capacity
        own = ring._owner
        self.priorities = torch.empty((cap,), dtype=torch.float64, device=dev)
        self._cum = torch.empty((cap,), dtype=torch.float64, device=dev)
        self._scratch = torch.empty(((cap + _ffi.IPP_REPLAY_SCAN_TILE - 1) // _ffi.IPP_REPLAY_SCAN_TILE,), dtype=torch.float64, device=dev)
        count = torch.zeros((1,), dtype=torch.int64, device=dev)
        if window is None:
            _ffi.check(own._lib.ipp_replay_priority_reset(C.byref(own._sp), self.priorities.data_ptr(), count.data_ptr(), own.env.engine.stream))
        else:
            _ffi.check(own._lib.ipp_replay_priority_reset_window(C.byref(own._sp), ring.iter.data_ptr(), int(window[0]), int(window[1]),
                                                                self.priorities.data_ptr(), count.data_ptr(), own.env.engine.stream))
        self.committed = int(count.item())  # (the one read: len(self.data_file_paths))
        if self.committed == 0:
            raise ValueError("the replay buffer holds no committed sample yet (no episode has ended)")
        self.total_steps = (self.committed // self.sample_size) * int(num_epochs)
        if self.total_steps <= 0:
            raise ValueError(f"total_steps = ({self.committed} committed rows // {self.sample_size}) x {num_epochs} epochs = 0: "
                             f"the beta schedule has no step")
        self.timing = None  # list of (start, drawn, end) events around the mass + draw and the gather launches while profiling

    def __len__(self) -> int:
        """Rows committed at construction (L; no device read)."""
        return self.committed

    def sample(self):
        """(states [n, C, N, N] f32 or None, policies [n, A] f32, values f64, rewards f64, valid_actions_msk [n, A] u8, indices i64
        (ring rows), weights f32), n = max(1, batch_size).  With no mass left (every sampled row re-opened): indices -1, NaN."""
        torch, r = self.torch, self.ring
        own, n = r._owner, self.sample_size
        dev, sp, st = r.flags.device, C.byref(r._owner._sp), r._owner.env.engine.stream
        states = torch.empty((n, r.channels, r.side, r.side), dtype=torch.float32, device=dev) if r.channels else None
        pol = torch.empty((n, r.num_actions), dtype=torch.float32, device=dev)
        msk = torch.empty((n, r.num_actions), dtype=torch.uint8, device=dev)
        val = torch.empty((n,), dtype=torch.float64, device=dev)
        rew = torch.empty((n,), dtype=torch.float64, device=dev)
        index = torch.empty((n,), dtype=torch.int64, device=dev)
        weights = torch.empty((n,), dtype=torch.float32, device=dev)
        if self.timing is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        _ffi.check(own._lib.ipp_replay_mass(sp, self.priorities.data_ptr(), self.alpha, self._cum.data_ptr(), self._scratch.data_ptr(),
                                            C.c_uint64(self._scratch.numel()), st))
        _ffi.check(own._lib.ipp_replay_draw_per(sp, self.priorities.data_ptr(), self._cum.data_ptr(), self.alpha, self.beta, self.committed, n,
                                                C.c_uint64(r.seed), C.c_uint64(REPLAY_STREAM + r.draws), index.data_ptr(),
                                                weights.data_ptr(), st))
        if self.timing is not None:
            ev[1].record()
        gc = r.channels if r.planes is not None else 0
        _ffi.check(own._lib.ipp_replay_gather_rows(sp, n, gc, r.side, r.planes.data_ptr() if gc else None, index.data_ptr(),
                                                   states.data_ptr() if gc else None, pol.data_ptr(), msk.data_ptr(),
                                                   val.data_ptr(), rew.data_ptr(), st))
        if r.compact is not None:
            r._compact_planes(n, 1, index, None, states)
        if self.timing is not None:
            ev[2].record()
            self.timing.append(ev)
        r.draws += 1
        return states, pol, val, rew, msk, index, weights

    def step(self):
        """beta towards 1 by (1 - beta0) / total_steps (:122-123)."""
        self.beta = per_beta_step(self.beta, self.beta0, self.total_steps)

    def update(self, indices, priorities):
        """priorities[indices] = priorities (:140-141; the caller adds the reference's 1e-8): device tensors stay on the device; the
        last occurrence of a repeated index wins, -1 is skipped."""
        torch, r = self.torch, self.ring
        dev = r.flags.device
        idx = torch.as_tensor(indices, device=dev).to(torch.int64).reshape(-1).contiguous()
        val = torch.as_tensor(priorities, device=dev).to(torch.float64).reshape(-1).contiguous()
        if idx.numel() != val.numel():
            raise ValueError(f"{idx.numel()} indices, {val.numel()} priorities")
        own = r._owner
        _ffi.check(own._lib.ipp_replay_priority_update(C.byref(own._sp), self.priorities.data_ptr(), idx.data_ptr(), val.data_ptr(),
                                                       int(idx.numel()), own.env.engine.stream))


# ---------------------------------------------------------------------------------------------------- the loop
class SelfPlay:
    def __init__(self, cfg, num_envs: int, hyper_params: Dict, meta_data: Dict, infer: Optional[Callable] = None,
                 capacity: Optional[int] = None, seed: int = 0, env_id_offset: int = 0, random_init_action: bool = True,
                 planes=True, sims_in_flight: int = 4, tie_break: str = "first", groups: int = 2, device: str = "cuda:0",
                 archive_episodes: Optional[int] = None, episode_priors: Optional[str] = None, **env_kwargs):
        """cfg: EngineConfig; hyper_params / meta_data: the reference's dictionaries (config/example.yaml: gamma, puct_*, dirichlet_*,
        num_mcts_simulations, temperature_scale / _threshold, input_history_length, use_fov_input, use_action_costs_input, shuffle_budget;
        initial_budget, max_episode_steps, episode_horizon, min / max_altitude, altitude_spacing, uav_specifications, scenario_info).
        infer: DeviceMCTS's network callback (None: uniform priors, value 0); with a network the leaves' planes come along.
        capacity: ring rows (a multiple of num_envs, at least (max_episode_steps + 1) num_envs; default the minimum).
        planes=False keeps no planes in the ring (large grids: a 50x50 plane is 25 MB per channel).  planes="compact" keeps, per row,
        the history entries, the mean and the episode tag (a few KB) and, per ended episode, one copy of its factor columns in a spare
        engine slot; the planes are built when a minibatch is drawn (ReplayBuffer).  archive_episodes = E: archive slots per env
        (spare_slots = num_envs E go to the env); None: the ring's step slots S, with which nothing is evicted; a smaller E evicts
        the rows of episode p - E when episode p ends: E >= S / (steps of the shortest episode expected) avoids it.
        episode_priors: None -- a true hyper_params["shuffle_prior_cov"] raises; "device" -- hyper_params["shuffle_prior_cov"] decides:
        True gives every episode its own prior (sigma^2, l) ~ U(0.8, 1.2) x nominal (mapping/mappings.py:238-240), drawn on the device
        by the reset that starts it (VecIPPEnv(shuffle_prior_cov="device"), vec_env.start_prior); False is the config's prior, bit for
        bit the run without the argument.
        env_kwargs go to VecIPPEnv."""
        S, steps = check_args(hyper_params, meta_data, num_envs, capacity, episode_priors)
        if episode_priors == "device" and hyper_params.get("shuffle_prior_cov", False):
            env_kwargs["shuffle_prior_cov"] = "device"
        E = check_replay_mode(planes, archive_episodes, S)
        if E:
            from ...engine import patch_layout_possible

            if not patch_layout_possible(cfg, env_kwargs.get("state", "factor"), env_kwargs.get("window_rows", -1), True,
                                         env_kwargs.get("rank_cap", 9 * (steps + int(meta_data["episode_horizon"]) + 2)),
                                         env_kwargs.get("tile_threads", 0)):
                raise ValueError("planes='compact' archives episodes as patch-layout factor slots (ipp_info.patch_layout == 1): this grid, "
                                 "window or rank_cap cannot have it")
            env_kwargs["spare_slots"] = int(num_envs) * E
        import torch

        from ...feature_planes import PlaneSpec
        from .device_mcts import DeviceMCTS

        self.torch = torch
        hp, md = dict(hyper_params), dict(meta_data)
        md.setdefault("budget", md["initial_budget"])
        self.hp, self.md = hp, md
        B = self.num_envs = int(num_envs)
        self.slots, self.max_episode_steps = S, steps
        self.seed, self.random_init = int(seed), bool(random_init_action)
        horizon = int(md["episode_horizon"])
        sims, W = int(hp["num_mcts_simulations"]), int(sims_in_flight)
        H = int(hp["input_history_length"])
        env_kwargs.setdefault("window_rows", -1)
        env_kwargs.setdefault("adaptive", md.get("scenario_info") is not None)
        env_kwargs.setdefault("use_flight_time", md.get("uav_specifications") is not None)
        env_kwargs.setdefault("node_capacity", B * (sims + 16))
        env_kwargs.setdefault("max_batch", B * W)
        env_kwargs.setdefault("rank_cap", 9 * (steps + horizon + 2))  # (a search adds up to horizon + 1 steps of columns to a root)
        self.env = VecIPPEnv(cfg, B, episode_steps=steps, device=device, seed=seed, env_id_offset=env_id_offset,
                             budget=float(md["initial_budget"]), shuffle_budget=bool(hp.get("shuffle_budget", False)), feature_history=H,
                             **env_kwargs)
        env = self.env
        self.device = env.device
        self.spec = PlaneSpec.from_params(hp, md, adaptive=env.adaptive, use_flight_time=env.use_flight_time)
        # (the search divides the engine's tree nodes among its SLOTS by default; with spare slots the roots are the envs alone)
        dev_per_root = max(1, min(2 * sims + 2 * W + 8, int(env.engine._c.node_capacity) // B)) if env.spare_slots else None
        self.mcts = DeviceMCTS(env.engine, hp, md, infer, sims_in_flight=W, tie_break=tie_break, seed=seed, groups=groups,
                               feature_planes=infer is not None, dev_per_root=dev_per_root)
        self.mcts._key_base = env.env_id_offset  # (the search's counter-based draws keyed on the global env id too)
        self.infer = infer
        geo = self.mcts._geometry(torch, self.device)
        self.kmax, self.num_actions = int(geo["kmax"]), int(self.mcts.num_actions)
        if self.kmax > MAX_KMAX:
            env.engine.close()
            raise ValueError(f"valid-action sets of up to {self.kmax} actions (max_valid_action_distance {hp['max_valid_action_distance']}): "
                             f"the ring rows hold at most {MAX_KMAX}")
        self.actions = geo["actions"]
        # temperatures: temperature_scale * (depth < temperature_threshold) (:118-120); a temperature-0 step takes the arg-max of the
        # read-out at temperature 1 (visits / sum: same order, same ties)
        scale, thr = float(hp["temperature_scale"]), int(hp["temperature_threshold"])
        self.temp_zero = not scale > 0
        need_pos, need_zero = (not self.temp_zero) and thr > 0, self.temp_zero or thr < steps
        self._temps = ([scale] if need_pos else []) + ([1.0] if need_zero and not (need_pos and scale == 1.0) else [])
        self._t_index = (0, len(self._temps) - 1)  # (policy_t, policy_1) among the read-outs
        self.replay = ReplayBuffer(self, S, B, self.kmax, self.num_actions, self.spec.channels if planes else 0, cfg.n_cells,
                                   seed, self.device, compact=(H, E) if E else None)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        self.ep_len, self.forced = z((B,), torch.int32), z((B,), torch.uint8)
        self.tie_u = z((B,), torch.float64)
        self.episode_values = torch.full((B,), float("nan"), dtype=torch.float64, device=self.device)
        self.action, self.action_idx = z((B, 3), torch.float64), z((B,), torch.int32)
        self._roots = torch.arange(B, dtype=torch.int32, device=self.device)
        self._lib = env.engine._lib
        r = self.replay
        sp = self._sp = _ffi.IppSelfPlay(
            num_envs=B, slots=S, kmax=self.kmax, num_actions=self.num_actions, horizon=horizon, temp_threshold=thr,
            temp_zero=int(self.temp_zero), random_init=int(self.random_init), device=self.device.index or 0, reserved=0,
            gamma=float(hp["gamma"]), seed=self.seed & (2 ** 64 - 1), row_offset=env.env_id_offset)
        ptrs = dict(actions=self.actions, budget=env.budget, depth=env.depth, episode=env.episode, done=env.done, prev=env.prev,
                    reward=env.reward, ep_len=self.ep_len, forced=self.forced, tie_u=self.tie_u, episode_value=self.episode_values,
                    action=self.action, action_idx=self.action_idx, r_policy=r.policy, r_idx=r.idx, r_value=r.value,
                    r_reward=r.reward, r_flags=r.flags)
        for name, t in ptrs.items():
            setattr(sp, name, t.data_ptr())
        self.t = 0
        self.last = None
        self._it = None  # the ipp_selfplay_iter of begin_iteration (the learn loop's iterations)
        self.timing = None  # dict phase -> list of (start, end) event pairs while profiling (tools/selfplay_bench.py)
        self.reset()

    # ------------------------------------------------------------------
    def reset(self):
        """Every env starts episode 0 (the env's reset), at its drawn first waypoint; the ring keeps its committed rows."""
        torch, env, B = self.torch, self.env, self.num_envs
        env.reset()
        gid = np.arange(B, dtype=np.int64) + env.env_id_offset
        epi = env.episode.cpu().numpy()
        if self.random_init:
            a0 = init_action_index(self.seed, gid, epi, self.num_actions)
            env.prev.copy_(self.actions[torch.as_tensor(a0, device=self.device)])
        self.tie_u.copy_(torch.as_tensor(step_uniform(TIE_STREAM, self.seed, gid, epi, env.depth.cpu().numpy()), device=self.device))
        self.ep_len.zero_()
        self.forced.zero_()
        self.replay.flags[self.replay.flags == PENDING] = 0  # (rows of episodes that will never end)

    def _mark(self, name):
        if self.timing is not None:
            ev = self.torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timing.setdefault(name, []).append(ev)

    def step(self, _iteration: bool = False):
        """One search per env, record, sample the actions, env.step, commit the episodes that ended.  episode_values: the
        total_episode_value of every env whose episode ended in this step (NaN elsewhere).  (_iteration: step_iteration's commit.)"""
        env, r, B = self.env, self.replay, self.num_envs
        t = self.t
        slot = t % self.slots
        self._mark("planes")
        ent = env.history_entries() if (r.channels or self.infer is not None) else None
        if r.compact is not None:  # (what the planes are a function of, not the planes)
            _ffi.check(self._lib.ipp_replay_record_compact(env.engine._h, C.byref(self._sp), C.byref(r.compact), int(t), ent.data_ptr(),
                                                           env.engine.stream))
        elif r.channels:  # (= env.feature_planes(spec, out=...): the same entries feed the search's leaf planes)
            env.engine.feature_planes(ent, self.spec, mask_env=ent[:, 0, 0], out=r.planes[slot * B:(slot + 1) * B])
        self._mark("search")
        out = self.mcts.search_device(self._roots, env.prev, env.budget, self._temps, self.tie_u, depth=0,
                                      root_history=ent if self.infer is not None else None)
        pol_t, pol_1 = out["policy"][self._t_index[0]], out["policy"][self._t_index[1]]
        self.last = dict(policy_t=pol_t, policy_1=pol_1, valid_idx=out["valid_idx"], ok=out["ok"])
        self._mark("record")
        _ffi.check(self._lib.ipp_selfplay_record(C.byref(self._sp), int(t), pol_t.data_ptr(), pol_1.data_ptr(), out["valid_idx"].data_ptr(),
                                                 out["ok"].data_ptr(), env.engine.stream))
        self._mark("step")
        env.step(self.action)
        if r.compact is not None:  # (the ended episodes' columns into their archive slots: behind the step's resets, before the commit)
            self._mark("archive")
            _ffi.check(self._lib.ipp_selfplay_archive(env.engine._h, C.byref(self._sp), C.byref(r.compact), env.engine.stream))
        self._mark("commit")
        if _iteration:
            _ffi.check(self._lib.ipp_selfplay_commit_iter(C.byref(self._sp), int(t), C.byref(self._it), env.engine.stream))
            _ffi.check(self._lib.ipp_selfplay_iter_totals(C.byref(self._sp), C.byref(self._it), self._it_totals.data_ptr(), env.engine.stream))
            self._it_totals_host.copy_(self._it_totals, non_blocking=True)
            self._it_totals_ev.record()
        else:
            _ffi.check(self._lib.ipp_selfplay_commit(C.byref(self._sp), int(t), env.engine.stream))
        self._mark("end")
        self.t += 1
        return self.episode_values

    def run(self, steps: int):
        for _ in range(int(steps)):
            self.step()
        return self

    # ------------------------------------------------------------------ iterations of the learn loop
    def begin_iteration(self, iteration: int, episodes_per_env: int):
        """Start self-play iteration `iteration` (mcts_zero_mission.py:305-340): every env is to end `episodes_per_env` episodes whose
        rows are tagged with the iteration; the counters start at zero and every env starts a new episode (reset(): running episodes are
        abandoned, as the reference starts fresh generators per iteration).  The iteration arrays are allocated once."""
        torch = self.torch
        iteration, cap = int(iteration), int(episodes_per_env)
        if iteration < 0 or cap < 1:
            raise ValueError(f"iteration = {iteration}, episodes_per_env = {cap}: need iteration >= 0 and at least 1 episode per env")
        if self._it is None:
            B, dev = self.num_envs, self.device
            self.iter_episodes = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.iter_examples = torch.zeros((B,), dtype=torch.int64, device=dev)
            self.iter_value_sum = torch.zeros((B,), dtype=torch.float64, device=dev)
            self._it_totals = torch.zeros((4,), dtype=torch.int64, device=dev)  # (the 32-byte record: three int64 and a double)
            self._it_totals_host = torch.zeros((4,), dtype=torch.int64).pin_memory()
            self._it_totals_ev = torch.cuda.Event()
            self._it = _ffi.IppSelfPlayIter(iter_episodes=self.iter_episodes.data_ptr(), r_iter=self.replay.iter.data_ptr(),
                                            examples=self.iter_examples.data_ptr(), value_sum=self.iter_value_sum.data_ptr())
        self._it.iteration, self._it.episode_cap = iteration, cap
        for t in (self.iter_episodes, self.iter_examples, self.iter_value_sum):
            t.zero_()
        self.iteration_totals = dict(episodes_kept=0, envs_at_cap=0, examples=0, value_sum=0.0)
        self.reset()

    def step_iteration(self):
        """step() of the running iteration: the commit applies the iteration rule (ipp_selfplay_commit_iter) and the iteration's totals
        come to pinned memory, the step's one small read.  Returns them: dict(episodes_kept, envs_at_cap, examples, value_sum)."""
        if self._it is None:
            raise ValueError("no iteration: call begin_iteration(i, episodes_per_env) first")
        self.step(_iteration=True)
        self._it_totals_ev.synchronize()
        rec = self._it_totals_host.numpy()
        self.iteration_totals = dict(episodes_kept=int(rec[0]), envs_at_cap=int(rec[1]), examples=int(rec[2]),
                                     value_sum=float(rec[3:4].view(np.float64)[0]))
        return self.iteration_totals

    def run_iteration(self, iteration: int, episodes_per_env: int, max_steps: Optional[int] = None):
        """begin_iteration, then step_iteration until every env has ended episodes_per_env episodes.  Past max_steps (default
        episodes_per_env x (max_episode_steps + 1): an episode takes at most max_episode_steps steps and one more where it ends without
        a sample) it raises instead of looping.  Returns the totals record as a dict."""
        self.begin_iteration(iteration, episodes_per_env)
        limit = int(episodes_per_env) * (self.max_episode_steps + 1) if max_steps is None else int(max_steps)
        steps = 0
        while self.iteration_totals["envs_at_cap"] < self.num_envs:
            if steps >= limit:
                raise RuntimeError(f"self-play iteration {int(iteration)}: {self.iteration_totals['envs_at_cap']} of {self.num_envs} envs "
                                   f"have ended {int(episodes_per_env)} episodes after {steps} steps (max_steps = {limit})")
            self.step_iteration()
            steps += 1
        return dict(self.iteration_totals, steps=steps)

    # ------------------------------------------------------------------ persistence of the ring
    def state_dict(self) -> Dict:
        """ReplayBuffer.state_dict of the loop's ring (compact or planes=False; tensors on the device)."""
        return self.replay.state_dict()

    def load_state_dict(self, sd: Dict):
        """ReplayBuffer.load_state_dict into the loop's ring.  A loop that has already stepped abandons its running episodes first
        (reset()), as an iteration does; their pending rows, like the checkpoint's, are dropped."""
        if self.t:
            self.reset()
        self.replay.load_state_dict(sd)

    def close(self):
        self.env.engine.close()
