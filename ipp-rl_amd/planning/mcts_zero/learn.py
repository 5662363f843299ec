"""
Learner: the reference's training loop -- MCTSZeroMission.learn and evaluate_trained_agent, planning/mcts_zero/mcts_zero_mission.py:254-455,
with its schedules (:231-252) -- over the stations that already run on the device:

    schedule      puct_init / dirichlet_alpha decay once per iteration > 0 (:231-243)                     DeviceMCTS.set_exploration
    self-play     every env ends `episodes_per_env` episodes, their rows tagged with the iteration (:320-340)   SelfPlay.run_iteration
    eviction      rows of iteration <= i - max_train_examples_history leave the ring (:364-368)
    temp          shared_net.temp.pth.tar: the weights in front of the training (:371-372)
    train         Trainer.train on the off-policy window of iterations max(0, i - w + 1) .. i (:374; ReplayBuffer(self_play_iteration,
                  window_size), replay_buffers.py:34-46, w = off_policy_window_size(i), :245-252)                  ReplayBuffer.window
    snapshot      shared_net.snapshot_{i}.pth.tar (:375)
    update        continuous_network_update: the deployment file, and the search plays with the new weights (:389-396); otherwise the
                  arena gate (:417-455): rejected -> the module goes back to the temp checkpoint, accepted -> deployment file + search

Two DevicePolicyValueNets: `search_net` serves the self-play search and is the arena's previous player; `trained_net` receives the
trained weights and is the arena's current player.  The search never sees weights that were not accepted.

Checkpoints are torch.save({"state_dict": module.state_dict()}) under the reference's file names (save_checkpoint,
network_wrappers/policy_value_network_wrappers.py:233-249) in `checkpoint_dir`; learn_state.pt beside them holds the last finished
iteration, the scheduled values, prev_network_wins, the rows each iteration reported and the draws' seeds and counters.

Divergences from the reference (INTEGRATION.md "Learn loop"): episodes per env, not per worker; an env's episodes past its share are
played out and dropped; an iteration abandons the running episodes; the ring is persisted only on request (persist_replay=True writes
replay_state.pt, and a resumed loop trains on the full off-policy window as the reference's does from its sample files; by default a
resumed loop starts with an empty window); the running episodes and their pending rows are abandoned at a resume either way;
shared_network=False, skip_first_self_play / train_examples_iter, TensorBoard and Telegram are not provided.
"""
from __future__ import annotations

import math
import os
import time
from typing import Callable, Dict, List, Optional, Tuple

TEMP_FILE = "shared_net.temp.pth.tar"
STATE_FILE = "learn_state.pt"
REPLAY_FILE = "replay_state.pt"


def snapshot_file(iteration: int) -> str:
    return f"shared_net.snapshot_{int(iteration)}.pth.tar"


def deployment_file(deployment_filename: str) -> str:
    return f"shared_net.{deployment_filename}"


# ---------------------------------------------------------------------------------------------------- the schedules
def exploration_schedule(hyper_params: Dict, iteration: int) -> Tuple[float, float]:
    """schedule_exploration_parmeters (:231-243) as a function: (puct_init, dirichlet_alpha) of `iteration` given the values of the
    iteration before in hyper_params -- for iteration > 0 each decays by its factor down to its minimum, iteration 0 keeps them.
    Apply it once per iteration (the reference writes the result back into hyper_params)."""
    puct, alpha = hyper_params["puct_init"], hyper_params["dirichlet_alpha"]
    if int(iteration) > 0:
        puct = max(hyper_params["puct_init_min"], puct * hyper_params["puct_init_decay"])
        alpha = max(hyper_params["dirichlet_alpha_min"], alpha * hyper_params["dirichlet_alpha_decay"])
    return puct, alpha


def off_policy_window_size(hyper_params: Dict, iteration: int) -> int:
    """schedule_off_policy_window_size (:245-252): how many iterations of samples the training of `iteration` draws from."""
    return min(int(hyper_params["start_train_examples_history"] + iteration / hyper_params["train_examples_history_step"]),
               hyper_params["max_train_examples_history"])


def check_args(hyper_params: Dict, num_envs: int, episodes_per_env: Optional[int], arena_envs: Optional[int]):
    """What the Learner cannot run, refused before anything touches the device.  Returns (episodes_per_env, arena_envs)."""
    if not hyper_params.get("shared_network", True):
        raise ValueError("shared_network=False (separate policy and value networks) is not supported: the device network, the trainer "
                         "and the arena serve the shared PolicyValueNetwork")
    B = int(num_envs)
    if B < 1:
        raise ValueError("num_envs must be >= 1")
    if episodes_per_env is None:
        episodes_per_env = math.ceil(int(hyper_params["num_episodes"]) * int(hyper_params.get("num_workers", 1)) / B)
    if int(episodes_per_env) < 1:
        raise ValueError(f"episodes_per_env = {episodes_per_env}: at least 1")
    if not hyper_params.get("continuous_network_update", False):
        games = int(hyper_params["num_arena_games"])
        if arena_envs is None:
            arena_envs = math.gcd(games, B)
        if int(arena_envs) < 1 or games % int(arena_envs):
            raise ValueError(f"num_arena_games = {games} is not a positive multiple of arena_envs = {arena_envs}")
    return int(episodes_per_env), (None if arena_envs is None else int(arena_envs))


# ---------------------------------------------------------------------------------------------------- the loop
class Learner:
    def __init__(self, cfg, num_envs: int, hyper_params: Dict, meta_data: Dict, module, checkpoint_dir: str,
                 episodes_per_env: Optional[int] = None, arena_envs: Optional[int] = None, seed: int = 0, env_id_offset: int = 0,
                 deployment_filename: str = "trained_model.pth.tar", precision: str = "fp32", net_max_batch: Optional[int] = None,
                 persist_replay: bool = False, **selfplay_kwargs):
        """cfg: EngineConfig; hyper_params / meta_data: the reference's dictionaries (config/example.yaml) for the search, the network
        and the trainer in one, as there; module: the PolicyValueNetwork to train, on the device.  episodes_per_env: episodes every env
        ends per iteration (default ceil(num_episodes x num_workers / num_envs): at least the reference's episodes per iteration).
        arena_envs: envs of the gate's arena (default gcd(num_arena_games, num_envs)).  net_max_batch: leaves one forward of a device
        network takes (default max(num_envs, arena_envs) x sims_in_flight).  persist_replay: every finished iteration also writes the ring
        (SelfPlay.state_dict: row arrays, archive bookkeeping and, for a compact ring, the archived episodes' columns, tensors on the
        host) to replay_state.pt, and learn(resume=True) loads it back, so the resumed iterations train on the whole off-policy window;
        planes="compact" rings only here (a dense-planes ring raises at the first save).  selfplay_kwargs go to SelfPlay (capacity: the ring has to
        hold the rows of a whole off-policy window, see INTEGRATION.md "Learn loop"; planes="compact" and archive_episodes: the compact
        ring, whose rows are a few KB, so that such a window fits beside thousands of envs; episode_priors="device": a true
        hyper_params["shuffle_prior_cov"] -- config/example.yaml's setting -- gives every self-play episode its own prior, drawn on the
        device, vec_env.start_prior; the arena stays on the config's prior, as the reference's does, and learn_state.pt needs nothing new:
        the priors are a function of seed, global env id and episode index); sims_in_flight, tie_break and groups go to the arena too."""
        self.episodes_per_env, self.arena_envs = check_args(hyper_params, num_envs, episodes_per_env, arena_envs)
        import torch

        from .networks import DevicePolicyValueNet
        from .selfplay import SelfPlay
        from .training import Trainer

        self.torch = torch
        self.cfg, self.num_envs = cfg, int(num_envs)
        hp = self.hp = dict(hyper_params)
        md = self.md = dict(meta_data)
        md.setdefault("num_grid_cells", cfg.n_cells)
        self.module = module
        self.checkpoint_dir, self.deployment_filename = str(checkpoint_dir), str(deployment_filename)
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)
        self.puct_init, self.dirichlet_alpha = float(hp["puct_init"]), float(hp["dirichlet_alpha"])
        self.prev_network_wins = 0
        self.persist_replay = bool(persist_replay)
        self.iteration = -1         # the last finished iteration
        self.reported: Dict[int, int] = {}  # iteration -> rows its self-play reported (for `evicted`)
        self.history: List[Dict] = []
        kw = dict(selfplay_kwargs)
        self._arena_kwargs = {k: kw[k] for k in ("sims_in_flight", "tie_break", "groups", "device", "grf_rows") if k in kw}
        W = int(kw.get("sims_in_flight", 4))
        device = kw.get("device", "cuda:0")
        if net_max_batch is None:
            net_max_batch = max(self.num_envs, self.arena_envs or 1) * W
        state = module.state_dict()
        self.search_net = DevicePolicyValueNet(hp, md, state, side=cfg.n_cells, precision=precision, max_batch=int(net_max_batch), device=device)
        self.trained_net = DevicePolicyValueNet(hp, md, state, side=cfg.n_cells, precision=precision, max_batch=int(net_max_batch), device=device)
        # (use_per is the trainer's switch: the episode loop refuses it)
        self.selfplay = SelfPlay(cfg, self.num_envs, dict(hp, use_per=False), md, infer=self.search_net.infer, seed=self.seed,
                                 env_id_offset=self.env_id_offset, **kw)
        if int(self.selfplay.spec.channels) != int(hp["input_channels"]) or not self.selfplay.replay.channels:
            self.close()
            raise ValueError(f"input_channels = {hp['input_channels']}: the ring's planes have {self.selfplay.spec.channels} channels "
                             f"(and the trainer needs them: planes=False is not for the learn loop)")
        self.trainer = Trainer(module, hp)

    # ------------------------------------------------------------------ checkpoints
    def _path(self, name: str) -> str:
        return os.path.join(self.checkpoint_dir, name)

    def save_checkpoint(self, name: str):
        """save_checkpoint (policy_value_network_wrappers.py:233-239)."""
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.torch.save({"state_dict": self.module.state_dict()}, self._path(name))

    def load_checkpoint(self, name: str):
        """load_checkpoint (:241-249) into the module, in place (the trainer's flat parameter buffers stay the parameters)."""
        ckpt = self.torch.load(self._path(name), map_location=next(self.module.parameters()).device)
        self.module.load_state_dict(ckpt["state_dict"], strict=True)

    def _save_replay(self):
        """replay_state.pt: the ring's state dict with its tensors on the host, and the iteration it belongs to.  Written to a temporary
        name and moved into place, BEFORE learn_state.pt: a learn_state.pt never names an iteration whose ring is not on disk."""
        torch = self.torch

        def to_host(x):
            if isinstance(x, torch.Tensor):
                return x.cpu()
            if isinstance(x, dict):
                return {k: to_host(v) for k, v in x.items()}
            return x

        os.makedirs(self.checkpoint_dir, exist_ok=True)
        tmp = self._path(REPLAY_FILE + ".tmp")
        torch.save(dict(iteration=int(self.iteration), replay=to_host(self.selfplay.state_dict())), tmp)
        os.replace(tmp, self._path(REPLAY_FILE))

    def _load_replay(self):
        path = self._path(REPLAY_FILE)
        if not os.path.exists(path):
            raise FileNotFoundError(f"persist_replay=True: {path} is missing ({REPLAY_FILE} is written beside {STATE_FILE} by a Learner "
                                    f"with persist_replay=True)")
        st = self.torch.load(path, map_location="cpu")
        if int(st["iteration"]) != self.iteration:
            raise ValueError(f"{REPLAY_FILE} holds the ring behind iteration {int(st['iteration'])}, {STATE_FILE} names iteration "
                             f"{self.iteration}")
        self.selfplay.load_state_dict(st["replay"])

    def _save_state(self):
        if self.persist_replay:
            self._save_replay()
        env = self.selfplay.env
        self.torch.save(dict(iteration=self.iteration, puct_init=self.puct_init, dirichlet_alpha=self.dirichlet_alpha,
                             prev_network_wins=self.prev_network_wins, reported=dict(self.reported), seed=self.seed,
                             env_id_offset=self.env_id_offset, episode=env.episode.cpu(), replay_draws=int(self.selfplay.replay.draws)),
                        self._path(STATE_FILE))

    def _resume(self):
        """Continue behind the last finished iteration: the schedules as they were applied, the deployed weights in the module and both
        device networks, the envs' episode counters and the ring's draw count (no episode and no minibatch draw comes twice).  The
        ring itself comes back only with persist_replay=True (replay_state.pt: a missing file or one of another iteration raises);
        otherwise the window starts empty.  Running episodes and pending rows are abandoned either way."""
        st = self.torch.load(self._path(STATE_FILE), map_location="cpu")
        if int(st["seed"]) != self.seed or int(st["env_id_offset"]) != self.env_id_offset:
            raise ValueError(f"learn_state.pt was written with seed {int(st['seed'])}, env_id_offset {int(st['env_id_offset'])}")
        self.iteration = int(st["iteration"])
        self.puct_init, self.dirichlet_alpha = float(st["puct_init"]), float(st["dirichlet_alpha"])
        self.prev_network_wins = int(st["prev_network_wins"])
        self.reported = {int(k): int(v) for k, v in st["reported"].items()}
        self.load_checkpoint(deployment_file(self.deployment_filename))
        self.trainer.hand_over(self.search_net)
        self.trainer.hand_over(self.trained_net)
        env = self.selfplay.env
        if tuple(st["episode"].shape) != tuple(env.episode.shape):
            raise ValueError(f"learn_state.pt holds {int(st['episode'].numel())} envs, this Learner {self.num_envs}")
        env.episode.copy_(st["episode"].to(env.episode.device))  # (begin_iteration's reset starts the episodes behind these)
        if self.persist_replay:
            self._load_replay()
        self.selfplay.replay.draws = int(st["replay_draws"])

    # ------------------------------------------------------------------ one iteration
    def _network_update(self, iteration: int) -> Optional[Dict]:
        """:389-398 and evaluate_trained_agent (:417-455).  Returns the arena's verdict (None with continuous_network_update)."""
        hp = self.hp
        deploy = deployment_file(self.deployment_filename)
        if hp.get("continuous_network_update", False):
            self.save_checkpoint(deploy)
            self.trainer.hand_over(self.search_net)
            return None
        from .arena import Arena

        self.trainer.hand_over(self.trained_net)
        # (the gate of iteration i plays episodes of its own: the arena's envs are keyed on another seed than self-play's)
        arena = Arena(self.cfg, self.arena_envs, dict(hp, use_per=False), self.md, self.search_net.infer, self.trained_net.infer,
                      seed=self.seed + 1 + int(iteration), env_id_offset=self.env_id_offset, **self._arena_kwargs)
        verdict = arena.evaluate()
        if verdict["accepted"]:
            self.save_checkpoint(deploy)
            self.trainer.hand_over(self.search_net)
        else:
            self.prev_network_wins += 1
            self.load_checkpoint(TEMP_FILE)
        return dict(verdict, prev_network_wins=self.prev_network_wins)

    def run_iteration(self, iteration: int) -> Dict:
        """Iteration `iteration` of learn (:305-398); returns its record."""
        torch, hp, sp = self.torch, self.hp, self.selfplay
        ring = sp.replay
        i = int(iteration)
        self.puct_init, self.dirichlet_alpha = exploration_schedule(dict(hp, puct_init=self.puct_init, dirichlet_alpha=self.dirichlet_alpha), i)
        sp.mcts.set_exploration(self.puct_init, self.dirichlet_alpha)
        t0 = time.perf_counter()
        totals = sp.run_iteration(i, self.episodes_per_env)
        t1 = time.perf_counter()
        self.reported[i] = int(totals["examples"])
        outdated = i - int(hp["max_train_examples_history"])  # (:364-368)
        if outdated >= 0:
            ring.flags[(ring.iter >= 0) & (ring.iter <= outdated) & (ring.flags == 2)] = 0
        self.save_checkpoint(TEMP_FILE)
        w = off_policy_window_size(hp, i)
        lo, hi = max(0, i - w + 1), i
        window = ring.window(lo, hi)
        length = len(window)
        evicted = sum(self.reported.get(j, 0) for j in range(lo, hi + 1)) - length
        t2 = time.perf_counter()
        epochs = self.trainer.train(window)
        t3 = time.perf_counter()
        self.save_checkpoint(snapshot_file(i))
        t4 = time.perf_counter()
        verdict = self._network_update(i)
        t5 = time.perf_counter()
        self.iteration = i
        self._save_state()
        return dict(iteration=i, totals=totals, puct_init=self.puct_init, dirichlet_alpha=self.dirichlet_alpha, window=(lo, hi),
                    window_length=length, evicted=int(evicted), epochs=epochs, arena=verdict,
                    seconds=dict(selfplay=t1 - t0, train=t3 - t2, update=t5 - t4))  # (host wall time: each phase ends with a device read)

    def learn(self, iterations: Optional[int] = None, resume: bool = False, on_iteration: Optional[Callable[[Dict], None]] = None):
        """learn (:254-415): the iterations behind the last finished one (resume=True: that of learn_state.pt, else none) up to
        num_self_play_iterations, at most `iterations` of them.  Returns one record per iteration run -- the totals of its self-play,
        the scheduled puct_init / dirichlet_alpha, the window (lo, hi), its length and `evicted` (the rows the window's iterations
        reported minus those still in the ring), the trainer's epoch means, the arena's verdict and the wall seconds of self-play, training
        and the network update -- and passes each to on_iteration."""
        if resume:
            self._resume()
        elif not os.path.exists(self._path(deployment_file(self.deployment_filename))):
            self.save_checkpoint(deployment_file(self.deployment_filename))  # (:266-268: the initial network is the first deployed one)
        first = self.iteration + 1
        last = int(self.hp["num_self_play_iterations"])
        if iterations is not None:
            last = min(last, first + int(iterations))
        out = []
        for i in range(first, last):
            rec = self.run_iteration(i)
            self.history.append(rec)
            out.append(rec)
            if on_iteration is not None:
                on_iteration(rec)
        return out

    def close(self):
        self.selfplay.close()
        self.search_net.close()
        self.trained_net.close()
