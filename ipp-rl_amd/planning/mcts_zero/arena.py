"""
Arena: the network gate of the MCTS-zero loop -- Arena.play_game(s) (planning/mcts_zero/arenas.py:25-56) and evaluate_trained_agent
(planning/mcts_zero/mcts_zero_mission.py:417-455) for a batch of envs on one device.  The previous and the new network each play
num_games episodes with the temperature-0 player (VecMctsZeroPolicy(mode="arena")); the new one is kept only if
total_curr / (total_prev + total_curr) >= network_update_threshold (:435-436).

Each player gets its OWN freshly built VecIPPEnv with the same cfg, seed and env_id_offset, one after the other (the first is closed
before the second is built).  The env's randomness is keyed on (global env id, episode), so game (e, j) is the same game -- ground truth,
start budget, measurement noise stream -- for both players: the games are paired.  (env.reset() advances the episode counters: one env
played twice would not pair them.)

Divergences from the reference (INTEGRATION.md "Deployment and arena"): two networks, not the same search object twice; games end with
the env's ledger; games are real episodes; Dirichlet noise keyed per root.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

from ..vec_mcts_zero import VecMctsZeroPolicy, gate, make_env


class Arena:
    def __init__(self, cfg, num_envs: int, hyper_params: Dict, meta_data: Dict, infer_prev: Optional[Callable],
                 infer_curr: Optional[Callable], seed: int = 0, env_id_offset: int = 0, device: str = "cuda:0", workers: int = 1,
                 sims_in_flight: int = 4, tie_break: str = "first", groups: int = 2, **env_kwargs):
        """cfg: EngineConfig; hyper_params / meta_data: the reference's dictionaries, as for SelfPlay; infer_prev / infer_curr: the two
        players' DeviceMCTS network callbacks (None: uniform priors, value 0).  workers: searches per decision (the reference's arena
        players run one).  env_kwargs go to VecIPPEnv; the defaults are SelfPlay's, with node_capacity / max_batch sized for `workers`."""
        if meta_data.get("initial_budget") is None:
            raise ValueError("the arena plays budget-mode episodes: meta_data['initial_budget'] is needed")
        self.cfg, self.num_envs = cfg, int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.hp, self.md = dict(hyper_params), dict(meta_data)
        self.infer_prev, self.infer_curr = infer_prev, infer_curr
        self.seed, self.env_id_offset, self.device = int(seed), int(env_id_offset), device
        self.workers, self.sims_in_flight, self.tie_break, self.groups = int(workers), int(sims_in_flight), tie_break, int(groups)
        self.env_kwargs = dict(env_kwargs)
        self.last = None  # per player the game_values / game_steps [B, G] (host arrays) of the last play_games

    def _play(self, infer, games_per_env: int):
        """One player's games on its own env.  Returns (total, game_values [B, G], game_steps [B, G]) on the host."""
        hp, md, B = self.hp, self.md, self.num_envs
        env = make_env(self.cfg, B, hp, md, workers=self.workers, sims_in_flight=self.sims_in_flight, seed=self.seed,
                       env_id_offset=self.env_id_offset, device=self.device, **self.env_kwargs)
        try:
            player = VecMctsZeroPolicy(env, hp, md, infer, workers=self.workers, mode="arena", games_per_env=games_per_env,
                                       sims_in_flight=self.sims_in_flight, tie_break=self.tie_break, groups=self.groups, seed=self.seed)
            out = player.play()
            if out["games"] != B * games_per_env:
                raise RuntimeError(f"{out['games']} of {B * games_per_env} arena games ended within their step limit")
            return out["total"], out["game_values"].cpu().numpy(), out["game_steps"].cpu().numpy()
        finally:
            env.close()

    def play_games(self, num_games: int):
        """(total_rewards_prev, total_rewards_curr) over num_games games per player (arenas.py:47-56); num_games must be a multiple of
        num_envs: env e plays games e, e + ... of its own episode sequence, the same games for both players."""
        num_games = int(num_games)
        if num_games < 1 or num_games % self.num_envs:
            raise ValueError(f"num_games = {num_games} is not a positive multiple of num_envs = {self.num_envs}")
        G = num_games // self.num_envs
        prev = self._play(self.infer_prev, G)
        curr = self._play(self.infer_curr, G)
        self.last = dict(prev=dict(game_values=prev[1], game_steps=prev[2]), curr=dict(game_values=curr[1], game_steps=curr[2]))
        return prev[0], curr[0]

    def evaluate(self, num_games: Optional[int] = None, threshold: Optional[float] = None):
        """evaluate_trained_agent (:430-453): dict(accepted, ratio, total_prev, total_curr, avg_reward_curr)."""
        num_games = int(self.hp["num_arena_games"] if num_games is None else num_games)
        threshold = float(self.hp["network_update_threshold"] if threshold is None else threshold)
        total_prev, total_curr = self.play_games(num_games)
        accepted, ratio = gate(total_prev, total_curr, threshold)
        return dict(accepted=accepted, ratio=ratio, total_prev=total_prev, total_curr=total_curr, avg_reward_curr=total_curr / num_games)
