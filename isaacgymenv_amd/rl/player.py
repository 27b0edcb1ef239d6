"""The policy player (rl_games ``players.py`` PpoPlayerContinuous / BasePlayer.run, rl-games 1.6.x semantics):
load a checkpoint, run inference only, report the episode reward and length of the policy.

The reference reaches it with ``python train.py task=Ant checkpoint=runs/Ant/nn/Ant.pth test=True num_envs=64``
(isaacgymenvs/train.py passes ``'play': cfg.test`` to the rl_games runner); rl_games is not vendored, so the
player is restated here from its published algorithm, as the learner is (a2c_continuous.py):

* ``get_action(obs, is_deterministic)``: the model's eval forward, ``mus`` when deterministic and the sampled
  ``actions`` otherwise, clamped to [-1, 1] with ``clip_actions`` (the action space is [-1, 1]: rescale_actions is
  the identity).  On the GPU the whole forward -- frozen input normalisation, the actor MLP, the mu head, the
  action -- is ONE launch (gae.PolicyInfer, rl_policy_infer) where the network fits it and the env count is at
  most ``INFER_MAX_ENVS``; elsewhere the model's own eval forward runs (the torch statements on the host).
* ``run()``: ``env.reset()`` once, then get_action -> env.step -> the episode bookkeeping (rl_play_post on the
  GPU, the same statements in torch on the host) until ``games_num`` episodes have finished or ``max_steps``;
  prints and returns the per-run averages rl_games prints (``av reward``, ``av steps``).

Checkpoints: ``restore`` loads the ``"model"`` entry of a file written by ``A2CAgent.save`` (network parameters
and both RunningMeanStd buffers; an ``"optimizer"`` entry may be present or absent and is ignored).  The state-dict
key names follow rl_games' names, but a file written by rl_games itself has not been loaded here (rl_games is not
available to this project's tests): no claim is made about it.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import gae
from .a2c_continuous import PpoConfig
from .network import ActorCriticNetwork, Linear, ModelA2CContinuousLogStd

# The largest env count at which get_action takes rl_policy_infer: the largest measured N at which the one-launch
# kernel was not slower than the model's eval forward beyond the run-to-run spread (the table is in
# profiles/player_infer_timing.txt and DESIGN.md section 9).  Above it the model's own forward runs.
INFER_MAX_ENVS = 4096

POLL_EVERY = 16  # steps between reads of the device's `finished` flag (the only host synchronisation of run())
DEFAULT_GAMES_NUM = 2000  # rl_games BasePlayer: player.games_num
DEFAULT_MAX_STEPS = 27000  # rl_games BasePlayer: 108000 // 4


def play_post_host(rewards, dones, cur_rewards, cur_steps, sums, games, games_num: int) -> None:
    """rl_play_post's statements (include/gymrl.h) on host tensors: f32 counters, float64 totals, the done envs
    added one by one in ascending env order."""
    cur_rewards += rewards
    cur_steps += 1.0
    done = dones != 0
    if int(games[1]) == 0:
        idx = done.nonzero().flatten().tolist()
        sr, ss = float(sums[0]), float(sums[1])
        for i in idx:
            sr += float(cur_rewards[i])
            ss += float(cur_steps[i])
        sums[0], sums[1] = sr, ss
        games[0] += len(idx)
        if int(games[0]) >= games_num:
            games[1] = 1
    cur_rewards[done] = 0.0
    cur_steps[done] = 0.0


class PpoPlayerContinuous:
    """rl_games PpoPlayerContinuous over a VecTask.  ``player_cfg``: ``params.config.player`` of the train config
    where present (games_num, deterministic, print_stats; rl_games' defaults 2000, True, True otherwise);
    ``games_num`` / ``deterministic`` override it."""

    def __init__(self, env, cfg: PpoConfig, device: Optional[str] = None, seed: Optional[int] = None,
                 player_cfg: Optional[Dict[str, Any]] = None, games_num: Optional[int] = None,
                 deterministic: Optional[bool] = None):
        self.env = env
        self.cfg = cfg
        self.device = torch.device(device or env.rl_device)
        self.num_envs = env.num_envs
        self.obs_dim = env.num_obs
        self.actions_num = env.num_actions
        pc = dict(player_cfg or {})
        self.games_num = int(games_num if games_num is not None else pc.get("games_num", DEFAULT_GAMES_NUM))
        self.is_deterministic = bool(deterministic if deterministic is not None else pc.get("deterministic", True))
        self.print_stats = bool(pc.get("print_stats", True))
        self.max_steps = DEFAULT_MAX_STEPS
        if seed is not None:
            torch.manual_seed(seed)
        net = ActorCriticNetwork(self.obs_dim, self.actions_num, cfg.units, cfg.activation, cfg.separate,
                                 cfg.fixed_sigma, cfg.sigma_init_val)
        self.model = ModelA2CContinuousLogStd(net, self.obs_dim, cfg.normalize_input, cfg.normalize_value)
        self.model.to(self.device)
        self.model.eval()
        self.last_path: Optional[str] = None  # "rl_policy_infer" or "torch": what the last get_action ran
        self._infer = None
        self._infer_decided = False

    # ------------------------------------------------------------------ checkpoints
    def restore(self, path: str) -> None:
        """Load the ``"model"`` entry (parameters and running-moment buffers) in place; nothing else is read."""
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        self.model.load_state_dict(ckpt["model"])
        self.model.eval()

    # ------------------------------------------------------------------ the forward
    def _bind_infer(self):
        """gae.PolicyInfer over the model's own parameters where rl_policy_infer applies: a GPU model, fixed sigma,
        an actor MLP of Linear + ELU(alpha 1) layers within the kernel's limits."""
        self._infer_decided = True
        net = self.model.a2c_network
        if self.device.type != "cuda" or not net.fixed_sigma:
            return
        mods = list(net.actor_mlp)
        if len(mods) % 2:
            return
        layers = []
        for lin, act in zip(mods[0::2], mods[1::2]):
            if not (isinstance(lin, Linear) and lin.bias is not None and type(act) is torch.nn.ELU
                    and act.alpha == 1.0 and lin.weight.dtype == torch.float32):
                return
            layers.append((lin.weight.detach(), lin.bias.detach()))
        if net.mu.bias is None or not gae.policy_infer_fits(self.obs_dim, [w.shape[0] for w, _ in layers],
                                                             self.actions_num):
            return
        rms = self.model.running_mean_std if self.model.normalize_input else None
        self._infer = gae.PolicyInfer(layers, net.mu.weight.detach(), net.mu.bias.detach(), net.sigma.detach(), rms)

    @torch.no_grad()
    def get_action(self, obs, is_deterministic: Optional[bool] = None):
        """rl_games PpoPlayerContinuous.get_action: the action for each row of obs [N, obs_dim]."""
        det = self.is_deterministic if is_deterministic is None else bool(is_deterministic)
        if isinstance(obs, dict):
            obs = obs["obs"]
        if not self._infer_decided:
            self._bind_infer()
        N = obs.shape[0]
        if (self._infer is not None and N <= INFER_MAX_ENVS and obs.is_cuda and obs.device == self._infer.device
                and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == self.obs_dim
                and obs.is_contiguous()):
            noise = None
            if not det:  # the learner's draw (network.py act forward): one [N, A] normal_ call
                noise = torch.empty(N, self.actions_num, dtype=torch.float32, device=obs.device).normal_(0.0, 1.0)
            actions, _ = self._infer(obs, noise, clip=self.cfg.clip_actions)
            self.last_path = "rl_policy_infer"
            return actions
        res = self.model({"is_train": False, "obs": obs})
        actions = res["mus"] if det else res["actions"]
        if self.cfg.clip_actions:
            actions = torch.clamp(actions, -1.0, 1.0)
        self.last_path = "torch"
        return actions

    # ------------------------------------------------------------------ the loop
    def run(self, max_steps: Optional[int] = None, printer=print) -> Dict[str, float]:
        """rl_games BasePlayer.run for a vectorised env: one reset, then steps until ``games_num`` episodes have
        finished (every env finishing in the crossing step counts) or ``max_steps``.  Returns ``av_reward`` and
        ``av_steps`` (the totals over ``games_played``; NaN when no episode finished), ``games_played``, ``steps``."""
        max_steps = int(max_steps if max_steps is not None else self.max_steps)
        N = self.num_envs
        obs = self.env.reset()
        state_dev = None
        cur_rewards = cur_steps = sums = games = None
        steps = 0
        for n in range(max_steps):
            actions = self.get_action(obs)
            obs, rewards, dones, _ = self.env.step(actions)
            if state_dev is None:  # the bookkeeping lives where the env's outputs do
                state_dev = rewards.device
                cur_rewards = torch.zeros(N, dtype=torch.float32, device=state_dev)
                cur_steps = torch.zeros(N, dtype=torch.float32, device=state_dev)
                sums = torch.zeros(2, dtype=torch.float64, device=state_dev)
                games = torch.zeros(2, dtype=torch.int64, device=state_dev)
            if state_dev.type == "cuda":
                gae.play_post(rewards if rewards.is_contiguous() else rewards.contiguous(), dones, cur_rewards,
                              cur_steps, sums, games, self.games_num, state_checked=n > 0)
            else:
                play_post_host(rewards, dones, cur_rewards, cur_steps, sums, games, self.games_num)
            steps = n + 1
            if steps % POLL_EVERY == 0 and int(games[1]) != 0:
                break
        played = int(games[0]) if games is not None else 0
        sr, ss = (float(sums[0]), float(sums[1])) if sums is not None else (0.0, 0.0)
        stats = {"av_reward": sr / played if played else float("nan"),
                 "av_steps": ss / played if played else float("nan"), "games_played": played, "steps": steps}
        if self.print_stats and printer:
            printer(f"av reward: {stats['av_reward']} av steps: {stats['av_steps']} games: {played}")
        return stats
