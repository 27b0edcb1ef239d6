"""The policy player without a GPU (isaacgymenv_amd/rl/player.py): PpoPlayerContinuous on the host backend, and the
plain Python restatement of the player's per-step bookkeeping (include/gymrl.h rl_play_post) that
tests/test_player_gpu.py holds the kernel to."""
import math

import numpy as np
import pytest
import torch


class PlayPostReference:
    """rl_play_post's statements, one env at a time: float32 counters, float64 totals (Python floats), the done envs
    added in ascending env order."""

    def __init__(self, n, games_num):
        self.cur_rewards = np.zeros(n, dtype=np.float32)
        self.cur_steps = np.zeros(n, dtype=np.float32)
        self.sum_rewards = 0.0
        self.sum_steps = 0.0
        self.games_played = 0
        self.finished = False
        self.games_num = games_num

    def step(self, rewards, dones):
        n = len(self.cur_rewards)
        for i in range(n):
            self.cur_rewards[i] = np.float32(self.cur_rewards[i] + np.float32(rewards[i]))
            self.cur_steps[i] = np.float32(self.cur_steps[i] + np.float32(1.0))
        if not self.finished:
            for i in range(n):
                if dones[i]:
                    self.sum_rewards += float(self.cur_rewards[i])
                    self.sum_steps += float(self.cur_steps[i])
                    self.games_played += 1
        if self.games_played >= self.games_num:
            self.finished = True
        for i in range(n):
            if dones[i]:
                self.cur_rewards[i] = 0.0
                self.cur_steps[i] = 0.0


def play_streams(n, steps, seed, done_p=0.2):
    """Synthetic (rewards [steps][n] f32, dones [steps][n] bool) streams."""
    rng = np.random.RandomState(seed)
    return (rng.randn(steps, n) * 3).astype(np.float32), rng.rand(steps, n) < done_p


@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("flag_dtype", [torch.bool, torch.int64])
def test_host_bookkeeping_matches_the_restatement(n, flag_dtype):
    """player.play_post_host (the sim_device=cpu path of run()) against the restatement: exact."""
    from isaacgymenv_amd.rl.player import play_post_host
    rew, done = play_streams(n, 50, seed=n)
    ref = PlayPostReference(n, 7)
    cr, cs = torch.zeros(n), torch.zeros(n)
    sums, games = torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    for t in range(50):
        ref.step(rew[t], done[t])
        play_post_host(torch.from_numpy(rew[t]), torch.from_numpy(done[t]).to(flag_dtype), cr, cs, sums, games, 7)
        assert games.tolist() == [ref.games_played, int(ref.finished)]
        assert sums.tolist() == [ref.sum_rewards, ref.sum_steps]
        np.testing.assert_array_equal(cr.numpy(), ref.cur_rewards)
        np.testing.assert_array_equal(cs.numpy(), ref.cur_steps)
    if n > 1:
        assert ref.finished


def _cartpole_player(monkeypatch, seed=42, **kw):
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    from isaacgymenv_amd.rl import PpoConfig, PpoPlayerContinuous
    import isaacgymenvs
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    env = isaacgymenvs.make(seed=seed, task="Cartpole", num_envs=16, sim_device="cpu", rl_device="cpu", headless=True,
                            overrides=["pipeline=cpu"])
    pcfg = PpoConfig.from_train_cfg(compose("config", ["task=Cartpole"])["train"])
    return PpoPlayerContinuous(env, pcfg, device="cpu", seed=seed, games_num=8, **kw)


def test_player_runs_to_finished_on_the_host_backend_and_is_deterministic(monkeypatch):
    lines = []
    stats = []
    for _ in range(2):
        player = _cartpole_player(monkeypatch)
        stats.append(player.run(printer=lines.append))
        assert player.last_path == "torch"
    s = stats[0]
    assert s["games_played"] >= 8 and s["steps"] % 16 == 0 and s["steps"] < 27000
    assert math.isfinite(s["av_reward"]) and math.isfinite(s["av_steps"]) and s["av_steps"] >= 1.0
    assert stats[0] == stats[1]
    assert len(lines) == 2 and lines[0].startswith("av reward:") and "av steps:" in lines[0]


def test_player_defaults_follow_rl_games_and_the_player_block(monkeypatch):
    from isaacgymenv_amd.rl.player import PpoPlayerContinuous
    player = _cartpole_player(monkeypatch)
    assert player.games_num == 8 and player.is_deterministic is True and player.max_steps == 27000
    p2 = PpoPlayerContinuous(player.env, player.cfg, device="cpu")
    assert (p2.games_num, p2.is_deterministic, p2.print_stats) == (2000, True, True)
    p3 = PpoPlayerContinuous(player.env, player.cfg, device="cpu",
                             player_cfg={"games_num": 5, "deterministic": False, "print_stats": False})
    assert (p3.games_num, p3.is_deterministic, p3.print_stats) == (5, False, False)
    # deterministic play returns the mean; sampled play differs from it and is clamped (Cartpole: clip_actions)
    obs = torch.randn(16, 4)
    a = player.get_action(obs, True)
    assert torch.equal(a, player.get_action(obs, True)) and a.shape == (16, 1)
    b = player.get_action(obs, False)
    assert not torch.equal(a, b) and float(b.abs().max()) <= 1.0


def test_player_restores_a_checkpoint_without_an_optimizer_entry(monkeypatch, tmp_path):
    from isaacgymenv_amd.rl import A2CAgent
    player = _cartpole_player(monkeypatch)
    agent = A2CAgent(player.env, player.cfg.__class__(**{**player.cfg.__dict__, "minibatch_size": 256}), device="cpu",
                     seed=7)
    with torch.no_grad():
        agent.model.running_mean_std.running_mean += 0.25
        agent.model.running_mean_std.running_var *= 1.5
    full, bare = tmp_path / "full.pth", tmp_path / "bare.pth"
    agent.save(str(full))
    torch.save({"model": agent.model.state_dict()}, str(bare))
    for path in (full, bare):
        fresh = _cartpole_player(monkeypatch, seed=1)
        fresh.restore(str(path))
        want, got = agent.model.state_dict(), fresh.model.state_dict()
        assert list(want) == list(got)
        for k in want:
            assert want[k].dtype == got[k].dtype and torch.equal(want[k], got[k]), k
        assert not fresh.model.training


def test_launch_refuses_multi_gpu_play():
    from isaacgymenv_amd.isaacgymenvs.train import launch
    with pytest.raises(ValueError, match="multi_gpu"):
        launch(["task=Cartpole", "test=True", "multi_gpu=True", "sim_device=cpu", "rl_device=cpu", "pipeline=cpu"])


def test_launch_test_true_plays_without_training_or_writing(monkeypatch, tmp_path):
    """test=True on the host pipeline: a player comes back, no learner runs, nothing is written."""
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    from isaacgymenv_amd.isaacgymenvs.train import launch
    from isaacgymenv_amd.rl import PpoPlayerContinuous
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    monkeypatch.chdir(tmp_path)
    player, stats = launch(["task=Cartpole", "test=True", "num_envs=16", "sim_device=cpu", "rl_device=cpu",
                            "pipeline=cpu"], printer=None, games_num=4)
    assert isinstance(player, PpoPlayerContinuous)
    assert stats["games_played"] >= 4 and math.isfinite(stats["av_reward"])
    assert not (tmp_path / "runs").exists() and not any(tmp_path.iterdir())
