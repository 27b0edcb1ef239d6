"""The Humanoid task on the GPU through isaacgymenvs.make with the asset root at the packed fixture: the kernel form
it runs, 50 steps with resets on the fused tail against the torch statements, two PPO epochs with HumanoidPPO.yaml at
256 envs, and five at 4096 envs asserted finite throughout."""
import numpy as np
import pytest
import torch

from tests import humanoid_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(n, monkeypatch, **over):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    torch.manual_seed(42)
    over = {"task.env.asset.assetRoot": HC.GOLDEN, "task.env.asset.assetFileName": HC.MODEL, **over}
    return isaacgymenvs.make(seed=42, task="Humanoid", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True,
                             force_render=False, overrides=[f"{k}={v}" for k, v in over.items()])


def test_fused_tail_equals_torch_tail_over_a_run(monkeypatch):
    """Two envs built from the same seed, one on the fused tail and reset, one on the torch statements: the same
    physics kernel and the same device generator stream, 50 random-action steps of 20-step episodes (every env times
    out twice, falls reset others in between).  Done masks, time-outs and the generator position exactly; the
    observations, rewards and states to float rounding (Ant's tolerances, tests/test_humanoid_tail_gpu.py)."""
    n = 128
    gen = torch.Generator(device=DEV).manual_seed(9)
    acts = [2 * torch.rand((n, 21), device=DEV, generator=gen) - 1 for _ in range(50)]
    out = {}
    for mode in ("kernels", "torch"):
        env = _make(n, monkeypatch, **{"task.env.episodeLength": 20})
        assert env.sim.kernel_variant == 4 and env.sim.self_collide and env.sim.num_sensors == 2
        assert env.max_episode_length == 20 and env.num_obs == 108 and env.num_actions == 21
        assert env._tail is not None and env.num_bodies == 16 and env.num_dof == 21
        assert env.dof_force_tensor.shape == (n, 21) and env.vec_sensor_tensor.shape == (n, 12)
        if mode == "torch":
            env._tail = None
        res = []
        for a in acts:
            obs, rew, reset, extras = env.step(a)
            res.append((obs["obs"].clone(), rew.clone(), reset.clone(), extras["time_outs"].clone(),
                        env.root_states.clone(), env.dof_state.clone(), env.potentials.clone(),
                        torch.cuda.get_rng_state()))
        out[mode] = res
    resets, falls, force_max, sens_max = 0, 0, 0.0, 0.0
    angles = [7, 8, 9]
    other = [c for c in range(108) if c not in angles]
    for t, (a, b) in enumerate(zip(out["kernels"], out["torch"])):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all(), f"step {t}"
        assert a[2].dtype == torch.int64 and torch.equal(a[2], b[2]), f"reset mask step {t}"
        assert torch.equal(a[3], b[3]), f"time_outs step {t}"
        resets += int(a[2].sum())
        falls += int((a[2].bool() & ~a[3].bool()).sum())
        torch.testing.assert_close(a[0][:, other], b[0][:, other], rtol=1e-5, atol=1e-5, msg=f"obs step {t}")
        d = torch.remainder(a[0][:, angles] - b[0][:, angles] + np.pi, 2 * np.pi) - np.pi
        assert float(d.abs().max()) < 2e-5, f"angles step {t}"
        ulp = float(torch.finfo(torch.float32).eps) * float(b[6].abs().max())
        torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=2 * ulp, msg=f"reward step {t}")
        for i, what in ((4, "root states"), (5, "dof state"), (6, "potentials")):
            torch.testing.assert_close(a[i], b[i], rtol=1e-5, atol=1e-5, msg=f"{what} step {t}")
        assert torch.equal(a[7], b[7]), f"generator position step {t}"
        force_max = max(force_max, float(a[0][:, 54:75].abs().max()))
        sens_max = max(sens_max, float(a[0][:, 75:87].abs().max()))
    assert resets >= 2 * n and falls > 0  # two time-outs per env, and falls in between
    assert force_max > 0.1 and sens_max > 0.1  # the DOF force tensor and the foot sensors reach the observation


def test_humanoid_ppo_epochs(monkeypatch):
    """Two PPO epochs through rl/a2c_continuous.py with HumanoidPPO.yaml (units 400-200-100, mixed precision) at 256
    envs.

    The untrained policy's actions (sigma 1, clipped to +-1) are mostly saturated torques: with the dofs in
    DOF_MODE_NONE 3 of 256 envs held non-finite root states after the first 32-step rollout and a_loss was nan
    ("Stability").  The task's passive joint springs and dampers take that to about one env in
    10^5 env-steps, and the tail ends such an env as a fallen one (a zero observation, the death cost, the done flag),
    so nothing non-finite reaches the learner whether or not one occurs in these 16384 env-steps."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    n = 256
    cfg = compose("config", ["task=Humanoid"])
    env = _make(n, monkeypatch)
    agent = A2CAgent(env, PpoConfig.from_train_cfg(cfg["train"], minibatch_size=2048), device=DEV, seed=42)
    assert agent.num_minibatches == 4
    for _ in range(2):
        agent.train_epoch()
    s = agent.epoch_stats()
    assert np.isfinite(s["kl"]) and np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"])
    assert all(torch.isfinite(p).all() for p in agent.params)
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.root_states).all()
    assert torch.isfinite(agent.b_obs).all()  # every observation of the last rollout
    assert (env.envs[0].actors[0].dof_props["driveMode"] == 1).all() and env.sim.kernel_variant == 4
    assert agent.frame == 2 * 32 * n


def test_humanoid_stays_finite_over_a_long_run(monkeypatch):
    """Five PPO epochs at 4096 envs (655360 env-steps, where about six envs are expected to diverge: DESIGN.md section
    14): every stored observation, reward and value, the losses and the parameters stay finite after each epoch, and
    no env is left non-finite for longer than the step in which the tail ends it."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    n = 4096
    cfg = compose("config", ["task=Humanoid"])
    env = _make(n, monkeypatch)
    agent = A2CAgent(env, PpoConfig.from_train_cfg(cfg["train"]), device=DEV, seed=42)
    ended = 0
    for ep in range(5):
        agent.train_epoch()
        s = agent.epoch_stats()
        assert np.isfinite(s["kl"]) and np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"]), (ep, s)
        assert np.isfinite(s["mean_reward"]) and np.isfinite(s["mean_length"]), (ep, s)
        assert torch.isfinite(agent.b_obs).all() and torch.isfinite(agent.t_rewards).all(), ep
        assert torch.isfinite(agent.t_values).all() and torch.isfinite(agent.d_adv).all(), ep
        assert all(torch.isfinite(p).all() for p in agent.params), ep
        assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.rew_buf).all(), ep
        # a non-finite state lives for one step at most: whatever is non-finite now is flagged for the next reset
        bad = ~(torch.isfinite(env.root_states).all(dim=1) & torch.isfinite(env.dof_state.view(n, -1)).all(dim=1))
        assert (env.reset_buf[bad] == 1).all(), ep
        ended += int((agent.b_obs.abs().sum(dim=-1) == 0).sum())
    print(f"envs ended by the non-finite guard in 655360 env-steps: {ended}")
    assert agent.frame == 5 * 32 * n
