"""The flat-ground tasks Anymal and Hound on the GPU through isaacgymenvs.make: the kernel form each runs, the fused
tail and reset against the torch statements across resets, and two PPO epochs with AnymalPPO.yaml."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 256


def _make(task, monkeypatch, **over):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    torch.manual_seed(42)
    return isaacgymenvs.make(seed=42, task=task, num_envs=N, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                             force_render=False, overrides=[f"{k}={v}" for k, v in over.items()])


@pytest.mark.parametrize("task,variant", [("Anymal", 1), ("Hound", 4)])
def test_kernel_tail_equals_torch_tail_across_resets(task, variant, monkeypatch):
    """Two envs built from the same seed, one on the fused tail and reset, one on the torch statements: the same
    physics kernel and the same device generator stream, 30 random-action steps of 10-step episodes (every env times
    out twice, contacts reset others in between).  Done masks, time-outs and the generator position exactly; the
    observations, rewards and states to float rounding."""
    over = {"task.env.learn.episodeLength_s": 0.2}
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    acts = [2 * torch.rand((N, 12), device="cuda:0", generator=gen) - 1 for _ in range(30)]
    out = {}
    for mode in ("kernels", "torch"):
        env = _make(task, monkeypatch, **over)
        assert env.sim.kernel_variant == variant and env.max_episode_length == 10
        assert env._tail is not None and env.num_obs == 48 and env.torques.shape == (N, 12)
        if mode == "torch":
            env._tail = None
        res = []
        for a in acts:
            obs, rew, reset, extras = env.step(a)
            res.append((obs["obs"].clone(), rew.clone(), reset.clone(), extras["time_outs"].clone(),
                        env.root_states.clone(), env.dof_state.clone(), env.commands.clone(), env.torques.clone(),
                        torch.cuda.get_rng_state()))
        out[mode] = res
    reset_steps, torque_max = 0, 0.0
    for t, (a, b) in enumerate(zip(out["kernels"], out["torch"])):
        assert a[2].dtype == torch.int64 and torch.equal(a[2], b[2]), f"reset mask step {t}"
        assert torch.equal(a[3], b[3]), f"time_outs step {t}"
        reset_steps += int(bool(a[2].any()))
        torch.testing.assert_close(a[0], b[0], rtol=1e-5, atol=1e-5, msg=f"obs step {t}")
        torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=1e-6, msg=f"reward step {t}")
        for i, what in ((4, "root states"), (5, "dof state"), (6, "commands"), (7, "torques")):
            torch.testing.assert_close(a[i], b[i], rtol=1e-5, atol=1e-5, msg=f"{what} step {t}")
        assert torch.equal(a[8], b[8]), f"generator position step {t}"
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and (a[1] >= 0).all()
        torque_max = max(torque_max, float(a[7].abs().max()))
    assert reset_steps >= 2 and torque_max > 1.0  # the drives' forces reach the reward


def test_anymal_ppo_epochs(monkeypatch):
    """Two PPO epochs through rl/a2c_continuous.py with AnymalPPO.yaml (shared trunk, mixed precision) at 256 envs."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    cfg = compose("config", ["task=Anymal"])
    env = _make("Anymal", monkeypatch)
    agent = A2CAgent(env, PpoConfig.from_train_cfg(cfg["train"], minibatch_size=2048), device="cuda:0", seed=42)
    assert agent.num_minibatches == 3
    for _ in range(2):
        agent.train_epoch()
    s = agent.epoch_stats()
    assert np.isfinite(s["kl"]) and np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"])
    assert all(torch.isfinite(p).all() for p in agent.params)
    assert agent.frame == 2 * 24 * N


def test_anymal_cpu_tensors_on_the_gpu_sim(monkeypatch):
    """pipeline=cpu with sim_device=cuda:0: the physics kernels run on the GPU, the tensors live on the host
    (Sim.refresh's third case) -- the DOF force tensor arrives there through its device mirror."""
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    env = isaacgymenvs.make(seed=3, task="Anymal", num_envs=64, sim_device="cuda:0", rl_device="cpu", headless=True,
                            force_render=False, overrides=["pipeline=cpu"])
    assert env.device == "cpu" and env._tail is None and env.sim.kernel_variant == 1
    assert env.torques.device.type == "cpu" and env.sim.dof_force_soa.is_cuda
    gen = torch.Generator().manual_seed(0)
    for _ in range(3):
        obs, rew, reset, extras = env.step(2.0 * torch.rand(64, 12, generator=gen) - 1.0)
    assert torch.isfinite(obs["obs"]).all() and torch.isfinite(env.torques).all() and env.torques.abs().max() > 1.0
    torch.cuda.synchronize()
    assert torch.equal(env.torques.reshape(-1), env.sim._dof_force_dev.cpu())
    assert torch.equal(env.torques, env.sim.dof_force_soa.t().cpu())
