"""The flat tasks' fused tail and reset (libgymtask gt_flat_post_physics / gt_flat_reset_flagged) vs the torch statements
of tasks/anymal.py on the same GPU tensors (the torch path is the golden-tested specification,
tests/test_flat_tasks_cpu.py), and vs the recordings of the reference itself (tests/golden/anymal_flat.npz,
hound_flat.npz).  Tolerance: float32 rounding of differently fused expressions, rtol 1e-5 / atol 1e-5; the done mask
and its count exactly; the fused reset bit-identical, generator position included."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from tests.fakegym_flat import TASKS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _make(task, n, monkeypatch):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    torch.manual_seed(42)
    return isaacgymenvs.make(seed=42, task=task, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                             force_render=False)


def _stepped(task, n, steps, seed, monkeypatch):
    env = _make(task, n, monkeypatch)
    assert env._tail is not None
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    for _ in range(steps):
        env.step(2 * torch.rand((n, 12), device="cuda:0", generator=gen) - 1)
    return env


@pytest.mark.parametrize("task", ["Anymal", "Hound"])
def test_tail_kernel_matches_torch_tail(task, monkeypatch):
    """300 envs: four full waves and a partial one, more than one workgroup."""
    from isaacgymenv_amd.isaacgymenvs.tasks.anymal import compute_flat_observations, compute_flat_reward
    n = 300
    env = _stepped(task, n, 20, 5, monkeypatch)
    env.progress_buf[: n // 8] = env.max_episode_length - 1  # the episode-end branch
    env.contact_forces[n // 8: n // 4, int(env.knee_indices[-1])] = torch.tensor([0.0, 2.0, 0.0], device="cuda:0")
    env.contact_forces[n // 4: n // 4 + 9, env.base_index, 2] = 1.5
    torch.cuda.synchronize()
    obs = compute_flat_observations(env.root_states, env.commands, env.dof_pos, env.default_dof_pos, env.dof_vel,
                                    env.gravity_vec, env.actions, env.lin_vel_scale, env.ang_vel_scale,
                                    env.dof_pos_scale, env.dof_vel_scale)
    rew, reset = compute_flat_reward(env.root_states, env.commands, env.torques, env.contact_forces, env.knee_indices,
                                     env.progress_buf, env.rew_scales, env.base_index, env.max_episode_length)
    env._tail()
    torch.cuda.synchronize()
    torch.testing.assert_close(env.obs_buf, obs, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(env.rew_buf, rew, rtol=1e-5, atol=1e-5)
    assert env.reset_buf.dtype == torch.int64 and torch.equal(env.reset_buf, reset.long())
    assert int(reset.sum()) >= n // 4 and env._tail.done_count() == int(reset.sum())
    assert float(env.torques.abs().max()) > 0.1 and (rew > 0).any()


@pytest.mark.parametrize("kind", ["anymal", "hound"])
def test_tail_kernel_matches_reference_golden(kind, monkeypatch):
    """gt_flat_post_physics pinned directly to the reference's outputs: each recorded step's tail inputs (after reset_idx
    and the refreshes) are loaded into the GPU env's tensors, and the kernel's observations, reward and done mask are
    compared with what the reference computed from them."""
    from isaacgymenv_amd.isaacgymenvs.tasks import anymal as flat
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    d = np.load(os.path.join(GOLDEN, TASKS[kind][1]))
    cfg = yaml.safe_load(str(d["cfg_yaml"]))
    cfg["sim"]["use_gpu_pipeline"] = True
    cfg["sim"]["physx"]["use_gpu"] = True
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    dev = "cuda:0"
    torch.manual_seed(42)
    env = getattr(flat, TASKS[kind][0])(copy.deepcopy(cfg), dev, dev, -1, True, False, False)
    assert env._tail is not None and env.max_episode_length == int(d["max_episode_length"])
    np.testing.assert_array_equal(env.knee_indices.cpu().numpy(), d["knee_indices"])
    assert env.base_index == int(d["base_index"])
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    T, n = d["out_obs"].shape[0], d["out_obs"].shape[1]
    assert n == env.num_envs and (d["out_rew"] == 0).any() and (d["out_rew"] > 0).any() and d["out_reset"].sum() > 0
    for t in range(T):
        env.root_states.copy_(g(d["in_root"][t]))
        env.dof_state.copy_(g(d["in_dof"][t]))
        env.contact_forces.copy_(g(d["in_contact"][t]))
        env.torques.copy_(g(d["in_torques"][t]))
        env.actions = g(d["in_actions"][t]).clone()
        env.commands.copy_(g(d["in_commands"][t]))
        env.progress_buf.copy_(g(d["in_progress"][t]))
        env._tail()
        torch.cuda.synchronize()
        np.testing.assert_allclose(env.obs_buf.cpu().numpy(), d["out_obs"][t], rtol=1e-5, atol=1e-5, err_msg=f"obs {t}")
        np.testing.assert_allclose(env.rew_buf.cpu().numpy(), d["out_rew"][t], rtol=1e-5, atol=1e-5, err_msg=f"rew {t}")
        np.testing.assert_array_equal(env.reset_buf.cpu().numpy(), d["out_reset"][t], err_msg=f"reset step {t}")
        assert env._tail.done_count() == int(d["out_reset"][t].sum())


def _reset_both_ways(env, flagged, k):
    names = ("dof_state", "commands", "progress_buf", "reset_buf")
    snap = {a: getattr(env, a).clone() for a in names}
    state0 = env.sim.state.clone()
    rng = torch.cuda.get_rng_state()
    env.reset_idx(flagged)
    torch.cuda.synchronize()
    want = {a: getattr(env, a).clone() for a in names}
    want_state, want_rng = env.sim.state.clone(), torch.cuda.get_rng_state()
    for a in names:
        getattr(env, a).copy_(snap[a])
    env.sim.state.copy_(state0)
    torch.cuda.set_rng_state(rng)
    ids = env._tail.reset_flagged(k)
    torch.cuda.synchronize()
    assert torch.equal(ids.long(), flagged)
    for a in names:
        assert torch.equal(getattr(env, a), want[a]), a
    assert torch.equal(env.sim.state, want_state)
    assert torch.equal(torch.cuda.get_rng_state(), want_rng)
    assert (env.reset_buf[flagged] == 1).all() and (env.progress_buf[flagged] == 0).all()


@pytest.mark.parametrize("task", ["Anymal", "Hound"])
def test_fused_reset_matches_torch_reset_idx(task, monkeypatch):
    """gt_flat_reset_flagged vs the torch reset_idx from the same state and the same device generator position: the dof
    state, commands, counters and the sim state after the indexed sets are bit-identical, and the generator ends where
    the five torch_rand_float calls leave it; then the same with exactly one env flagged (the .squeeze() path)."""
    n = 300
    env = _stepped(task, n, 10, 9, monkeypatch)
    env.progress_buf[:] = 3
    env.contact_forces[:] = 0.0
    env.progress_buf[5: n: 7] = env.max_episode_length - 1   # flagged envs in every wave, the partial one included
    env._tail()
    torch.cuda.synchronize()
    k = env._tail.done_count()
    flagged = env.reset_buf.nonzero(as_tuple=False).flatten()
    assert k == len(flagged) == len(range(5, n, 7)) and int(flagged[-1]) >= 256
    _reset_both_ways(env, flagged, k)
    # exactly one env, in the last (partial) wave
    env.progress_buf[:] = 3
    env.progress_buf[n - 2] = env.max_episode_length - 1
    env._tail()
    torch.cuda.synchronize()
    flagged = env.reset_buf.nonzero(as_tuple=False).flatten()
    assert env._tail.done_count() == 1 and flagged.tolist() == [n - 2]
    _reset_both_ways(env, flagged, 1)


def test_invalid_link_indices_are_refused():
    """The entry points validate what indexes memory before any launch."""
    from isaacgymenv_amd import gymtask
    L = gymtask.lib()
    keep = torch.zeros(4096, device="cuda:0")
    p = gymtask.GtFlatParams()
    p.num_envs, p.num_dofs, p.num_bodies, p.base_index, p.num_knees = 4, 12, 13, 0, 4
    p.knee_idx[:4] = [2, 5, 8, 13]  # one past the last link
    b = gymtask.GtFlatBuffers()
    for name, _ in gymtask.GtFlatBuffers._fields_:
        if name != "seq":
            setattr(b, name, keep.data_ptr())
    assert L.gt_flat_post_physics(ctypes.byref(p), ctypes.byref(b), None) != 0
    assert "gt_flat_post_physics" in L.gt_last_error().decode()
