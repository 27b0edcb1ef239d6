"""Houndarm on the GPU: the fused kernels (libgymtask gt_arm_control / gt_arm_post_physics / gt_arm_reset_flagged), the
simulator's gravity switch on the runtime-sized and the one-env-per-lane kernels, and the task on the real simulator.

* gt_arm_control on the recorded control inputs (tests/golden/houndarm.npz) against the fixture's float64 restatement,
  |got - ref| <= 1e-4 max(1, |ref|) (the gt_hound_control rule), the effort tensor bit-equal to the torques;
* gt_arm_post_physics replaying the recording (reset, progress and the done count exact, obs / rew at rtol 1e-5 /
  atol 2e-6), and against the task's torch statements on seeded random inputs at 130 envs (two full waves and a
  partial one); gt_arm_reset_flagged against the torch reset_idx from the same generator position, bit for bit;
* the arm fixture under AssetOptions.disable_gravity against the oracle with zero gravity in its own parameters;
* the task: finite outputs, resets, kernel variant 4, fused kernels in use, and the end-effector holding its height
  where a sim with the flag forced off lets it sag.
"""
import copy
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch
import yaml

from tests import arm_cases as A
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WAVES = 130  # two full waves and a partial one


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(A.GOLDEN, "houndarm.npz"))


def _gpu_env(fixture, n, monkeypatch, episode_length=A.EPISODE_LENGTH, gravity_off=True):
    """Houndarm on the real simulator from the fixture's config (GPU pipeline)."""
    from isaacgymenv_amd.isaacgym import gymapi
    from isaacgymenv_amd.isaacgymenvs.tasks import hound_arm
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    cfg = A.point_at_fixture(yaml.safe_load(str(fixture["cfg_yaml"])))
    cfg["env"]["numEnvs"] = n
    cfg["env"]["episodeLength"] = episode_length
    cfg["sim"]["use_gpu_pipeline"] = True
    cfg["sim"]["physx"]["use_gpu"] = True
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)

    class WithGravity(hound_arm.Houndarm):  # the flag forced off: what today's physics would do to the task
        def _asset_options(self):
            opts = super()._asset_options()
            opts.disable_gravity = False
            return opts

    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        cls = hound_arm.Houndarm if gravity_off else WithGravity
        env = cls(copy.deepcopy(cfg), DEV, DEV, -1, True, False, False)
    assert env._kernels is not None and env.sim.kernel_variant == 4 and env.sim.disable_gravity is gravity_off
    return env


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- the controller
def test_control_kernel_matches_the_float64_restatement(fixture):
    from isaacgymenv_amd import gymtask
    from isaacgymenv_amd._stream import raw_stream
    d = fixture
    L = gymtask.lib()
    n, nl, eef, row = N_WAVES, 7, int(d["eef_index"]), 5
    tile = np.arange(n) % d["ctl_actions"].shape[1]
    p = gymtask.GtArmParams()
    p.num_envs, p.num_links, p.jac_row, p.eef_link, p.effort_stride = n, nl, row, eef, 6
    p.action_scale = 1.0
    for name, vals in (("kp", [A.KP] * 6), ("kd", d["kd"]), ("kp_null", [A.KP_NULL] * 6), ("kd_null", d["kd_null"]),
                       ("cmd_limit", A.CMD_LIMIT), ("dof_default", [0.0] * 6), ("effort_limit", d["effort_limits"])):
        getattr(p, name)[:] = [float(v) for v in vals]
    clamped = unclamped = 0
    worst = 0.0
    for t in range(d["ctl_actions"].shape[0]):
        # the sim's Jacobian tensor [n][links][6][6]; the task's is the view without the welded root's row
        jac_full = torch.zeros((n, nl, 6, 6), device=DEV)
        jac = jac_full[:, 1:]
        jac[:, row] = _g(d["ctl_jac"][t][tile])
        rb = torch.zeros((n, nl, 13), device=DEV)
        rb[:, eef] = _g(d["ctl_eef"][t][tile])
        actions = _g(np.clip(d["ctl_actions"][t][tile], -1.0, 1.0))
        mm, dof = _g(d["ctl_mm"][t][tile]), _g(d["ctl_dof"][t][tile])
        torques = torch.full((n, 6), float("nan"), device=DEV)
        effort = torch.full((n, 6), float("nan"), device=DEV)
        rc = L.gt_arm_control(ctypes.byref(p), actions.data_ptr(), dof.data_ptr(), mm.data_ptr(), jac.data_ptr(),
                              rb.data_ptr(), torques.data_ptr(), effort.data_ptr(), ctypes.c_void_p(raw_stream(DEV)))
        assert rc == 0, L.gt_last_error()
        torch.cuda.synchronize()
        got, ref = torques.cpu().numpy().astype(np.float64), d["torques64"][t][tile]
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= 1e-4).all(), (t, float(err.max()))
        assert torch.equal(torques, effort)
        lim = d["effort_limits"][None]
        clamped += int((np.abs(got) == lim).sum())
        unclamped += int((np.abs(got) < lim).sum())
    assert clamped > 0 and unclamped > 0
    H.parity_report(f"gt_arm_control vs float64 restatement (130 envs x {d['ctl_actions'].shape[0]} recorded steps): "
                    f"worst {worst:.3g} of the 1e-4 max(1, |ref|) bound; {clamped} clamped, {unclamped} unclamped")


# ---------------------------------------------------------------- the tail and the reset
def test_tail_kernel_replays_the_recording(fixture, monkeypatch):
    d = fixture
    A.assert_fixture_conditions(d)
    n = d["obs"].shape[1]
    env = _gpu_env(d, n, monkeypatch)
    assert env.eef_index == int(d["eef_index"]) and env.max_episode_length == int(d["max_episode_length"])
    for t in range(d["obs"].shape[0]):
        env.rigid_body_state[:, env.eef_index] = _g(d["in_eef"][t])
        env.commands.copy_(_g(d["in_commands"][t]))
        env.progress_buf.copy_(_g(d["in_progress"][t]))
        env.reset_buf.copy_(_g(d["in_reset_buf"][t]))
        env._kernels()
        torch.cuda.synchronize()
        np.testing.assert_allclose(env.obs_buf.cpu().numpy(), d["obs"][t], rtol=1e-5, atol=2e-6, err_msg=f"obs {t}")
        np.testing.assert_allclose(env.rew_buf.cpu().numpy(), d["rew"][t], rtol=1e-5, atol=2e-6, err_msg=f"rew {t}")
        np.testing.assert_array_equal(env.reset_buf.cpu().numpy(), d["reset"][t], err_msg=f"reset step {t}")
        np.testing.assert_array_equal(env.progress_buf.cpu().numpy(), d["progress"][t], err_msg=f"progress step {t}")
        assert env._kernels.done_count() == int((d["reset"][t] != 0).sum())


def _random_tail_inputs(env, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n = env.num_envs
    env.rigid_body_state.copy_(torch.randn(env.rigid_body_state.shape, device=DEV, generator=gen) * 0.3)
    env.commands.copy_(torch.rand((n, 3), device=DEV, generator=gen) * 0.6 - 0.3)
    # every fourth env in reach with a slow end-effector; every eighth just outside 0.02
    env.commands[::4] = env.eef_state[::4, :3] + torch.tensor([0.004, -0.003, 0.002], device=DEV)
    env.commands[2::8] = env.eef_state[2::8, :3] + torch.tensor([0.0, 0.0201, 0.0], device=DEV)
    env.rigid_body_state[::4, env.eef_index, 7:] *= 0.03
    env.progress_buf.copy_(torch.randint(0, env.max_episode_length - 1, (n,), device=DEV, generator=gen))


def _flag(env, pattern):
    """Time-outs on the pattern's envs through the tail kernel itself (its ballots are what the reset reads)."""
    n = env.num_envs
    env.reset_buf.zero_()
    env.progress_buf[:] = 3
    ids = {"none": [], "one": [n - 2], "all": list(range(n))}[pattern]
    if ids:
        env.progress_buf[torch.tensor(ids, device=DEV)] = env.max_episode_length - 1
    env._kernels()
    torch.cuda.synchronize()
    return ids


@pytest.fixture
def env130(fixture, monkeypatch):
    return _gpu_env(fixture, N_WAVES, monkeypatch)


@pytest.mark.parametrize("pattern", ["none", "one", "all"])
def test_tail_kernel_matches_torch_tail(env130, pattern):
    from isaacgymenv_amd.isaacgymenvs.tasks.hound_arm import compute_houndarm_reward
    env = env130
    _random_tail_inputs(env, 5)
    env.reset_buf.zero_()
    ids = {"none": [], "one": [N_WAVES - 2], "all": list(range(N_WAVES))}[pattern]
    if ids:
        env.progress_buf[torch.tensor(ids, device=DEV)] = env.max_episode_length - 1
    env.reset_buf[7] = 1  # a flag the tail must keep (reset = time-out ? 1 : reset_buf)
    torch.cuda.synchronize()
    obs = torch.cat((env.eef_state[:, :3], env.eef_state[:, 3:7], env.commands), dim=-1)
    rew, reset = compute_houndarm_reward(env.reset_buf, env.progress_buf, env.eef_state, env.commands,
                                         env.reward_settings["r_dist_scale"], env.reward_settings["r_vel_scale"],
                                         env.max_episode_length)
    dist = torch.norm(env.eef_state[:, :3] - env.commands, dim=-1)
    assert int((dist < 0.02).sum()) >= N_WAVES // 4 and int(((dist >= 0.02) & (dist < 0.021)).sum()) >= N_WAVES // 8 - 1
    env._kernels()
    torch.cuda.synchronize()
    torch.testing.assert_close(env.obs_buf, obs, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(env.rew_buf, rew, rtol=1e-5, atol=2e-6)
    assert env.reset_buf.dtype == torch.int64 and torch.equal(env.reset_buf, reset)
    assert int(reset[7]) == 1 and env._kernels.done_count() == int((reset != 0).sum()) == len(set(ids) | {7})
    assert (rew > 0).any() and (rew >= 0).all()


@pytest.mark.parametrize("pattern", ["none", "one", "all"])
def test_fused_reset_matches_torch_reset_idx(env130, pattern):
    """gt_arm_reset_flagged vs the torch reset_idx from the same state and the same device generator position:
    commands, dof state, controls, counters and the sim's state and forces after the indexed sets are bit-identical,
    and the generator ends where the four torch.rand calls leave it."""
    env = env130
    _random_tail_inputs(env, 9)
    env.effort_control.copy_(torch.randn(env.effort_control.shape, device=DEV))
    env.sim.dof_force.copy_(env.effort_control.reshape(-1))
    ids = _flag(env, pattern)
    k = env._kernels.done_count()
    flagged = env.reset_buf.nonzero(as_tuple=False).flatten()
    assert k == len(ids) and flagged.tolist() == ids
    if k == 0:  # nothing flagged: the count tells the task so, and it launches no reset (post_physics_step)
        return
    names = ("dof_state", "commands", "progress_buf", "reset_buf", "pos_control", "effort_control")
    snap = {a: getattr(env, a).clone() for a in names}
    state0, force0 = env.sim.state.clone(), env.sim.dof_force.clone()
    rng = torch.cuda.get_rng_state()
    env.reset_idx(flagged)
    torch.cuda.synchronize()
    want = {a: getattr(env, a).clone() for a in names}
    want_state, want_force, want_rng = env.sim.state.clone(), env.sim.dof_force.clone(), torch.cuda.get_rng_state()
    for a in names:
        getattr(env, a).copy_(snap[a])
    env.sim.state.copy_(state0)
    env.sim.dof_force.copy_(force0)
    torch.cuda.set_rng_state(rng)
    out = env._kernels.reset_flagged(k)
    torch.cuda.synchronize()
    assert torch.equal(out.long(), flagged)
    for a in names:
        assert torch.equal(getattr(env, a), want[a]), a
    assert torch.equal(env.sim.state, want_state) and torch.equal(env.sim.dof_force, want_force)
    assert torch.equal(torch.cuda.get_rng_state(), want_rng)
    q = env.dof_pos[flagged]
    assert (env.reset_buf[flagged] == 0).all() and (env.progress_buf[flagged] == 0).all()
    assert (env.dof_vel[flagged] == 0).all() and (q.abs() <= 1.57).all()
    assert k == 1 or ((q.abs() == 1.57).any() and (q.abs() < 1.57).any())  # noise 2.0: the clamp engages


# ---------------------------------------------------------------- physics under the switch
def _arm_run(params, root, dof, tau, mu, steps, disable_gravity=True):
    n = root.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gym, sim = A.make_sim("arm", n, params, disable_gravity)
    assert sim.kernel_variant == 4 and sim.disable_gravity is disable_gravity
    H.load_state_into(sim, root, dof, mu)
    sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)).to(sim.state.device))
    for _ in range(steps):
        gym.simulate(sim)
    torch.cuda.synchronize()
    return H.read_state(sim, 6)


@pytest.mark.parametrize("solver,steps", A.PHYSICS_CASES)
def test_arm_without_gravity_matches_the_zero_gravity_oracle(solver, steps):
    """The arm fixture on the runtime-sized kernel, 64 random states inside the joint limits with random efforts: with
    the asset's gravity off the kernel computes what the oracle computes with zero gravity in its own parameters; with
    the flag off it does not."""
    n = 64
    art, flat = A.arm()
    root, dof, tau, mu = A.arm_states(n, seed=A.PHYSICS_SEED)
    params = dict(A.ARM_PARAMS, solver_type=1 if solver == "tgs" else 0)
    oparams = dict(A.ARM_PARAMS, solver_type=3 if solver == "tgs" else 0, gravity=[0.0, 0.0, 0.0])
    g_root, g_dof = _arm_run(params, root, dof, tau, mu, steps)
    o_root, o_dof, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, steps)

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        out = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, steps)
        return H.state_fields(out[0], out[1])
    H.assert_close_or_explained(H.state_fields(g_root, g_dof), H.state_fields(o_root, o_dof), rerun, max_env_frac=0.02,
                                what=f"arm without gravity vs the zero-gravity oracle ({solver}, {steps} simulates)")
    # the flag off: the same states fall, and the result leaves the zero-gravity oracle's by far more than its tolerance
    w_root, w_dof = _arm_run(params, root, dof, tau, mu, steps, disable_gravity=False)
    at, rt = H.STATE_TOL["qd"]
    off = np.abs(w_dof[:, :, 1] - o_dof[:, :, 1]) / (at + rt * np.abs(o_dof[:, :, 1]))
    assert (off.max(axis=1) > 10.0).mean() > 0.9, float(off.max())


def test_arm_at_rest_without_gravity_stays_where_it_is():
    """Known answer: zero effort and zero velocity off the ground under zero gravity.  The bias force of a resting
    articulation is then exactly zero and no contact or limit row exists, so the state does not change at all."""
    n = 64
    root, dof, tau, mu = A.arm_states(n, seed=3, moving=False)
    _, end = _arm_run(A.ARM_PARAMS, root, dof, tau, mu, 20)
    np.testing.assert_array_equal(end, dof.astype(np.float32).astype(np.float64))


def test_cartpole_at_rest_without_gravity_on_the_lane_kernel():
    """The host-backend case of tests/test_houndarm_cpu.py on the one-env-per-lane GPU kernel at 64 envs."""
    n = 64
    root, dof, mu = A.tilted_cartpole(n)
    for disable, moved in ((True, False), (False, True)):
        gym, sim = A.make_sim("cartpole", n, H.CARTPOLE_PARAMS, disable)
        assert sim.kernel_variant == 1
        H.load_state_into(sim, root, dof, mu)
        sim.dof_force.zero_()
        for _ in range(20):
            gym.simulate(sim)
        torch.cuda.synchronize()
        end = H.read_state(sim, 2)[1]
        if moved:
            assert (np.abs(end[:, 1, 0] - dof[:, 1, 0]) > 1e-2).all()
        else:
            np.testing.assert_array_equal(end, dof.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- the task on the real simulator
def test_task_steps_on_the_simulator(fixture, monkeypatch):
    n = 64
    env = _gpu_env(fixture, n, monkeypatch)
    launches = {"control": 0, "tail": 0, "reset": 0}
    K = env._kernels
    control, reset_flagged = K.control, K.reset_flagged

    def counted_control(*a):
        launches["control"] += 1
        return control(*a)

    def counted_reset(k):
        launches["reset"] += 1
        return reset_flagged(k)

    K.control, K.reset_flagged = counted_control, counted_reset
    gen = torch.Generator(device=DEV).manual_seed(1)
    resets = 0
    for _ in range(40):
        obs, rew, reset, extras = env.step(2 * torch.rand((n, 6), device=DEV, generator=gen) - 1)
        assert obs["obs"].shape == (n, 10) and torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all()
        assert (rew >= 0).all() and reset.dtype == torch.int64
        assert torch.isfinite(env.effort_control).all() and float(env.effort_control.abs().max()) <= 1000.0
        assert torch.equal(env.sim.dof_force.view(n, 6), env.effort_control)  # what the sim reads
        resets += int(reset.sum())
    assert resets >= 3 * n and env.sim.kernel_variant == 4
    assert launches["control"] == 40 and launches["reset"] >= 3  # the fused kernels are in use
    assert float(env.effort_control.abs().max()) > 0.1


def _eef_drop(fixture, monkeypatch, gravity_off):
    env = _gpu_env(fixture, 64, monkeypatch, episode_length=1000, gravity_off=gravity_off)
    from isaacgymenv_amd.isaacgym import gymtorch
    env.dof_state.zero_()  # the default pose, at rest
    env.gym.set_dof_state_tensor(env.sim, gymtorch.unwrap_tensor(env.dof_state))
    env.sim.dof_force.zero_()
    env._refresh()
    torch.cuda.synchronize()
    z0 = env.eef_state[:, 2].clone()
    zero = torch.zeros((64, 6), device=DEV)
    for _ in range(30):
        env.step(zero)
    torch.cuda.synchronize()
    return float((env.eef_state[:, 2] - z0).abs().max())


def test_end_effector_holds_its_height_only_without_gravity(fixture, monkeypatch):
    """Zero actions from the default pose: the OSC has no gravity compensation, so under gravity the arm sags."""
    held = _eef_drop(fixture, monkeypatch, True)
    sagged = _eef_drop(fixture, monkeypatch, False)
    H.parity_report(f"Houndarm, zero actions from the default pose, 30 steps: end-effector height change {held:.3g} m "
                    f"with the asset's gravity off, {sagged:.3g} m with the flag forced off")
    assert held < sagged and np.isfinite(held) and np.isfinite(sagged)
