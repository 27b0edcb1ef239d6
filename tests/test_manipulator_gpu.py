"""Manipulator on the GPU: the lane-team controller gt_osc_control, the tail and the 7-dof reset, the packed Franka on
the runtime-sized kernel, and the task on the real simulator.

* gt_osc_control at nd = 7 on the recorded control inputs (tests/golden/manipulator.npz) tiled to 19 envs (two full
  8-env waves and a ragged one) and to 130, against the fixture's float64 restatement:
  |got - ref| <= 1e-4 max(1, |ref|), the project's rule for the OSC kernels, four orders above what two float64
  algorithms differ by on these inputs (tests/test_manipulator_cpu.py); the effort tensor bit-equal to the torques;
* at nd = 6, on Houndarm's recorded inputs, the bits gt_arm_control returns;
* a posture error changes the kernel's torques and leaves J M^-1 u where it was: the term lands in the null space;
* gt_arm_post_physics replaying the recording with the done count exact; gt_manip_reset_flagged against the task's
  torch reset_idx from the same generator position, bit for bit;
* the packed Franka under AssetOptions.disable_gravity against the zero-gravity oracle;
* the task through isaacgymenvs.make: fused against torch path, finite observations, the end-effector's height, and
  two PPO epochs.
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
from tests import manip_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WAVES = 130  # two full 64-lane waves and a partial one; sixteen 8-env controller waves and a ragged one
SIZES = (19, 130)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(M.GOLDEN, "manipulator.npz"))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(d, n, nd, nl, row, eef, default, effort=None):
    from isaacgymenv_amd import gymtask
    effort = d["effort_limits"] if effort is None else effort
    return gymtask.manip_params(nd, n, nl, row, eef, nd, 1.0, [M.KP] * 6, d["kd"], M.CMD_LIMIT, [M.KP_NULL] * nd,
                                d["kd_null"], default, effort, d["dof_lower"], d["dof_upper"])


def _control_inputs(d, t, tile, nd, nl, row, eef):
    """The recorded control inputs of step t in the sim's layouts: the Jacobian tensor [n][links][6][nd], of which the
    task sees the view without the welded root's row."""
    n = len(tile)
    jac_full = torch.zeros((n, nl, 6, nd), device=DEV)
    jac = jac_full[:, 1:]
    jac[:, row] = _g(d["ctl_jac"][t][tile])
    rb = torch.zeros((n, nl, 13), device=DEV)
    rb[:, eef] = _g(d["ctl_eef"][t][tile])
    actions = _g(np.clip(d["ctl_actions"][t][tile], -1.0, 1.0))
    return actions, _g(d["ctl_dof"][t][tile]), _g(d["ctl_mm"][t][tile]), jac, rb, jac_full


def _osc(p, actions, dof, mm, jac, rb):
    """One gt_osc_control launch -> (torques, effort), NaN-filled before."""
    from isaacgymenv_amd import gymtask
    from isaacgymenv_amd._stream import raw_stream
    L = gymtask.lib()
    torques = torch.full((p.num_envs, p.nd), float("nan"), device=DEV)
    effort = torch.full((p.num_envs, p.effort_stride), float("nan"), device=DEV)
    rc = L.gt_osc_control(ctypes.byref(p), actions.data_ptr(), dof.data_ptr(), mm.data_ptr(), jac.data_ptr(),
                          rb.data_ptr(), torques.data_ptr(), effort.data_ptr(), ctypes.c_void_p(raw_stream(DEV)))
    assert rc == 0, L.gt_last_error()
    torch.cuda.synchronize()
    return torques, effort


# ---------------------------------------------------------------- the controller
@pytest.mark.parametrize("n", SIZES)
def test_osc_kernel_matches_the_float64_restatement(fixture, n):
    d = fixture
    nl, eef, row = 8, int(d["eef_index"]), 6
    tile = np.arange(n) % d["ctl_actions"].shape[1]
    p = _params(d, n, 7, nl, row, eef, M.DEFAULT_POSE)
    lim = d["effort_limits"][None]
    clamped = unclamped = 0
    worst = 0.0
    for t in range(d["ctl_actions"].shape[0]):
        actions, dof, mm, jac, rb, _ = _control_inputs(d, t, tile, 7, nl, row, eef)
        torques, effort = _osc(p, actions, dof, mm, jac, rb)
        got, ref = torques.cpu().numpy().astype(np.float64), d["torques64"][t][tile]
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= M.TORQUE_BOUND).all(), (t, float(err.max()))
        assert torch.equal(torques, effort)
        clamped += int((np.abs(got) == lim).sum())
        unclamped += int((np.abs(got) < lim).sum())
        assert (np.abs(got) <= lim).all()
    assert clamped > 0 and unclamped > 0
    H.parity_report(f"gt_osc_control nd=7 vs float64 restatement ({n} envs x {d['ctl_actions'].shape[0]} recorded "
                    f"steps): worst {worst:.3g} of the 1e-4 max(1, |ref|) bound; {clamped} clamped, {unclamped} "
                    f"unclamped")


@pytest.mark.parametrize("n", SIZES)
def test_osc_kernel_at_six_dofs_returns_the_serial_kernels_bits(n):
    """Houndarm's recorded inputs through gt_arm_control (one env per lane, csrc/gt_osc6.h) and through gt_osc_control
    at nd = 6: the same operations in the same order, so the same bits."""
    from isaacgymenv_amd import gymtask
    from isaacgymenv_amd._stream import raw_stream
    d = np.load(os.path.join(A.GOLDEN, "houndarm.npz"))
    L = gymtask.lib()
    nl, eef, row = 7, int(d["eef_index"]), 5
    tile = np.arange(n) % d["ctl_actions"].shape[1]
    pa = gymtask.GtArmParams()
    pa.num_envs, pa.num_links, pa.jac_row, pa.eef_link, pa.effort_stride = n, nl, row, eef, 6
    pa.action_scale = 1.0
    for name, vals in (("kp", [A.KP] * 6), ("kd", d["kd"]), ("kp_null", [A.KP_NULL] * 6), ("kd_null", d["kd_null"]),
                       ("cmd_limit", A.CMD_LIMIT), ("dof_default", [0.0] * 6), ("effort_limit", d["effort_limits"])):
        getattr(pa, name)[:] = [float(v) for v in vals]
    for limits in (d["effort_limits"], np.full(6, 3.0e38, np.float32)):  # as recorded, and with nothing clamped
        pa.effort_limit[:] = [float(v) for v in limits]
        p = _params(d, n, 6, nl, row, eef, [0.0] * 6, effort=limits)
        differing = 0
        for t in range(d["ctl_actions"].shape[0]):
            actions, dof, mm, jac, rb, _ = _control_inputs(d, t, tile, 6, nl, row, eef)
            want_t = torch.full((n, 6), float("nan"), device=DEV)
            want_e = torch.full((n, 6), float("nan"), device=DEV)
            rc = L.gt_arm_control(ctypes.byref(pa), actions.data_ptr(), dof.data_ptr(), mm.data_ptr(), jac.data_ptr(),
                                  rb.data_ptr(), want_t.data_ptr(), want_e.data_ptr(), ctypes.c_void_p(raw_stream(DEV)))
            assert rc == 0, L.gt_last_error()
            torques, effort = _osc(p, actions, dof, mm, jac, rb)
            assert torch.isfinite(want_t).all()
            differing += int((torques != want_t).sum())
            assert torch.equal(torques, want_t) and torch.equal(effort, want_e), (t, differing)


def test_posture_term_lands_in_the_null_space(fixture):
    """Nothing clamped (limits of 3e38).  A posture error of 0.3 rad on every joint changes the torques by far more
    than the bound, and J M^-1 u -- the task-space acceleration the torques produce, in float64 from the float32
    outputs -- stays within 1e-4 max(1, |ref|) of the float64 restatement's, with and without the error."""
    d = fixture
    n, nl, eef, row = N_WAVES, 8, int(d["eef_index"]), 6
    tile = np.arange(n) % d["ctl_actions"].shape[1]
    big = np.full(7, 3.0e38, np.float32)
    shifted = np.asarray(M.DEFAULT_POSE) + 0.3
    p0 = _params(d, n, 7, nl, row, eef, M.DEFAULT_POSE, effort=big)
    p1 = _params(d, n, 7, nl, row, eef, shifted, effort=big)
    worst, moved = 0.0, 0.0
    for t in (0, 7, 19):
        actions, dof, mm, jac, rb, _ = _control_inputs(d, t, tile, 7, nl, row, eef)
        u0 = _osc(p0, actions, dof, mm, jac, rb)[0].cpu().numpy().astype(np.float64)
        u1 = _osc(p1, actions, dof, mm, jac, rb)[0].cpu().numpy().astype(np.float64)
        J, Mm = d["ctl_jac"][t][tile].astype(np.float64), d["ctl_mm"][t][tile].astype(np.float64)
        JMi = J @ np.linalg.inv(Mm)
        acc = lambda u: (JMi @ u[..., None])[..., 0]  # noqa: E731
        ref = acc(M.restatement(d, t, parts=True)[1][tile])
        moved = max(moved, float(np.abs(u1 - u0).max()))
        # the term is not dropped: every env's torques change by at least ten times what the bound could hide (the
        # float64 restatement moves them by 120 bounds or more on these steps), half of the envs' by over 1 N m
        change = np.abs(u1 - u0)
        assert ((change / (M.TORQUE_BOUND * np.maximum(1.0, np.abs(u0)))).max(axis=1) > 10.0).all()
        assert np.median(change.max(axis=1)) > 1.0
        for a in (acc(u0), acc(u1)):
            err = np.abs(a - ref) / np.maximum(1.0, np.abs(ref))
            worst = max(worst, float(err.max()))
            assert (err <= M.TORQUE_BOUND).all(), (t, float(err.max()))
    H.parity_report(f"gt_osc_control nd=7, posture error 0.3 rad: torques move by up to {moved:.3g} N m, J M^-1 u "
                    f"stays within {worst:.3g} of the 1e-4 max(1, |ref|) bound")


# ---------------------------------------------------------------- the tail and the reset
def _gpu_env(fixture, n, monkeypatch, episode_length=M.EPISODE_LENGTH, gravity_off=True, dof_noise=M.DOF_NOISE):
    """Manipulator on the real simulator from the fixture's config (GPU pipeline)."""
    from isaacgymenv_amd.isaacgym import gymapi
    from isaacgymenv_amd.isaacgymenvs.tasks import manipulator
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    cfg = M.point_at_fixture(yaml.safe_load(str(fixture["cfg_yaml"])))
    cfg["env"]["numEnvs"] = n
    cfg["env"]["episodeLength"] = episode_length
    cfg["env"]["frankaDofNoise"] = dof_noise
    cfg["sim"]["use_gpu_pipeline"] = True
    cfg["sim"]["physx"]["use_gpu"] = True
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)

    class WithGravity(manipulator.Manipulator):  # the flag forced off
        def _asset_options(self):
            opts = super()._asset_options()
            opts.disable_gravity = False
            return opts

    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        cls = manipulator.Manipulator if gravity_off else WithGravity
        env = cls(copy.deepcopy(cfg), DEV, DEV, -1, True, False, False)
    assert env._kernels is not None and env.sim.kernel_variant == 4 and env.sim.disable_gravity is gravity_off
    assert type(env._kernels).__name__ == "ManipulatorKernels" and env.num_dofs == 7
    return env


def test_tail_kernel_replays_the_recording(fixture, monkeypatch):
    d = fixture
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


PATTERNS = {"none": lambda n: [], "one": lambda n: [n - 2], "every-third": lambda n: list(range(1, n, 3)),
            "all": lambda n: list(range(n))}


@pytest.fixture(scope="module")
def env130(fixture):
    mp = pytest.MonkeyPatch()
    yield _gpu_env(fixture, N_WAVES, mp)
    mp.undo()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_fused_reset_matches_torch_reset_idx(env130, pattern):
    """gt_manip_reset_flagged vs the torch reset_idx from the same state and the same device generator position:
    commands, dof state, controls, counters and the sim's state and forces after the indexed sets are bit-identical,
    and the generator ends where the four torch.rand calls leave it."""
    env = env130
    n = env.num_envs
    gen = torch.Generator(device=DEV).manual_seed(9)
    env.rigid_body_state.copy_(torch.randn(env.rigid_body_state.shape, device=DEV, generator=gen) * 0.3)
    env.commands.copy_(torch.rand((n, 3), device=DEV, generator=gen) - 0.5)
    env.effort_control.copy_(torch.randn(env.effort_control.shape, device=DEV, generator=gen))
    env.sim.dof_force.copy_(env.effort_control.reshape(-1))
    ids = PATTERNS[pattern](n)
    env.reset_buf.zero_()
    env.progress_buf[:] = 3
    if ids:
        env.progress_buf[torch.tensor(ids, device=DEV)] = env.max_episode_length - 1
    env._kernels()  # the tail's ballots are what the reset reads
    torch.cuda.synchronize()
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
    assert (env.dof_vel[flagged] == 0).all()
    assert (q >= env.dof_lower_limits).all() and (q <= env.dof_upper_limits).all()
    assert torch.equal(q[:, -2:], env.default_dof_pos[-2:].expand(k, 2))  # the last two joints: defaults exactly
    if k > 1:  # noise 3.0: the clamp engages on both bounds of panda_joint2, and not everywhere
        assert (q[:, 1] == env.dof_upper_limits[1]).any() and (q[:, 1] == env.dof_lower_limits[1]).any()
        assert ((q[:, 1] > env.dof_lower_limits[1]) & (q[:, 1] < env.dof_upper_limits[1])).any()


# ---------------------------------------------------------------- physics
def _franka_run(params, root, dof, tau, mu, steps, disable_gravity=True):
    n = root.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gym, sim = M.make_sim(n, params, disable_gravity)
    assert sim.kernel_variant == 4 and sim.disable_gravity is disable_gravity
    H.load_state_into(sim, root, dof, mu)
    sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)).to(sim.state.device))
    for _ in range(steps):
        gym.simulate(sim)
    torch.cuda.synchronize()
    return H.read_state(sim, 7)


@pytest.mark.parametrize("solver,steps", M.PHYSICS_CASES)
def test_franka_without_gravity_matches_the_zero_gravity_oracle(solver, steps):
    """The packed Franka (masses from its hulls) on the runtime-sized kernel, 64 random states inside the joint limits
    with random efforts, against the oracle with zero gravity in its own parameters; with the flag off it does not
    match."""
    n = 64
    art, flat = M.franka()
    root, dof, tau, mu = M.franka_states(n, seed=M.PHYSICS_SEED)
    params = dict(M.MANIP_PARAMS, solver_type=1 if solver == "tgs" else 0)
    oparams = dict(M.MANIP_PARAMS, solver_type=3 if solver == "tgs" else 0, gravity=[0.0, 0.0, 0.0])
    g_root, g_dof = _franka_run(params, root, dof, tau, mu, steps)
    o_root, o_dof, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, steps)

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        out = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, steps)
        return H.state_fields(out[0], out[1])
    H.assert_close_or_explained(H.state_fields(g_root, g_dof), H.state_fields(o_root, o_dof), rerun, max_env_frac=0.02,
                                what=f"Franka without gravity vs the zero-gravity oracle ({solver}, {steps} simulates)")
    w_root, w_dof = _franka_run(params, root, dof, tau, mu, steps, disable_gravity=False)
    at, rt = H.STATE_TOL["qd"]
    off = np.abs(w_dof[:, :, 1] - o_dof[:, :, 1]) / (at + rt * np.abs(o_dof[:, :, 1]))
    assert (off.max(axis=1) > 10.0).mean() > 0.9, float(off.max())


def test_franka_at_rest_without_gravity_stays_where_it_is():
    """Known answer: zero effort and zero velocity off the ground under zero gravity.  The bias force of a resting
    articulation is then exactly zero and no contact or limit row exists, so the state does not change at all."""
    n = 64
    root, dof, tau, mu = M.franka_states(n, seed=3, moving=False)
    _, end = _franka_run(M.MANIP_PARAMS, root, dof, tau, mu, 20)
    np.testing.assert_array_equal(end, dof.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------- the task through make()
N_TASK, TASK_STEPS = 64, 40


def _make(monkeypatch, n=N_TASK, seed=42):
    from isaacgymenv_amd.isaacgym import gymapi
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    torch.manual_seed(seed)  # (the device generator the initial reset draws from)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        env = isaacgymenvs.make(seed=seed, task="Manipulator", num_envs=n, sim_device=DEV, rl_device=DEV,
                                headless=True, force_render=False,
                                overrides=[f"task.env.asset.assetRoot={M.GOLDEN}",
                                           f"task.env.asset.assetFileNameFranka={M.MANIP_MODEL}"])
    assert env.sim.kernel_variant == 4 and env.sim.disable_gravity is True and env.max_episode_length == 1000
    assert type(env._kernels).__name__ == "ManipulatorKernels"
    return env


def _rollout(env, acts, fused, start_noise=None):
    """TASK_STEPS steps -> the compared fields as numpy [n, ...]; start_noise (q, qd) [n, 7] is added to the dof state
    first."""
    from isaacgymenv_amd.isaacgym import gymtorch
    if not fused:
        env._kernels = None
    if start_noise is not None:
        env.dof_pos.add_(start_noise[0])
        env.dof_vel.add_(start_noise[1])
        env.gym.set_dof_state_tensor(env.sim, gymtorch.unwrap_tensor(env.dof_state))
        env._refresh()
    peak = 0.0
    start = env.dof_state.clone()
    for a in acts:
        obs, rew, reset, extras = env.step(a)
        assert torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all() and (rew >= 0).all()
        assert obs["obs"].shape == (env.num_envs, 10) and not reset.any()
        assert torch.equal(env.sim.dof_force.view(env.num_envs, 7), env.effort_control)  # what the sim reads
        assert (env.effort_control.abs() <= env.effort_limits).all()
        peak = max(peak, float(env.effort_control.abs().max()))
    torch.cuda.synchronize()
    assert peak > 1.0
    f = lambda x: x.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    return {"q": f(env.dof_pos), "qd": f(env.dof_vel), "pose": f(env.eef_state[:, :7]),
            "vel": f(env.eef_state[:, 7:])}, start


def test_fused_and_torch_paths_agree_on_the_simulator(monkeypatch):
    """make(task="Manipulator") at 64 envs, 40 random-action steps from the same seed, once on the fused kernels and
    once on the torch statements (env._kernels = None).  The two controllers differ in precision (float64 against
    torch's float32 LU inverses), so the closed loop separates the runs a little more every step.  The compared state
    after 40 steps -- joint positions and velocities, end-effector pose and velocity, at the per-simulate tolerances of
    tests/helpers.STATE_TOL -- must be within tolerance, or explained env by env by the torch path's own sensitivity:
    the same torch run from a start perturbed at float32-rounding size moves the env at least half as far
    (assert_close_or_explained, 8 reruns of all 64 envs).  No cap on how many envs need the explanation: the cap of the
    physics tests is for one simulate against a float64 oracle, this is 40 closed-loop steps against float32.
    Both runs start from the same draws (the initial reset's), bit for bit."""
    gen = torch.Generator(device=DEV).manual_seed(1)
    acts = [2 * torch.rand((N_TASK, 6), device=DEV, generator=gen) - 1 for _ in range(TASK_STEPS)]
    fused, start_f = _rollout(_make(monkeypatch), acts, True)
    torch_, start_t = _rollout(_make(monkeypatch), acts, False)
    assert torch.equal(start_f, start_t) and float(start_f.abs().max()) > 1.0

    def rerun(idx, rng):
        noise = (torch.from_numpy(rng.normal(0, 1e-6, (N_TASK, 7)).astype(np.float32)).to(DEV),
                 torch.from_numpy(rng.normal(0, 1e-5, (N_TASK, 7)).astype(np.float32)).to(DEV))
        out, _ = _rollout(_make(monkeypatch), acts, False, start_noise=noise)
        return {k: v[idx] for k, v in out.items()}
    H.assert_close_or_explained(fused, torch_, rerun, max_env_frac=1.0, tries=8,
                                what=f"Manipulator fused vs torch path, {TASK_STEPS} steps at {N_TASK} envs")
    assert np.abs(fused["qd"]).max() > 0.05  # the arms move


def _eef_drop(monkeypatch, gravity_off, fixture):
    env = _gpu_env(fixture, 64, monkeypatch, episode_length=1000, gravity_off=gravity_off)
    from isaacgymenv_amd.isaacgym import gymtorch
    env.dof_pos[:] = env.default_dof_pos  # the default pose, at rest: no posture error, no task error
    env.dof_vel.zero_()
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
    held = _eef_drop(monkeypatch, True, fixture)
    sagged = _eef_drop(monkeypatch, False, fixture)
    H.parity_report(f"Manipulator, zero actions from the default pose, 30 steps: end-effector height change "
                    f"{held:.3g} m with the asset's gravity off, {sagged:.3g} m with the flag forced off")
    assert np.isfinite(held) and np.isfinite(sagged) and held < 1e-3 < sagged


def test_task_resets_through_the_fused_kernels(fixture, monkeypatch):
    """12-step episodes at 64 envs: 40 steps reset every env three times through gt_manip_reset_flagged."""
    n = 64
    env = _gpu_env(fixture, n, monkeypatch, dof_noise=0.25)
    launches = {"control": 0, "reset": 0}
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
        assert torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all() and reset.dtype == torch.int64
        resets += int(reset.sum())
    assert resets >= 3 * n and launches["control"] == 40 and launches["reset"] >= 3


def test_ppo_epochs_run_with_finite_losses(monkeypatch):
    """Two PPO epochs of the in-repo learner on 64 envs with ManipulatorPPO.yaml (the minibatch cut to the 64 x 32
    batch): finite losses and parameters."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    cfg = compose("config", ["task=Manipulator"])
    assert cfg["train"]["params"]["config"]["name"] == "Manipulator"
    env = _make(monkeypatch)
    agent = A2CAgent(env, PpoConfig.from_train_cfg(cfg["train"], minibatch_size=1024), device=DEV, seed=42)
    for _ in range(2):
        agent.train_epoch()
    s = agent.epoch_stats()
    assert np.isfinite(s["kl"]) and np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"])
    assert all(torch.isfinite(p).all() for p in agent.params)
    assert agent.frame == 2 * 32 * N_TASK
