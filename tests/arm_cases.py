"""Houndarm test cases -- TEST INFRASTRUCTURE shared by tests/golden/make_golden_houndarm.py, tests/test_houndarm_cpu.py
and tests/test_houndarm_gpu.py: the fake simulator the task is recorded on, the fixture's settings and the cases it
must hold, a float64 restatement of the operational-space controller, and sims of the arm fixture and of Cartpole
with the asset's gravity switched on or off.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from isaacgymenv_amd.isaacgym import gymapi as _g
from tests.fakegym import FakeGym

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARM_MODEL = "open_manipulator_p.model.json"
N_ENVS, STEPS = 32, 30
EPISODE_LENGTH = 12
DOF_NOISE = 2.0          # 2 * 2 * (r - 0.5) spans +-2: the clamp at the +-1.57 limits engages
IN_REACH_EVERY = 4       # every fourth env: command within reach, slow end-effector
FAKE_SEED = 2026
HEAVY_EVERY, HEAVY = 5, 3.0e4  # every fifth env's mass matrix scaled: its OSC torques clamp at the effort limits
# envs per initial progress value 0..11 (sum 32): no env at 0 and one at 1, so the recording holds a step that
# resets nobody and a step that resets exactly one env; the pattern repeats every EPISODE_LENGTH steps
STAGGER_COUNTS = (0, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4)
# hound_arm.py:161-168
KP, KP_NULL = 150.0, 10.0
CMD_LIMIT = (0.1, 0.1, 0.1, 0.5, 0.5, 0.5)
ARM_OPTS = dict(fix_base_link=True, collapse_fixed_joints=False, replace_cylinder_with_capsule=False,
                disable_gravity=True, thickness=0.001)
# Houndarm.yaml's sim block (dt 1/60, 2 substeps, 8/1 iterations, contact offset 5 mm) in the oracle's terms
ARM_PARAMS = dict(dt=0.01667, substeps=2, gravity=[0.0, 0.0, -9.81], pos_iters=8, vel_iters=1, contact_offset=0.005,
                  rest_offset=0.0, max_depen_vel=1000.0, collect_contacts=0, has_ground=1, ground_friction=1.0,
                  limit_margin=0.1)
# the random arm states of the GPU physics comparison: the oracle's own float32 run stays inside the comparison's cap
# for this seed (tests/test_houndarm_cpu.py checks it)
PHYSICS_SEED = 5
PHYSICS_CASES = (("tgs", 1), ("pgs", 20))  # (solver, simulates)


class ArmFakeGym(FakeGym):
    """FakeGym with a rigid-body tensor that changes with every refresh: each link keeps a seeded position that
    jitters by a millimetre, its velocity is redrawn (not from the torch RNG), and every fourth env's is slow, so the
    reward's velocity term is positive there."""

    def _rigid_body(self, sim):
        n, nb = sim.N, sim.nb
        base = np.random.RandomState(self.seed + 17).normal(0.0, 0.25, (n, nb, 3))
        rng = np.random.RandomState(self.seed + 3000 + sim.t)
        rb = np.zeros((n, nb, 13))
        rb[..., 0:3] = base + rng.normal(0.0, 1e-3, (n, nb, 3))
        q = rng.normal(0.0, 1.0, (n, nb, 4))
        rb[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        rb[..., 7:13] = rng.normal(0.0, 0.3, (n, nb, 6))
        rb[::IN_REACH_EVERY, :, 7:13] *= 0.03
        return torch.from_numpy(rb.reshape(n * nb, 13).astype(np.float32))

    def acquire_rigid_body_state_tensor(self, sim):
        self._sizes(sim)
        if sim.rb_t is None:
            sim.rb_t = self._rigid_body(sim)
        return _g.GymTensor(sim.rb_t, "rigid_body")

    def refresh_rigid_body_state_tensor(self, sim):
        sim.rb_t.copy_(self._rigid_body(sim))

    # The base fake's Jacobian rows are normal(0, 0.3) matrices whose condition number reaches 1e4: the controller
    # inverts J M^-1 J^T in float32, and two LAPACK builds then differ by more than the torque tolerance.  Here every
    # row is a perturbed identity (condition number below 3), so the recorded float32 torques sit well inside the
    # tolerance of their float64 restatement (assert_fixture_conditions); every fifth env's arm is HEAVY times heavier,
    # which scales its torques past the effort limits without changing the conditioning.
    def refresh_jacobian_tensors(self, sim):
        rng = np.random.RandomState(self.seed + 1000 + sim.t)
        j = np.eye(6)[None, None] + rng.normal(0.0, 0.15, tuple(sim.jac_t.shape))
        sim.jac_t.copy_(torch.from_numpy(j.astype(np.float32)))

    def refresh_mass_matrix_tensors(self, sim):
        super().refresh_mass_matrix_tensors(sim)
        sim.mm_t[1::HEAVY_EVERY] *= HEAVY


def fixture_cfg(num_envs: int = N_ENVS) -> dict:
    """Houndarm.yaml on the CPU pipeline with the fixture's settings; env.asset names the packed arm model relative
    to tests/golden (point_at_fixture makes the root absolute for the run)."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    cfg = compose("config", ["task=Houndarm", f"num_envs={num_envs}", "sim_device=cpu", "pipeline=cpu"])["task"]
    cfg["env"]["episodeLength"] = EPISODE_LENGTH
    cfg["env"]["houndarmDofNoise"] = DOF_NOISE
    cfg["env"]["asset"] = {"assetRoot": "", "assetFileNamehoundarm": ARM_MODEL}
    return cfg


def point_at_fixture(cfg: dict) -> dict:
    cfg["env"]["asset"] = {"assetRoot": GOLDEN, "assetFileNamehoundarm": ARM_MODEL}
    return cfg


def stagger(env):
    """Once after construction: spread progress_buf so the time-outs do not all fall on one step."""
    n = env.num_envs
    values = np.repeat(np.arange(EPISODE_LENGTH), STAGGER_COUNTS)
    values = np.resize(values, n)[np.random.RandomState(11).permutation(n)]
    env.progress_buf[:] = torch.from_numpy(values).to(env.progress_buf.device)


def place_commands(env, eef_name="eef_state"):
    """Before each step: every fourth env's command within 0.02 of its end-effector."""
    eef = getattr(env, eef_name)
    offset = torch.tensor([0.004, -0.003, 0.002], device=eef.device)
    env.commands[::IN_REACH_EVERY] = eef[::IN_REACH_EVERY, :3] + offset


def assert_fixture_conditions(d):
    """The cases a Houndarm recording must hold (the generator asserts them, the tests re-check them)."""
    k = d["reset_count_in"]
    eef, cmd = d["in_eef"], d["in_commands"]
    dist = np.linalg.norm(eef[..., :3] - cmd, axis=-1)
    vel_term = 1.0 - np.tanh(10.0 * np.linalg.norm(eef[..., 7:], axis=-1))
    reset_q = np.concatenate([d["dof_state"][t][d["in_reset"][t] != 0, :, 0].reshape(-1) for t in range(len(k))])
    limit = float(d["dof_upper"].max())
    tq, lim = np.abs(d["torques"]), d["effort_limits"][None, None, :]
    cases = {"time-out resets": int((d["time_outs"] != 0).sum()), "steps without a reset": int((k == 0).sum()),
             "steps resetting exactly one env": int((k == 1).sum()),
             "in-reach envs with a positive velocity term": int(((dist < 0.02) & (vel_term > 1e-3)).sum()),
             "out-of-reach envs": int((dist >= 0.02).sum()),
             "clamped reset positions": int((np.abs(reset_q) == np.float32(limit)).sum()),
             "unclamped reset positions": int((np.abs(reset_q) < np.float32(limit)).sum()),
             "clamped OSC torques": int((tq == lim).sum()), "unclamped OSC torques": int((tq < lim).sum())}
    for what, count in cases.items():
        assert count > 0, f"fixture lacks: {what}"
    # the reference's float32 torques lie within half the torque tolerance (rtol 1e-4, atol 1e-4) of their float64
    # restatement: the inputs are conditioned well enough for another machine's float32 inverse to land inside it
    slack = np.abs(d["torques"] - d["torques64"]) / (1e-4 + 1e-4 * np.abs(d["torques64"]))
    assert slack.max() <= 0.5, f"float32 torques use {slack.max():.3g} of the tolerance against float64"
    cases["float32 torque error / tolerance"] = float(slack.max())
    return cases


def osc_float64(actions, jac, mm, eef, dof, effort_limits, action_scale=1.0, default=None):
    """hound_arm.py:462-523 restated in float64 on float32 inputs: actions [n, 6], jac / mm [n, 6, 6], eef [n, 13],
    dof [n, 6, 2] -> clamped torques [n, 6] (float64).  dpose is the reference's float32 product."""
    f = np.float64
    dpose = (np.asarray(actions, np.float32) * np.asarray(CMD_LIMIT, np.float32) / np.float32(action_scale)).astype(f)
    J, M, eef, dof = (np.asarray(a, f) for a in (jac, mm, eef, dof))
    kp, kpn = np.float32(KP), np.float32(KP_NULL)
    kd, kdn = f(np.float32(2) * np.sqrt(kp)), f(np.float32(2) * np.sqrt(kpn))  # float32 gains, as torch holds them
    kp, kpn = f(kp), f(kpn)
    default = np.zeros(6) if default is None else np.asarray(default, f)
    Jt = np.transpose(J, (0, 2, 1))
    Minv = np.linalg.inv(M)
    Meef = np.linalg.inv(J @ Minv @ Jt)
    u = Jt @ Meef @ (kp * dpose - kd * eef[:, 7:])[..., None]
    q, qd = dof[:, :, 0], dof[:, :, 1]
    u_null = kdn * -qd + kpn * (np.mod(default - q + np.pi, 2 * np.pi) - np.pi)
    u_null = M @ u_null[..., None]
    u = u + (np.eye(6)[None] - Jt @ (Meef @ J @ Minv)) @ u_null
    lim = np.asarray(effort_limits, f)[None]
    return np.clip(u[..., 0], -lim, lim)


# ---------------------------------------------------------------- physics under the gravity switch
def arm():
    """(articulation, flat model) of the packed arm fixture with Houndarm's asset options."""
    import json
    from isaacgymenv_amd.isaacgym._assets import RawModel, build_articulation
    from isaacgymenv_amd.isaacgym._model import flatten
    with open(os.path.join(GOLDEN, ARM_MODEL)) as f:
        art = build_articulation(RawModel.from_json(json.load(f)), ARM_OPTS)
    flat = flatten(art)
    flat["self_collide"] = 0  # (fixed base: its pairs are dropped)
    return art, flat


def arm_states(n, seed=0, moving=True):
    """Random arm states in the oracle's layout: the welded root at (0, 0, height) with the arm clear of the ground,
    joints inside their +-1.57 limits (away from the limit margin), random velocities and efforts."""
    rng = np.random.RandomState(seed)
    art, flat = arm()
    root = np.zeros((n, 13))
    root[:, 2] = 1.0
    root[:, 6] = 1.0
    dof = np.zeros((n, 6, 2))
    dof[:, :, 0] = rng.uniform(-1.2, 1.2, (n, 6))
    tau = np.zeros((n, 6))
    if moving:
        dof[:, :, 1] = rng.normal(0.0, 0.5, (n, 6))
        tau = rng.uniform(-2.0, 2.0, (n, 6))
    mu = np.ones((n, max(1, flat["ns"])))
    return root, dof, tau, mu


def make_sim(kind, n, params, disable_gravity, host=False, height=None):
    """A libgymsim sim of the arm fixture ("arm", collision filter 0 as the task creates it) or of Cartpole
    ("cartpole", filter 1) through the drop-in gymapi, with AssetOptions.disable_gravity as given."""
    gym = _g.acquire_gym()
    sp = _g.SimParams()
    sp.dt, sp.substeps, sp.up_axis = params["dt"], params["substeps"], _g.UP_AXIS_Z
    sp.gravity = _g.Vec3(*params["gravity"])
    sp.use_gpu_pipeline = not host
    sp.physx.use_gpu = not host
    sp.physx.num_threads = 2
    sp.physx.num_position_iterations = params["pos_iters"]
    sp.physx.num_velocity_iterations = params["vel_iters"]
    sp.physx.contact_offset = params["contact_offset"]
    sp.physx.rest_offset = params["rest_offset"]
    sp.physx.max_depenetration_velocity = params["max_depen_vel"]
    sp.physx.contact_collection = _g.ContactCollection(params["collect_contacts"])
    sp.physx.solver_type = int(params.get("solver_type", 0))
    sim = gym.create_sim(0, -1, _g.SIM_PHYSX, sp)
    plane = _g.PlaneParams()
    plane.static_friction = params.get("ground_friction", 1.0)
    gym.add_ground(sim, plane)
    opts = _g.AssetOptions()
    opts.fix_base_link = True
    opts.disable_gravity = disable_gravity
    opts.default_dof_drive_mode = _g.DOF_MODE_EFFORT
    if kind == "arm":
        opts.collapse_fixed_joints, opts.replace_cylinder_with_capsule, opts.thickness = False, False, 0.001
        asset = gym.load_asset(sim, GOLDEN, ARM_MODEL, opts)
    else:
        asset = gym.load_asset(sim, "/nonexistent", "urdf/cartpole.urdf", opts)
    for i in range(n):
        env = gym.create_env(sim, _g.Vec3(-1, -1, 0), _g.Vec3(1, 1, 1), 8)
        pose = _g.Transform()
        pose.p = _g.Vec3(0, 0, (1.0 if kind == "arm" else 2.0) if height is None else height)
        handle = gym.create_actor(env, asset, pose, kind, i, 0 if kind == "arm" else 1, 0)
        props = gym.get_actor_dof_properties(env, handle)
        props["driveMode"][:] = _g.DOF_MODE_EFFORT
        props["stiffness"][:] = 0.0
        props["damping"][:] = 0.0
        gym.set_actor_dof_properties(env, handle, props)
    gym.prepare_sim(sim)
    return gym, sim


def tilted_cartpole(n):
    """Cartpole at rest with the pole tilted by 0.3 rad: (root, dof, mu) in the oracle's layout."""
    root = np.zeros((n, 13))
    root[:, 2], root[:, 6] = 2.0, 1.0
    dof = np.zeros((n, 2, 2))
    dof[:, 1, 0] = 0.3
    return root, dof, np.ones((n, 1))
