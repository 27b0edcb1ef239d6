"""Manipulator test cases -- TEST INFRASTRUCTURE shared by tests/golden/make_golden_manipulator.py,
tests/test_manipulator_cpu.py and tests/test_manipulator_gpu.py: the fake simulator the task is recorded on, the
fixture's settings and the cases it must hold, a float64 restatement of the 7-dof operational-space controller in two
algorithms (LAPACK and Gauss-Jordan inverses), and the packed Franka for the physics comparisons.  Builds on
tests/arm_cases.py (Houndarm's).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from isaacgymenv_amd.isaacgym import gymapi as _g
from tests import arm_cases as A

GOLDEN = A.GOLDEN
MANIP_MODEL = "franka_panda_manipulator.model.json"
ND = 7
N_ENVS, STEPS, EPISODE_LENGTH, FAKE_SEED = A.N_ENVS, A.STEPS, A.EPISODE_LENGTH, A.FAKE_SEED
# frankaDofNoise (0.25 in the task's config): 2 * 3 * (r - 0.5) spans +-3, so the reset's clamp engages on both bounds
# of panda_joint2 (0.1963 in +-1.7628) and panda_joint4 (-2.618 in [-3.0718, -0.0698])
DOF_NOISE = 3.0
# manipulator.py:153-167
DEFAULT_POSE = (0.0, 0.1963, 0.0, -2.6180, 0.0, 2.9416, 0.7854)
KP, KP_NULL, CMD_LIMIT = A.KP, A.KP_NULL, A.CMD_LIMIT
EFFORT = (87.0, 87.0, 87.0, 87.0, 12.0, 12.0, 12.0)
# every fifth env's mass matrix scaled: more of its torques clamp at the 87 N m limits.  The scale leaves the
# conditioning alone, but the null-space projection cancels M u_null down to a small remainder, so a larger scale
# costs float32 digits: at 3 the reference's float32 torques stay within 0.3 of the CPU tolerance of their float64
# restatement, at 10 they leave it
HEAVY_EVERY, HEAVY = 5, 3.0
MANIP_OPTS = dict(fix_base_link=True, collapse_fixed_joints=False, disable_gravity=True, thickness=0.001,
                  flip_visual_attachments=True)
MANIP_PARAMS = dict(A.ARM_PARAMS)  # Manipulator.yaml's sim block is Houndarm.yaml's
# the random Franka states of the GPU physics comparison.  After 20 PGS simulates the oracle's own float32 build sits at
# the edge of the position tolerance (2e-5 rad) for most seeds: of seeds 1..8 it leaves 0 to 4 of 64 envs beyond it,
# worst 0.6 to 2.5 tolerances.  Seed 6 is the one with the most room (none beyond, worst 0.57), so the 2 % cap asks the
# kernel for no more than float32 gives (tests/test_manipulator_cpu.py checks it)
PHYSICS_SEED = 6
PHYSICS_CASES = A.PHYSICS_CASES
TORQUE_BOUND = 1e-4      # |got - ref| <= 1e-4 max(1, |ref|), the project's rule for the OSC kernels
ALGORITHM_BOUND = 1e-8   # the restatement's two algorithms agree to this: the torque bound is attainable


class ManipFakeGym(A.ArmFakeGym):
    """ArmFakeGym for a 7-dof arm: every Jacobian row is a perturbed [I6 | 0] (6 x 7, full row rank, condition number
    of a few), and every fifth env's arm is HEAVY times heavier."""

    def refresh_jacobian_tensors(self, sim):
        rng = np.random.RandomState(self.seed + 1000 + sim.t)
        shape = tuple(sim.jac_t.shape)
        j = np.eye(6, shape[-1])[None, None] + rng.normal(0.0, 0.15, shape)
        sim.jac_t.copy_(torch.from_numpy(j.astype(np.float32)))

    def refresh_mass_matrix_tensors(self, sim):
        A.FakeGym.refresh_mass_matrix_tensors(self, sim)
        sim.mm_t[1::HEAVY_EVERY] *= HEAVY


def fixture_cfg(num_envs: int = N_ENVS) -> dict:
    """Manipulator.yaml on the CPU pipeline with the fixture's settings; env.asset names the packed Franka relative to
    tests/golden (point_at_fixture makes the root absolute for the run)."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    cfg = compose("config", ["task=Manipulator", f"num_envs={num_envs}", "sim_device=cpu", "pipeline=cpu"])["task"]
    cfg["env"]["episodeLength"] = EPISODE_LENGTH
    cfg["env"]["frankaDofNoise"] = DOF_NOISE
    cfg["env"]["asset"] = {"assetRoot": "", "assetFileNameFranka": MANIP_MODEL}
    return cfg


def point_at_fixture(cfg: dict) -> dict:
    cfg["env"]["asset"] = {"assetRoot": GOLDEN, "assetFileNameFranka": MANIP_MODEL}
    return cfg


stagger, place_commands = A.stagger, A.place_commands


# ---------------------------------------------------------------- the float64 restatement
def gauss_jordan_inverse(a):
    """Batched inverse [..., n, n] by Gauss-Jordan elimination with partial pivoting (float64): the restatement's
    second algorithm, independent of LAPACK."""
    a = np.array(a, np.float64)
    n = a.shape[-1]
    flat = a.reshape(-1, n, n)
    out = np.empty_like(flat)
    for b, m in enumerate(flat):
        w = np.concatenate([m, np.eye(n)], axis=1)
        for c in range(n):
            piv = c + int(np.argmax(np.abs(w[c:, c])))
            w[[c, piv]] = w[[piv, c]]
            w[c] = w[c] / w[c, c]
            for r in range(n):
                if r != c:
                    w[r] = w[r] - w[r, c] * w[c]
        out[b] = w[:, n:]
    return out.reshape(a.shape)


def osc_float64(actions, jac, mm, eef, dof, effort_limits, action_scale=1.0, default=DEFAULT_POSE, inverse=None,
                parts=False):
    """manipulator.py:534-561 restated in float64 on float32 inputs: actions [n, 6], jac [n, 6, nd], mm [n, nd, nd],
    eef [n, 13], dof [n, nd, 2] -> clamped torques [n, nd] (float64).  dpose is the reference's float32 product;
    ``inverse`` is the matrix inverse to use (numpy's LAPACK one, or gauss_jordan_inverse).  parts=True returns
    (clamped, unclamped)."""
    f = np.float64
    inverse = inverse or np.linalg.inv
    dpose = (np.asarray(actions, np.float32) * np.asarray(CMD_LIMIT, np.float32) / np.float32(action_scale)).astype(f)
    J, M, eef, dof = (np.asarray(a, f) for a in (jac, mm, eef, dof))
    nd = M.shape[-1]
    kp, kpn = np.float32(KP), np.float32(KP_NULL)
    kd, kdn = f(np.float32(2) * np.sqrt(kp)), f(np.float32(2) * np.sqrt(kpn))  # float32 gains, as torch holds them
    kp, kpn = f(kp), f(kpn)
    default = np.asarray(np.asarray(default, np.float32), f)  # the task holds its default pose in float32
    Jt = np.transpose(J, (0, 2, 1))
    Minv = inverse(M)
    Meef = inverse(J @ Minv @ Jt)
    u = Jt @ Meef @ (kp * dpose - kd * eef[:, 7:])[..., None]
    q, qd = dof[:, :, 0], dof[:, :, 1]
    u_null = kdn * -qd + kpn * (np.mod(default - q + np.pi, 2 * np.pi) - np.pi)
    u_null = M @ u_null[..., None]
    u = (u + (np.eye(nd)[None] - Jt @ (Meef @ J @ Minv)) @ u_null)[..., 0]
    lim = np.asarray(effort_limits, f)[None]
    clamped = np.clip(u, -lim, lim)
    return (clamped, u) if parts else clamped


def restatement(d, t, **kw):
    """osc_float64 on step t of a recording."""
    return osc_float64(d["ctl_actions"][t], d["ctl_jac"][t], d["ctl_mm"][t], d["ctl_eef"][t], d["ctl_dof"][t],
                       d["effort_limits"], **kw)


def algorithm_gap(d):
    """The largest |LAPACK - Gauss-Jordan| / max(1, |LAPACK|) of the restatement over a recording, on the unclamped
    torques: how far two correct float64 evaluations of the recorded inputs lie apart."""
    worst = 0.0
    for t in range(d["ctl_actions"].shape[0]):
        a = restatement(d, t, parts=True)[1]
        b = restatement(d, t, parts=True, inverse=gauss_jordan_inverse)[1]
        worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
    return worst


def assert_fixture_conditions(d):
    """The cases a Manipulator recording must hold (the generator asserts them, the tests re-check them)."""
    k = d["reset_count_in"]
    steps = len(k)
    eef, cmd = d["in_eef"], d["in_commands"]
    dist = np.linalg.norm(eef[..., :3] - cmd, axis=-1)
    vel_term = 1.0 - np.tanh(10.0 * np.linalg.norm(eef[..., 7:], axis=-1))
    reset_q = np.concatenate([d["dof_state"][t][d["in_reset"][t] != 0, :, 0] for t in range(steps)])  # [resets, 7]
    lower, upper = d["dof_lower"], d["dof_upper"]
    default = np.asarray(DEFAULT_POSE, np.float32)
    free = reset_q[:, :ND - 2]
    at_lower, at_upper = free == lower[None, :ND - 2], free == upper[None, :ND - 2]
    tq, lim = np.abs(d["torques"]), d["effort_limits"][None, None, :]
    big, small = slice(0, 4), slice(4, 7)
    assert tuple(d["effort_limits"]) == EFFORT
    cases = {"time-out resets": int((d["time_outs"] != 0).sum()), "steps without a reset": int((k == 0).sum()),
             "steps resetting exactly one env": int((k == 1).sum()),
             "in-reach envs with a positive velocity term": int(((dist < 0.02) & (vel_term > 1e-3)).sum()),
             "out-of-reach envs": int((dist >= 0.02).sum()),
             "joints clamped on both bounds": int((at_lower.any(axis=0) & at_upper.any(axis=0)).sum()),
             "unclamped reset positions": int((~at_lower & ~at_upper).sum()),
             "clamped torques on the 87 N m joints": int((tq[..., big] == lim[..., big]).sum()),
             "unclamped torques on the 87 N m joints": int((tq[..., big] < lim[..., big]).sum()),
             "clamped torques on the 12 N m joints": int((tq[..., small] == lim[..., small]).sum()),
             "unclamped torques on the 12 N m joints": int((tq[..., small] < lim[..., small]).sum())}
    for what, count in cases.items():
        assert count > 0, f"fixture lacks: {what}"
    # joints 6 and 7 exactly at their defaults after every reset (manipulator.py:413)
    assert len(reset_q) > 0 and (reset_q[:, ND - 2:] == default[None, ND - 2:]).all()
    init_q = d["init_dof_state"][:, :, 0]
    assert (init_q[:, ND - 2:] == default[None, ND - 2:]).all()
    # the bound is attainable: two float64 algorithms on the recorded inputs agree far inside it
    gap = algorithm_gap(d)
    assert gap <= ALGORITHM_BOUND, f"LAPACK and Gauss-Jordan restatements differ by {gap:.3g} max(1, |ref|)"
    cases["restatement algorithm gap"] = gap
    # and the reference's own float32 torques sit inside half the CPU comparison's tolerance of it
    slack = np.abs(d["torques"] - d["torques64"]) / (1e-4 + 1e-4 * np.abs(d["torques64"]))
    assert slack.max() <= 0.5, f"float32 torques use {slack.max():.3g} of the tolerance against float64"
    cases["float32 torque error / tolerance"] = float(slack.max())
    return cases


# ---------------------------------------------------------------- the packed Franka on the simulator
def franka():
    """(articulation, flat model) of the packed Franka with the task's asset options."""
    import json
    from isaacgymenv_amd.isaacgym._assets import RawModel, build_articulation
    from isaacgymenv_amd.isaacgym._model import flatten
    with open(os.path.join(GOLDEN, MANIP_MODEL)) as f:
        art = build_articulation(RawModel.from_json(json.load(f)), MANIP_OPTS)
    flat = flatten(art)
    flat["self_collide"] = 0  # (fixed base: its pairs are dropped)
    return art, flat


def franka_states(n, seed=0, moving=True):
    """Random states in the oracle's layout: the welded root at (0, 0, 1) with the arm clear of the ground, joints well
    inside their limits (away from the limit margin), random velocities and efforts."""
    rng = np.random.RandomState(seed)
    art, flat = franka()
    lower = np.array([d.lower for d in art.dofs]) + 0.35
    upper = np.array([d.upper for d in art.dofs]) - 0.35
    root = np.zeros((n, 13))
    root[:, 2] = 1.0
    root[:, 6] = 1.0
    dof = np.zeros((n, ND, 2))
    dof[:, :, 0] = rng.uniform(lower, upper, (n, ND))
    tau = np.zeros((n, ND))
    if moving:
        dof[:, :, 1] = rng.normal(0.0, 0.5, (n, ND))
        tau = rng.uniform(-2.0, 2.0, (n, ND))
    mu = np.ones((n, max(1, flat["ns"])))
    return root, dof, tau, mu


def make_sim(n, params, disable_gravity):
    """A libgymsim sim of the packed Franka (collision filter 0 as the task creates it) through the drop-in gymapi."""
    gym = _g.acquire_gym()
    sp = _g.SimParams()
    sp.dt, sp.substeps, sp.up_axis = params["dt"], params["substeps"], _g.UP_AXIS_Z
    sp.gravity = _g.Vec3(*params["gravity"])
    sp.use_gpu_pipeline = True
    sp.physx.use_gpu = True
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
    opts.default_dof_drive_mode = _g.DOF_MODE_EFFORT
    for k, v in MANIP_OPTS.items():
        setattr(opts, k, v)
    opts.disable_gravity = disable_gravity
    asset = gym.load_asset(sim, GOLDEN, MANIP_MODEL, opts)
    for i in range(n):
        env = gym.create_env(sim, _g.Vec3(-1, -1, 0), _g.Vec3(1, 1, 1), 8)
        pose = _g.Transform()
        pose.p = _g.Vec3(0, 0, 1.0)
        handle = gym.create_actor(env, asset, pose, "franka", i, 0, 0)
        props = gym.get_actor_dof_properties(env, handle)
        props["driveMode"][:] = _g.DOF_MODE_EFFORT
        props["stiffness"][:] = 0.0
        props["damping"][:] = 0.0
        gym.set_actor_dof_properties(env, handle, props)
    gym.prepare_sim(sim)
    return gym, sim
