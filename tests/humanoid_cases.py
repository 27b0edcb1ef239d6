"""Humanoid test cases -- TEST INFRASTRUCTURE shared by tests/golden/make_golden_humanoid.py, tests/test_humanoid_cpu.py
and the Humanoid GPU tests: the fake simulator the task is recorded on, the fixture's settings and the cases it must
hold, the packed body as an articulation, and the states of the physics comparison.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from tests.fakegym_flat import FlatFakeGym

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL = "nv_humanoid.model.json"
N_ENVS, STEPS = 32, 30
EPISODE_LENGTH = 12
FAKE_SEED = 2027
ND = 21
# envs per initial progress value 0..11 (sum 32): no env at 0 and one at 1, so the recording holds a step that resets
# nobody and a step that resets exactly one env (the falls below are kept off those two steps' envs)
STAGGER_COUNTS = (0, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4)
STAGGER_STEP = 1  # before this step: the first step resets every env (reset_buf starts at ones), which would undo it
TILT_EVERY, TILT = 4, 0.09   # every fourth env's torso quaternion walks 9x faster: up / heading projections cross
SINK_EVERY, SINK = 8, 0.09   # every eighth env (offset 3) sinks 9 cm a step: below terminationHeight after 6 steps
# the fake narrows three joints' ranges (the task reads its limits from the actor's dof properties): with the body's
# own ranges 0 lies inside every range, so the start pose is 0 everywhere and only the knee's upper bound (2 degrees)
# is within a reset offset's reach
LIMIT_OVERRIDES = {"right_elbow": (0.1, 0.87),       # lower > 0: the start pose is the lower limit, the clamp engages there
                   "left_shoulder1": (-1.57, -0.1),  # upper < 0: the start pose is the upper limit
                   "left_elbow": (-0.05, 0.87)}      # 0 inside, the lower limit within a draw's reach
HUMANOID_OPTS = dict(angular_damping=0.01, max_angular_velocity=100.0, default_dof_drive_mode=0)
# Humanoid.yaml's sim block in the oracle's terms (dt 1/60, 2 substeps, 4/0 iterations, contact offset 2 cm)
HUMANOID_PARAMS = dict(dt=0.0166, substeps=2, gravity=[0.0, 0.0, -9.81], pos_iters=4, vel_iters=0,
                       contact_offset=0.02, rest_offset=0.0, max_depen_vel=10.0, collect_contacts=0, has_ground=1,
                       ground_friction=1.0)
FEET = ("right_foot", "left_foot")


class HumanoidFakeGym(FlatFakeGym):
    """FlatFakeGym (DOF force tensor) whose torsos tilt and sink in some envs and whose actors report the narrowed
    ranges of LIMIT_OVERRIDES."""

    def get_actor_dof_properties(self, env, actor):
        p = super().get_actor_dof_properties(env, actor)
        names = env.actors[actor].asset.art.dof_names()
        for name, (lo, hi) in LIMIT_OVERRIDES.items():
            p["lower"][names.index(name)] = lo
            p["upper"][names.index(name)] = hi
        return p

    def simulate(self, sim):
        super().simulate(sim)
        rng = np.random.RandomState(self.seed + 7000 + sim.t)
        q = sim.root[::TILT_EVERY, 3:7] + torch.from_numpy(rng.normal(0, TILT, (len(sim.root[::TILT_EVERY]), 4))
                                                          .astype(np.float32))
        sim.root[::TILT_EVERY, 3:7] = q / q.norm(dim=1, keepdim=True)
        sim.root[3::SINK_EVERY, 2] -= SINK


def fixture_cfg(num_envs: int = N_ENVS) -> dict:
    """Humanoid.yaml on the CPU pipeline with the fixture's 12-step episodes."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    cfg = compose("config", ["task=Humanoid", f"num_envs={num_envs}", "sim_device=cpu", "pipeline=cpu"])["task"]
    cfg["env"]["episodeLength"] = EPISODE_LENGTH
    return cfg


def point_at_fixture(cfg: dict) -> dict:
    cfg["env"]["asset"] = {"assetRoot": GOLDEN, "assetFileName": MODEL}
    return cfg


def stagger(env):
    """Once, before step STAGGER_STEP: spread progress_buf so the time-outs do not all fall on one step.  The sinking
    envs take the late phases, so the first steps that reset nobody / exactly one env stay that way."""
    n = env.num_envs
    values = np.sort(np.resize(np.repeat(np.arange(EPISODE_LENGTH), STAGGER_COUNTS), n))
    order = np.concatenate([np.setdiff1d(np.arange(n), np.arange(3, n, SINK_EVERY)), np.arange(3, n, SINK_EVERY)])
    out = np.zeros(n, dtype=np.int64)
    out[order] = values
    env.progress_buf[:] = torch.from_numpy(out).to(env.progress_buf.device)


def assert_fixture_conditions(d):
    """The cases a Humanoid recording must hold (the generator asserts them, the tests re-check them).  "A step" of
    the joint-limit case is one env's step: the knees rest at 0.975 of their range, so some env of 32 is beyond 0.98
    at every time step."""
    k = d["reset_count_in"]
    obs = d["out_obs"]
    fallen = obs[:, :, 0] < float(d["termination_height"])
    beyond = (np.abs(obs[:, :, 12:33]) > 0.98).any(-1)
    lo, hi = d["dof_limits_lower"], d["dof_limits_upper"]
    q = np.concatenate([d["in_dof"][t].reshape(-1, ND, 2)[d["in_reset"][t] != 0, :, 0] for t in range(len(k))])
    cases = {"height terminations": int((fallen & (d["out_reset"] != 0)).sum()),
             "time-outs": int(((d["time_outs"] != 0) & ~fallen).sum()),
             "steps without a reset": int((k == 0).sum()), "steps resetting exactly one env": int((k == 1).sum()),
             "heading_proj above 0.8": int((obs[:, :, 11] > 0.8).sum()),
             "heading_proj below 0.8": int((obs[:, :, 11] <= 0.8).sum()),
             "up_proj above 0.93": int((obs[:, :, 10] > 0.93).sum()),
             "up_proj below 0.93": int((obs[:, :, 10] <= 0.93).sum()),
             "env steps with a scaled dof beyond 0.98": int(beyond.sum()),
             "env steps with none": int((~beyond).sum()),
             "reset positions clamped at the lower limit": int((q == lo[None]).sum()),
             "reset positions clamped at the upper limit": int((q == hi[None]).sum()),
             "unclamped reset positions": int(((q > lo[None]) & (q < hi[None])).sum())}
    for what, count in cases.items():
        assert count > 0, f"fixture lacks: {what}"
    return cases


# ---------------------------------------------------------------- the packed body and the physics comparison's states
def load_humanoid():
    """(articulation, flat model) of the packed body with the task's asset options."""
    from isaacgymenv_amd.isaacgym._assets import RawModel, build_articulation
    from isaacgymenv_amd.isaacgym._model import flatten
    with open(os.path.join(GOLDEN, MODEL)) as f:
        raw = RawModel.from_json(json.load(f))
    art = build_articulation(raw, HUMANOID_OPTS)
    return art, flatten(art)


def sensor_bodies(art):
    """Dynamic bodies of the two foot sensors (the API takes reported link indices)."""
    names = art.link_names()
    return [art.links[names.index(n)].body for n in FEET]


PHYSICS_N = 64
PHYSICS_SEED = 12  # chosen on the float32 oracle with the drives on: of seeds 3..12 it leaves 0 envs beyond tolerance in
# both cases (seed 4 too); seeds 3, 5, 9, 10 leave one env after 20 simulates (inside the cap), seeds 6, 7, 8, 11 two
# (solver, simulates, efforts as a fraction of each motor's limit).  The long case runs without efforts: 20 simulates
# carry float32 rounding far enough as it is (physics_states)
PHYSICS_CASES = (("tgs", 1, 0.02), ("pgs", 20, 0.0))


# arm poses (shoulder1, shoulder2, elbow) that lay the lower arm on the torso within the contact offset, found by
# sampling the arm joints' ranges against the oracle's self-contact query
RIGHT_ARM_ON_TORSO = (0.849, -0.145, 0.873)
LEFT_ARM_ON_TORSO = (0.912, -1.544, 0.748)
LIMIT_DOFS = 5       # dofs per env put on a limit in the third kind of state, drawn from LIMIT_JOINTS: the joints
# that reach a limit without folding one shape into another (a hip or the waist at its limit self-penetrates by
# centimetres, which no state of the task holds)
LIMIT_JOINTS = ("right_knee", "left_knee", "right_elbow", "left_elbow", "right_ankle_y", "right_ankle_x",
                "left_ankle_y", "left_ankle_x")
UPPER_ONLY = ("right_knee", "left_knee", "right_elbow", "left_elbow")  # (their lower limits fold the limb onto itself)
SETTLE_STEPS = 120   # simulates of the fp64 oracle that bring the lying envs to rest before the comparison starts


def physics_states(n=PHYSICS_N, seed=PHYSICS_SEED):
    """(root [n,13], dof [n,21,2], tau [n,21] uniform in +-1 times each motor's effort limit -- a case scales them --,
    mu [n,ns]) float64, every value a float32: a third of the envs standing
    at rest with both feet in ground contact; a third lying on the back with both lower arms laid across the torso
    (self-contacts), brought to rest by SETTLE_STEPS simulates of the fp64 oracle; a third in the air with LIMIT_DOFS
    dofs on a limit or up to 0.03 rad beyond it, moving further out.  The states are quiet on purpose: an unactuated
    40 kg humanoid in contact is a chaotic system, and after 20 simulates the oracle's own float32 build leaves
    STATE_TOL (one simulate's tolerances) in a quarter of the envs from states that merely drop 2 mm onto the ground,
    and in nine of ten with 30 % efforts (tests/test_humanoid_physics_cpu.py records what it leaves from these)."""
    from tests import helpers as H
    art, flat = load_humanoid()
    flat["self_collide"] = 1
    rng = np.random.RandomState(seed)
    lo, hi = flat["lower"], flat["upper"]
    root = np.zeros((n, 13))
    root[:, 6] = 1.0
    dof = np.zeros((n, ND, 2))
    names = art.dof_names()
    arms = [(names.index(f"{side}_{j}"), v) for side, pose in (("right", RIGHT_ARM_ON_TORSO), ("left", LEFT_ARM_ON_TORSO))
            for j, v in zip(("shoulder1", "shoulder2", "elbow"), pose)]
    kind = np.arange(n) % 3
    for i in range(n):
        if kind[i] == 0:    # standing: the soles (foot capsules, radius 0.027, 1.285 below the root) up to 1 mm into the plane
            root[i, 2] = 1.2845 + rng.uniform(-0.0005, 0.0005)
            dof[i, :, 0] = rng.uniform(-0.002, 0.002, ND)
        elif kind[i] == 1:  # lying on the back, the lower arms on the torso
            root[i, 2] = 0.105 + rng.uniform(0.0, 0.01)
            a = -np.pi / 2 + rng.uniform(-0.05, 0.05)
            root[i, 3:7] = [0.0, np.sin(a / 2), 0.0, np.cos(a / 2)]
            dof[i, :, 0] = rng.uniform(-0.02, 0.02, ND)
            for j, v in arms:
                dof[i, j, 0] = v + rng.uniform(-0.01, 0.01)
        else:               # in the air, some dofs on a limit or slightly beyond it
            root[i, 2] = 3.0
            dof[i, :, 0] = rng.uniform(-0.03, 0.03, ND)
            for j in rng.choice([names.index(x) for x in LIMIT_JOINTS], LIMIT_DOFS, replace=False):
                low = rng.rand() < 0.5 and names[j] not in UPPER_ONLY
                dof[i, j, 0] = lo[j] - rng.uniform(0.0, 0.03) if low else hi[j] + rng.uniform(0.0, 0.03)
                dof[i, j, 1] = (-1.0 if low else 1.0) * rng.uniform(0.0, 0.2)
    mu = np.full((n, flat["ns"]), 1.0)
    lying = np.nonzero(kind == 1)[0]
    r, d, _, _ = H.oracle_run(flat, dict(HUMANOID_PARAMS, solver_type=0), root[lying], dof[lying],
                              np.zeros((len(lying), ND)), mu[lying], 64, SETTLE_STEPS)
    root[lying], dof[lying] = r, d
    tau = rng.uniform(-1.0, 1.0, (n, ND)) * flat["effort"]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return f32(root), f32(dof), f32(tau), mu


def make_sim(n, params):
    """A libgymsim sim of the packed body as the task creates it (collision filter 0, sensors on both feet, every dof in
    DOF_MODE_POS with the MJCF's stiffness and damping toward 0, the DOF force tensor acquired) through the drop-in
    gymapi."""
    from isaacgymenv_amd.isaacgym import gymapi as g
    gym = g.acquire_gym()
    sp = g.SimParams()
    sp.dt, sp.substeps, sp.up_axis = params["dt"], params["substeps"], g.UP_AXIS_Z
    sp.gravity = g.Vec3(*params["gravity"])
    sp.use_gpu_pipeline = True
    sp.physx.use_gpu = True
    sp.physx.num_threads = 2
    sp.physx.num_position_iterations = params["pos_iters"]
    sp.physx.num_velocity_iterations = params["vel_iters"]
    sp.physx.contact_offset = params["contact_offset"]
    sp.physx.rest_offset = params["rest_offset"]
    sp.physx.max_depenetration_velocity = params["max_depen_vel"]
    sp.physx.contact_collection = g.ContactCollection(params["collect_contacts"])
    sp.physx.solver_type = int(params.get("solver_type", 0))
    sim = gym.create_sim(0, -1, g.SIM_PHYSX, sp)
    plane = g.PlaneParams()
    plane.static_friction = params.get("ground_friction", 1.0)
    gym.add_ground(sim, plane)
    opts = g.AssetOptions()
    for k, v in HUMANOID_OPTS.items():
        setattr(opts, k, v)
    asset = gym.load_asset(sim, GOLDEN, MODEL, opts)
    for name in FEET:
        gym.create_asset_force_sensor(asset, gym.find_asset_rigid_body_index(asset, name), g.Transform())
    for i in range(n):
        env = gym.create_env(sim, g.Vec3(-1, -1, 0), g.Vec3(1, 1, 1), 8)
        pose = g.Transform()
        pose.p = g.Vec3(0, 0, 1.34)
        actor = gym.create_actor(env, asset, pose, "humanoid", i, 0, 0)
        props = gym.get_actor_dof_properties(env, actor)  # the passive joint springs and dampers, as the task sets them
        props["driveMode"][:] = g.DOF_MODE_POS
        gym.set_actor_dof_properties(env, actor, props)
    gym.acquire_dof_force_tensor(sim)
    gym.prepare_sim(sim)
    return gym, sim


def drive_gains(art):
    """(kp, kd) of the task's joint drives: the MJCF's stiffness and damping of every dof."""
    return (np.array([d.stiffness for d in art.dofs], dtype=np.float64),
            np.array([d.damping for d in art.dofs], dtype=np.float64))


def oracle_reference(art, flat, params, root, dof, tau, mu, steps, bits=64):
    """The oracle with the task's drives after `steps` simulates: (fields with the foot sensors, expected DOF force of
    the last substep [n, 21], its tolerance) -- tests/dof_force_cases.Case.reference's construction: the state before
    the last substep is steps - 1 whole simulates and one single-substep simulate of dt / 2."""
    from tests import dof_force_cases as D
    from tests import helpers as H
    gains = drive_gains(art)
    n = root.shape[0]
    z = np.zeros((n, ND))
    sb = sensor_bodies(art)
    kw = dict(nsens=2, sensor_bodies=sb, drives=gains, pos_targets=z, vel_targets=z)
    assert int(params["substeps"]) == 2
    h = float(params["dt"]) / 2
    r0, d0 = (root, dof) if steps == 1 else H.oracle_run(flat, params, root, dof, tau, mu, bits, steps - 1, **kw)[:2]
    db = H.oracle_run(flat, dict(params, dt=h, substeps=1), r0, d0, tau, mu, bits, 1, **kw)[1]
    ra, da, _, sa = H.oracle_run(flat, params, r0, d0, tau, mu, bits, 1, **kw)
    force, tol, _ = D.expected_force(flat, h, gains, db, da, tau, z, z)
    return H.state_fields(ra, da, sens=sa), force, tol
