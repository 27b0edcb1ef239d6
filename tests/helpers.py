"""Shared test helpers (test infrastructure)."""
import json
import os

import numpy as np

from isaacgymenv_amd.isaacgym._assets import PACKED_DIR, RawModel, build_articulation
from isaacgymenv_amd.isaacgym._model import flatten

ANYMAL_OPTS = dict(collapse_fixed_joints=True, replace_cylinder_with_capsule=True)
CARTPOLE_OPTS = dict(fix_base_link=True)
ANYMAL_DEFAULT = {"LF_HAA": 0.03, "LH_HAA": 0.03, "RF_HAA": -0.03, "RH_HAA": -0.03, "LF_HFE": 0.4,
                  "LH_HFE": -0.4, "RF_HFE": 0.4, "RH_HFE": -0.4, "LF_KFE": -0.8, "LH_KFE": 0.8,
                  "RF_KFE": -0.8, "RH_KFE": 0.8}
# AnymalTerrain.yaml:129-146
ANYMAL_PARAMS = dict(dt=0.005, substeps=1, gravity=[0.0, 0.0, -9.81], pos_iters=4, vel_iters=1,
                     contact_offset=0.02, rest_offset=0.0, max_depen_vel=100.0, collect_contacts=1,
                     has_ground=1, ground_friction=1.0)
# Cartpole.yaml:23-42
CARTPOLE_PARAMS = dict(dt=0.0166, substeps=2, gravity=[0.0, 0.0, -9.81], pos_iters=4, vel_iters=0,
                       contact_offset=0.02, rest_offset=0.001, max_depen_vel=100.0, collect_contacts=0,
                       has_ground=1, ground_friction=1.0)


# Ant.yaml:42-61 (dt 1/60, 2 substeps, 4/0 iterations, contact collection never)
ANT_PARAMS = dict(dt=0.0166, substeps=2, gravity=[0.0, 0.0, -9.81], pos_iters=4, vel_iters=0,
                  contact_offset=0.02, rest_offset=0.0, max_depen_vel=10.0, collect_contacts=0,
                  has_ground=1, ground_friction=1.0, limit_margin=0.1)
ANT_FEET = [2, 4, 6, 8]  # bodies whose names contain "foot" (ant.py:166-173)

# UsefulHound.yaml:161-180 (dt 0.005, 1 substep, 4/1 iterations, contact collection last substep);
# asset options useful_hound.py:318-329 (fixed joints kept: 19 dynamic bodies, 24 links)
HOUND_OPTS = dict(collapse_fixed_joints=False, replace_cylinder_with_capsule=False, fix_base_link=False,
                  density=0.001, angular_damping=0.0, linear_damping=0.0, armature=0.0, thickness=0.01)
HOUND_PARAMS = dict(dt=0.005, substeps=1, gravity=[0.0, 0.0, -9.81], pos_iters=4, vel_iters=1,
                    contact_offset=0.02, rest_offset=0.0, max_depen_vel=100.0, collect_contacts=1,
                    has_ground=1, ground_friction=1.0, limit_margin=0.1)


# collision filters of the reference tasks' create_actor calls: 0 (self-collision) for AnymalTerrain
# (anymal_terrain.py:282) and UsefulHound (useful_hound.py:421), 1 for Ant (ant.py:190) and Cartpole
# (cartpole.py:107).  flatten() results of these helpers carry it as flat["self_collide"], which the
# oracle (OracleSim) and make_gpu_sim follow.
SELF_COLLIDE = {"anymal": 1, "hound": 1, "ant": 0, "cartpole": 0, "hound_new": 0}
# hound.py:170-181 (the fork's own quadruped, assets/urdf/Hound_new/Hound.urdf; collision filter 1, :208) and
# cfg/task/Hound.yaml:31-32,53 (position drives 85 / 2, fixed joints kept): no compiled topology -- the
# runtime-sized kernel (gs_generic.hip) runs it
HOUND_NEW_OPTS = dict(HOUND_OPTS, collapse_fixed_joints=False)
HOUND_NEW_DRIVES = (np.full(12, 1, dtype=np.int32), np.full(12, 85.0), np.full(12, 2.0))


def load_art(name, opts):
    with open(os.path.join(PACKED_DIR, name)) as f:
        return build_articulation(RawModel.from_json(json.load(f)), opts)


def anymal():
    art = load_art("anymal_c.model.json", ANYMAL_OPTS)
    flat = flatten(art)
    flat["self_collide"] = SELF_COLLIDE["anymal"]
    return art, flat


def cartpole():
    art = load_art("cartpole.model.json", CARTPOLE_OPTS)
    flat = flatten(art)
    flat["self_collide"] = SELF_COLLIDE["cartpole"]
    return art, flat


def ant():
    art = load_art("nv_ant.model.json", dict(angular_damping=0.0))
    flat = flatten(art)
    flat["self_collide"] = SELF_COLLIDE["ant"]
    return art, flat


def hound():
    art = load_art("hound.model.json", HOUND_OPTS)
    flat = flatten(art)
    flat["self_collide"] = SELF_COLLIDE["hound"]
    return art, flat


def hound_new():
    art = load_art("hound_new.model.json", HOUND_NEW_OPTS)
    flat = flatten(art)
    flat["self_collide"] = SELF_COLLIDE["hound_new"]
    return art, flat


def hound_new_states(n, seed=0, spread=1.0):
    """Random Hound_new states: standing near Hound.yaml's 0.62 m (feet on, above or into the ground), tilted,
    moving, joints within their limits."""
    rng = np.random.RandomState(seed)
    art, flat = hound_new()
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    root[:, 2] = rng.uniform(0.35, 0.65, n)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.3 * spread, n)
    root[:, 3:6] = axis * np.sin(ang / 2)[:, None]
    root[:, 6] = np.cos(ang / 2)
    root[:, 7:10] = rng.normal(0, 0.3 * spread, (n, 3))
    root[:, 10:13] = rng.normal(0, 0.5 * spread, (n, 3))
    dof = np.zeros((n, 12, 2))
    leg = np.tile([0.0, 0.6, -1.2], 4)
    dof[:, :, 0] = leg + rng.uniform(-0.4, 0.4, (n, 12)) * spread
    dof[:, :, 1] = rng.normal(0, 1.0 * spread, (n, 12))
    tau = rng.uniform(-60, 60, (n, 12))
    mu = np.repeat(rng.uniform(0.5, 1.25, (n, 1)), flat["ns"], axis=1)
    return root, dof, tau, mu


def hound_states(n, seed=0, spread=1.0):
    """Random Hound states: legs near a stand, arm anywhere in its limits, base tilted/moving."""
    rng = np.random.RandomState(seed)
    art, flat = hound()
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    root[:, 2] = rng.uniform(0.45, 0.7, n)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.3 * spread, n)
    root[:, 3:6] = axis * np.sin(ang / 2)[:, None]
    root[:, 6] = np.cos(ang / 2)
    root[:, 7:10] = rng.normal(0, 0.3 * spread, (n, 3))
    root[:, 10:13] = rng.normal(0, 0.5 * spread, (n, 3))
    dof = np.zeros((n, 18, 2))
    leg = np.tile([0.0, 0.7, -1.4], 4)
    dof[:, :12, 0] = leg + rng.uniform(-0.3, 0.3, (n, 12)) * spread
    dof[:, 12:, 0] = rng.uniform(-1.5, 1.5, (n, 6))
    dof[:, :, 1] = rng.normal(0, 1.0 * spread, (n, 18))
    tau = np.concatenate([rng.uniform(-80, 80, (n, 12)), rng.uniform(-20, 20, (n, 6))], axis=1)
    mu = np.repeat(rng.uniform(0.5, 1.25, (n, 1)), flat["ns"], axis=1)
    return root, dof, tau, mu


def ant_states(n, seed=0, spread=1.0):
    """Random Ant states: near/on/into the ground, dofs anywhere in (and slightly beyond) their limits."""
    rng = np.random.RandomState(seed)
    art, flat = ant()
    lo, hi = flat["lower"], flat["upper"]
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    root[:, 2] = rng.uniform(0.2, 0.6, n)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.4 * spread, n)
    root[:, 3:6] = axis * np.sin(ang / 2)[:, None]
    root[:, 6] = np.cos(ang / 2)
    root[:, 7:10] = rng.normal(0, 0.5 * spread, (n, 3))
    root[:, 10:13] = rng.normal(0, 1.0 * spread, (n, 3))
    dof = np.zeros((n, 8, 2))
    dof[:, :, 0] = rng.uniform(lo - 0.05, hi + 0.05, (n, 8))
    dof[:, :, 1] = rng.normal(0, 2.0 * spread, (n, 8))
    tau = rng.uniform(-15, 15, (n, 8))
    mu = np.full((n, flat["ns"]), 1.5)
    return root, dof, tau, mu


def anymal_states(n, seed=0, spread=1.0):
    """Random but physically plausible ANYmal states: standing, airborne, penetrating, tilted."""
    rng = np.random.RandomState(seed)
    art, flat = anymal()
    q0 = np.array([ANYMAL_DEFAULT[d] for d in art.dof_names()])
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    root[:, 2] = rng.uniform(0.45, 0.65, n)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.25 * spread, n)
    root[:, 3:6] = axis * np.sin(ang / 2)[:, None]
    root[:, 6] = np.cos(ang / 2)
    root[:, 7:10] = rng.normal(0, 0.3 * spread, (n, 3))
    root[:, 10:13] = rng.normal(0, 0.5 * spread, (n, 3))
    dof = np.zeros((n, 12, 2))
    dof[:, :, 0] = q0 * rng.uniform(0.5, 1.5, (n, 12))
    dof[:, :, 1] = rng.normal(0, 1.0 * spread, (n, 12))
    tau = rng.uniform(-80, 80, (n, 12))
    mu = np.repeat(rng.uniform(0.5, 1.25, (n, 1)), flat["ns"], axis=1)
    return root, dof, tau, mu


def make_gpu_sim(kind: str, n: int, params: dict, terrain=None, host: bool = False, threads: int = 4, drives=None,
                 self_collide=None, asset_hook=None):
    """A libgymsim sim built through the drop-in gymapi (GPU pipeline); `terrain` (terrain_from_heights)
    adds the heightfield mesh with gym.add_triangle_mesh.  host=True builds the sim_device=cpu pipeline
    instead (physx.use_gpu False: libgymsim's host backend on `threads` threads, host tensors).
    drives = (mode [nd], stiffness [nd], damping [nd]) sets every actor's dof drive properties.
    asset_hook(asset) may edit the loaded asset's model (asset.flat) before the envs are created."""
    from isaacgymenv_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.dt = params["dt"]
    sp.substeps = params["substeps"]
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(*params["gravity"])
    sp.use_gpu_pipeline = not host
    sp.physx.use_gpu = not host
    sp.physx.num_threads = threads
    sp.physx.num_position_iterations = params["pos_iters"]
    sp.physx.num_velocity_iterations = params["vel_iters"]
    sp.physx.contact_offset = params["contact_offset"]
    sp.physx.rest_offset = params["rest_offset"]
    sp.physx.max_depenetration_velocity = params["max_depen_vel"]
    sp.physx.contact_collection = gymapi.ContactCollection(params["collect_contacts"])
    # the oracle's parameter dicts mean PGS unless they say otherwise (gymapi's own default is TGS, as Isaac Gym's)
    sp.physx.solver_type = int(params.get("solver_type", 0))
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    assert sim is not None
    if params.get("has_ground", 1):
        plane = gymapi.PlaneParams()
        plane.static_friction = params.get("ground_friction", 1.0)
        gym.add_ground(sim, plane)
    if terrain is not None:
        tm = gymapi.TriangleMeshParams()
        tm.nb_vertices = terrain["vertices"].shape[0]
        tm.nb_triangles = terrain["triangles"].shape[0]
        tm.transform.p = gymapi.Vec3(*terrain["shift"])
        tm.static_friction = terrain["friction"]
        gym.add_triangle_mesh(sim, terrain["vertices"].flatten(), terrain["triangles"].flatten(), tm)
    opts = gymapi.AssetOptions()
    sensors = []
    if kind == "anymal":
        opts.collapse_fixed_joints = True
        opts.replace_cylinder_with_capsule = True
        opts.default_dof_drive_mode = gymapi.DOF_MODE_EFFORT
        asset = gym.load_asset(sim, "/nonexistent", "urdf/anymal_c/urdf/anymal_minimal.urdf", opts)
    elif kind == "ant":
        opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
        opts.angular_damping = 0.0
        asset = gym.load_asset(sim, "/nonexistent", "mjcf/nv_ant.xml", opts)
        for b in ANT_FEET:
            gym.create_asset_force_sensor(asset, b, gymapi.Transform())
    elif kind == "hound":
        for k, v in HOUND_OPTS.items():
            setattr(opts, k, v)
        opts.default_dof_drive_mode = gymapi.DOF_MODE_EFFORT
        asset = gym.load_asset(sim, "/nonexistent", "urdf/UsefulHound/urdf/Hound.urdf", opts)
    elif kind == "hound_new":
        for k, v in HOUND_NEW_OPTS.items():
            setattr(opts, k, v)
        opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE  # hound.py:171
        asset = gym.load_asset(sim, "/nonexistent", "urdf/Hound_new/Hound.urdf", opts)
    else:
        opts.fix_base_link = True
        asset = gym.load_asset(sim, "/nonexistent", "urdf/cartpole.urdf", opts)
    if asset_hook is not None:
        asset_hook(asset)
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 8)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0, 0, {"anymal": 0.62, "ant": 0.44, "hound": 0.55, "hound_new": 0.62}.get(kind, 2.0))
        a = gym.create_actor(env, asset, pose, kind, i, 0 if (SELF_COLLIDE[kind] if self_collide is None else self_collide)
                             else 1, 0)
        if drives is not None:
            props = gym.get_actor_dof_properties(env, a)
            props["driveMode"], props["stiffness"], props["damping"] = drives
            gym.set_actor_dof_properties(env, a, props)
    gym.prepare_sim(sim)
    return gym, sim


def make_host_sim(kind: str, n: int, params: dict, terrain=None, threads: int = 4, drives=None, self_collide=None,
                  asset_hook=None):
    return make_gpu_sim(kind, n, params, terrain=terrain, host=True, threads=threads, drives=drives,
                        self_collide=self_collide, asset_hook=asset_hook)


def heavy_base(flat, scale=1000.0):
    """ANYmal's base body (27.8 kg) made `scale` times heavier, inertia alike (a body above
    1000 kg must still rest on the plane)."""
    flat["mass"][0] *= scale
    flat["inertia"][0] *= scale
    flat["lmass"][0] *= scale


def upside_down_anymal(n):
    """ANYmal on its back: the base capsule (radius 0.1, axis x) 5 mm above the plane, legs up."""
    root = np.zeros((n, 13))
    root[:, 2] = 0.105
    root[:, 3] = 1.0  # quat xyzw (1, 0, 0, 0): 180 degrees about x
    dof = np.zeros((n, 12, 2))
    dof[:, :, 0] = [ANYMAL_DEFAULT[d] for d in ("LF_HAA", "LF_HFE", "LF_KFE", "LH_HAA", "LH_HFE", "LH_KFE",
                                                 "RF_HAA", "RF_HFE", "RF_KFE", "RH_HAA", "RH_HFE", "RH_KFE")]
    return root, dof


def sim_self_contacts(sim, mode=0):
    """The sim's self-contact pools from its current state (gs_debug_self_contacts): (contacts [n, npk, 10] float64
    = x xyz, n xyz, separation, friction, body a, body b -- the oracle's self_contacts layout; counts [n])."""
    import torch
    from isaacgymenv_amd.isaacgym import _lib
    n, npk = sim.num_envs, max(1, int(sim.asset.flat["npool"]))
    dev = sim.state.device
    out = torch.zeros((n, npk, 10), dtype=torch.float32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = None if dev.type == "cpu" else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().gs_debug_self_contacts(sim.handle, mode, out.data_ptr(), cnt.data_ptr(), stream),
               "gs_debug_self_contacts")
    return out.cpu().numpy().astype(np.float64), cnt.cpu().numpy()


def load_state_into(sim, root, dof, mu):
    """Write oracle-layout numpy state ([N,13] internal root, [N,nd,2]) into the SoA sim state."""
    import torch
    n, nd = root.shape[0], dof.shape[1]
    st = np.zeros((13 + 2 * nd, n), dtype=np.float32)
    st[0:13] = root.T
    st[13:13 + nd] = dof[:, :, 0].T
    st[13 + nd:] = dof[:, :, 1].T
    sim.state.copy_(torch.from_numpy(st))
    m = np.ones(tuple(sim.shape_mu.shape), dtype=np.float32)
    m[:mu.shape[1]] = mu.T
    sim.shape_mu.copy_(torch.from_numpy(m))


def read_state(sim, nd):
    st = sim.state.cpu().numpy().astype(np.float64)
    n = st.shape[1]
    root = st[0:13].T.copy()
    dof = np.ascontiguousarray(np.stack([st[13:13 + nd].T, st[13 + nd:].T], axis=-1))
    return root, dof


def terrain_from_heights(hf, hs=0.1, vs=0.005, slope_threshold=0.5, shift=(0.0, 0.0, 0.0), friction=1.0):
    """A heightfield as the trimesh gym.add_triangle_mesh receives it (terrain_utils layout, translated by
    `shift`) plus the oracle's terrain dict (world vertices, grid origin, spacing)."""
    from isaacgymenv_amd.isaacgym import terrain_utils
    v, t = terrain_utils.convert_heightfield_to_trimesh(np.asarray(hf, dtype=np.int16), hs, vs, slope_threshold)
    return mesh_terrain(v, t, hf.shape[0], hf.shape[1], hs, shift, friction)


def mesh_terrain(v, t, rows, cols, hs, shift=(0.0, 0.0, 0.0), friction=1.0):
    world = (v.astype(np.float64) + np.asarray(shift)).astype(np.float32)
    grid = v.reshape(rows, cols, 3)
    oracle = dict(vertices=world, rows=rows, cols=cols, x0=float(grid[0, :, 0].min()) + shift[0],
                  y0=float(grid[:, 0, 1].min()) + shift[1], hs=hs, friction=friction)
    return dict(vertices=v, triangles=t, shift=shift, friction=friction, oracle=oracle)


def rough_terrain(seed=0, rows=120, cols=120):
    """Stairs, blocks and a random field around the origin (cells of 0.1 m), centred on (0, 0)."""
    return terrain_from_heights(rough_heights(seed, rows, cols), shift=(-rows * 0.05, -cols * 0.05, 0.0))


def rough_heights(seed=0, rows=120, cols=120):
    """rough_terrain's height samples (int16 counts of 0.005 m)."""
    from isaacgymenv_amd.isaacgym import terrain_utils as tu
    np.random.seed(seed)
    hf = np.zeros((rows, cols), dtype=np.int16)
    a = tu.SubTerrain("a", width=rows // 2, length=cols, vertical_scale=0.005, horizontal_scale=0.1)
    tu.pyramid_stairs_terrain(a, step_width=0.31, step_height=0.08, platform_size=1.0)
    b = tu.SubTerrain("b", width=rows - rows // 2, length=cols, vertical_scale=0.005, horizontal_scale=0.1)
    tu.random_uniform_terrain(b, -0.06, 0.06, step=0.01, downsampled_scale=0.2)
    tu.discrete_obstacles_terrain(b, 0.1, 0.5, 1.0, 10, platform_size=0.5)
    hf[: rows // 2] = a.height_field_raw
    hf[rows // 2:] = b.height_field_raw
    return hf


# per-field tolerances of one simulate (test_physics_gpu.py bounds) for assert_close_or_explained
STATE_TOL = {"pose": (2e-5, 0.0), "q": (2e-5, 0.0), "vel": (5e-3, 5e-3), "qd": (5e-3, 5e-3), "cf": (1.0, 2e-2),
             "sens": (0.09, 2e-2)}


def state_fields(root, dof, cf=None, sens=None):
    """The compared outputs of a simulate as {field: [n, ...]} (STATE_TOL keys)."""
    out = {"pose": root[:, 0:7], "vel": root[:, 7:13], "q": dof[:, :, 0], "qd": dof[:, :, 1]}
    if cf is not None:
        out["cf"] = cf
    if sens is not None:
        out["sens"] = sens
    return out


# an off-tolerance env counts as explained only when, field by field, its error is at most this multiple of the
# largest deviation the reference itself shows from fp32-rounding-sized perturbations of the same start
EXPLAIN_K = 2.0


def parity_report(line):
    """Print a parity report line and append it to $PARITY_REPORT when set (the GPU round scripts set it,
    so the reports of a GPU run are kept under profiles/)."""
    print(line)
    path = os.environ.get("PARITY_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


def parity_dump(name, **arrays):
    """On a failing parity check, keep its inputs and outputs for a CPU replay: an .npz under $PARITY_DUMP when set
    (the GPU round scripts point it into gpurun_out/, which comes back from the box)."""
    path = os.environ.get("PARITY_DUMP")
    if path:
        os.makedirs(path, exist_ok=True)
        np.savez_compressed(os.path.join(path, name + ".npz"), **arrays)


def _field_ratios(a, d, tol, n):
    """{field: [n]} -- per env, the largest |a - d| / (atol + rtol |d|) over the field's elements."""
    out = {}
    for k in d:
        at, rt = tol[k]
        dd = np.asarray(d[k], np.float64).reshape(n, -1)
        e = np.abs(np.asarray(a[k], np.float64).reshape(n, -1) - dd)
        out[k] = (e / (at + rt * np.abs(dd))).max(axis=1)
    return out


def oracle_run(flat, params, root, dof, tau, mu, bits=64, steps=1, nc=None, nsens=0, **kw):
    """The physics oracle (fp64, or bits=32: the same restatement compiled with float arithmetic) on copies of
    the inputs: returns float64 (root, dof, cf [n, nc, 3] or None, sens [n, nsens, 6] or None).  kw: OracleSim's
    sensor_bodies / terrain / drives and simulate's pos_targets / vel_targets."""
    from oracle.oracle import OracleSim
    dt = np.float64 if bits == 64 else np.float32
    c = lambda a: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    ctor = {k: kw[k] for k in ("sensor_bodies", "terrain", "drives") if k in kw}
    sim_kw = {k: c(kw[k]) for k in ("pos_targets", "vel_targets") if k in kw}
    o = OracleSim(flat, params, real_bits=bits, **ctor)
    n = root.shape[0]
    r, d = np.array(root, dtype=dt, order="C"), np.array(dof, dtype=dt, order="C")  # copies: stepped in place
    cf = np.zeros((n, nc, 3), dt) if nc else None
    sens = np.zeros((n, nsens, 6), dt) if nsens else None
    for _ in range(steps):
        o.simulate(r, d, c(tau), c(mu), cf, sens=sens, **sim_kw)
    f = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    return f(r), f(d), f(cf), f(sens)


def assert_close_or_explained(actual, desired, rerun, tol=None, max_env_frac=0.02, tries=16, k=EXPLAIN_K, what=""):
    """Every env within tolerance, or its divergence explained by the reference's own sensitivity.

    `rerun(idx, rng)` returns the reference's outputs for envs idx started from a state perturbed at
    fp32-rounding size (same {field: [len(idx), ...]} layout as `desired`).  A rerun taking a third argument
    `bits` is also called with bits=32: the oracle restatement itself run in float arithmetic (oracle_run),
    which measures how far fp32 rounding carries through the spec where the dynamics is ill-conditioned
    (light links, joints at their velocity limits), not only where a contact switches.  For an env beyond
    tolerance, spread[field] is the largest deviation (in tolerance units) of those reruns (`tries` of each
    kind) from the unperturbed fp64 reference; the env is explained only when every field beyond tolerance
    has error <= k * spread[field].  At most `max_env_frac` of the envs may be beyond tolerance at all.  The
    report (worst env, off count, unexplained count, the least-explained envs) goes through parity_report."""
    import inspect
    fp32 = len(inspect.signature(rerun).parameters) >= 3
    tol = tol or STATE_TOL
    n = next(iter(desired.values())).shape[0]
    for f in desired:
        assert np.all(np.isfinite(np.asarray(actual[f], np.float64))), f"{what}: non-finite {f}"
    fr = _field_ratios(actual, desired, tol, n)
    r = np.max(np.stack(list(fr.values())), axis=0)
    off = np.nonzero(r > 1.0)[0]
    spread = {f: np.zeros(n) for f in desired}
    if off.size:
        rng = np.random.RandomState(0)
        sub = {f: np.asarray(v)[off] for f, v in desired.items()}
        for bits in ((64, 32) if fp32 else (64,)):
            for _ in range(tries):
                out = rerun(off, rng, bits) if fp32 else rerun(off, rng)
                pr = _field_ratios(out, sub, tol, off.size)
                for f in desired:
                    spread[f][off] = np.maximum(spread[f][off], pr[f])
    explained = np.ones(n, dtype=bool)
    margin = np.zeros(n)  # error / spread of the env's least-explained field
    for f in desired:
        beyond = fr[f] > 1.0
        m = np.where(beyond, fr[f] / np.maximum(spread[f], 1e-30), 0.0)
        margin = np.maximum(margin, m)
        explained &= ~beyond | (fr[f] <= k * spread[f])
    unexplained = off[~explained[off]]
    w = int(np.argmax(r))
    wf = max(fr, key=lambda f: fr[f][w])
    worst = sorted(off.tolist(), key=lambda i: -margin[i])[:5]
    detail = "; ".join(f"env {i}: {r[i]:.3g}x tol, error/spread {margin[i]:.3g}" for i in worst)
    report = (f"{what}: worst env {w} at {r[w]:.3g} x tolerance in {wf} (reference spread {spread[wf][w]:.3g}); "
              f"{off.size} of {n} envs beyond tolerance, {unexplained.size} unexplained "
              f"{unexplained[:8].tolist()} (rule: error <= {k:g} x spread per field, {tries} perturbed reruns"
              f"{' in fp64 and fp32' if fp32 else ''})"
              + (f"; least explained: {detail}" if off.size else ""))
    parity_report(report)
    assert unexplained.size == 0, report
    assert off.size <= max_env_frac * n, report
    return report


def perturbed(root, dof, idx, rng):
    """root[idx], dof[idx] with fp32-rounding-size noise on positions and velocities."""
    import numpy as np
    r, d = root[idx].copy(), dof[idx].copy()
    m = len(idx)
    r[:, :3] += rng.normal(0, 1e-6, (m, 3))
    r[:, 7:] += rng.normal(0, 1e-5, (m, 6))
    d[:, :, 0] += rng.normal(0, 1e-6, d[:, :, 0].shape)
    d[:, :, 1] += rng.normal(0, 1e-5, d[:, :, 1].shape)
    return r, d


# ---- PPO loss minibatches that reach every branch of the loss on known rows (test_ppo_loss_oracle.py,
# ---- test_ppo_loss_gpu.py); every cycle below runs on (row + seed), the periods 8, 3, 5, 7 pairwise coprime
PPO_E_CLIP = 0.2
PPO_RATIO_TARGETS = (0.5, 0.79, 0.81, 0.95, 1.05, 1.19, 1.21, 2.0)  # >= 1 % from 1 -+ e_clip
PPO_VDIFF = (-2.0, -0.5, 0.0, 0.5, 2.0)  # (values - old_values) / e_clip
PPO_RETURN_OFFSETS = (-0.8, -0.07, 0.07, 0.8, -0.4, 0.4, 0.09)  # returns - (values + clipped value) / 2
PPO_FAR_MU = (1.5, -1.5, 3.0, -3.0)  # every 10th element of mu: the bound loss active on both sides
PPO_INPUTS = ("mu", "values", "logstd", "actions", "old_neglogp", "advantages", "old_values", "returns")
PPO_ONE_ROW_SEEDS = range(120)  # a one-row minibatch is one cell: lcm(8, 3, 5) = 120 phases (>= 5 * 7, 40) reach all


def ppo_minibatch(B, A, seed=0, mu_f16=False, values_f16=False, mu=None, values=None):
    """{name: CPU tensor} of rl_ppo_loss's inputs (mu / values fp16 or f32, the rest f32) at e_clip = PPO_E_CLIP:
    logstd in +-0.5; mu in +-1 with a tenth of its elements at PPO_FAR_MU; actions = mu + sigma N(0, 1);
    old_neglogp = neglogp(mu, actions) + log(target), so that the ratio is PPO_RATIO_TARGETS[(row + seed) % 8];
    advantages U(0.1, 2), -U(0.1, 2), exactly 0 by (row + seed) % 3; old_values = values - e_clip PPO_VDIFF[...];
    returns = (values + clipped value) / 2 + PPO_RETURN_OFFSETS[...].  Everything is derived from the rounded mu /
    values (given ones: the heads tests') in float64 and then rounded to f32."""
    import torch
    e = PPO_E_CLIP
    rng = np.random.RandomState(1000 + seed)
    idx = np.arange(B) + seed
    logstd = rng.uniform(-0.5, 0.5, A).astype(np.float32)
    m = rng.uniform(-1.0, 1.0, (B, A))
    j = (np.arange(B * A) + seed).reshape(B, A)
    m = np.where(j % 10 == 3, np.asarray(PPO_FAR_MU)[(j // 10) % 4], m)
    v = rng.uniform(-1.0, 1.0, B)
    if mu is None:
        mu = torch.from_numpy(m).to(torch.float16 if mu_f16 else torch.float32)
    if values is None:
        values = torch.from_numpy(v).to(torch.float16 if values_f16 else torch.float32)
    mu64, v64 = mu.double().numpy().reshape(B, A), values.double().numpy().reshape(B)
    ls64 = logstd.astype(np.float64)
    sigma = np.exp(ls64)
    actions = (mu64 + sigma * rng.normal(size=(B, A))).astype(np.float32)
    z = (actions.astype(np.float64) - mu64) / sigma
    nlp = 0.5 * (z * z).sum(-1) + 0.5 * np.log(2.0 * np.pi) * A + ls64.sum()
    old_neglogp = (nlp + np.log(np.asarray(PPO_RATIO_TARGETS)[idx % 8])).astype(np.float32)
    mag = rng.uniform(0.1, 2.0, B)
    advantages = np.where(idx % 3 == 0, mag, np.where(idx % 3 == 1, -mag, 0.0)).astype(np.float32)
    old_values = (v64 - e * np.asarray(PPO_VDIFF)[idx % 5]).astype(np.float32)
    ov64 = old_values.astype(np.float64)
    vpc = ov64 + np.clip(v64 - ov64, -e, e)
    returns = (0.5 * (v64 + vpc) + np.asarray(PPO_RETURN_OFFSETS)[idx % 7]).astype(np.float32)
    t = torch.from_numpy
    return dict(mu=mu.reshape(B, A).contiguous(), values=values.reshape(B).contiguous(), logstd=t(logstd),
                actions=t(actions), old_neglogp=t(old_neglogp), advantages=t(advantages), old_values=t(old_values),
                returns=t(returns))


def ppo_heads_minibatch(B, H, A, seed=0):
    """rl_ppo_heads_loss's inputs on a lattice where the heads are exact in any summation order: hidden_a, hidden_c
    [B][H] in {-1, 0, 1}, w_mu [A][H], w_v [H] = k / 256 with |k| <= 2, b_mu, b_v = k / 256 with |k| <= 512 (every
    4th b_mu at +-1.5 or +-2: mu beyond +-1.1), all fp16; so mu = hidden_a w_mu^T + b_mu and v = hidden_c w_v + b_v
    are multiples of 1 / 256 below 8, exact in fp16.  Rows whose mu would come within 0.02 of +-1.1 are redrawn.
    Then ppo_minibatch on that mu and v.  Returns (heads {name: CPU fp16 tensor}, minibatch)."""
    import torch
    rng = np.random.RandomState(2000 + seed)
    ha = rng.randint(-1, 2, (B, H)).astype(np.float64)
    hc = rng.randint(-1, 2, (B, H)).astype(np.float64)
    w_mu = rng.randint(-2, 3, (A, H)) / 256.0
    w_v = rng.randint(-2, 3, H) / 256.0
    kb = rng.randint(-180, 181, A)
    far = np.asarray([384, -384, 512, -512])[(np.arange(A) // 4) % 4]
    b_mu = np.where(np.arange(A) % 4 == 2, far, kb) / 256.0
    b_v = np.asarray([rng.randint(-128, 129) / 256.0])
    for _ in range(100):
        mu = ha @ w_mu.T + b_mu
        bad = (np.abs(np.abs(mu) - 1.1) < 0.02).any(axis=1)
        if not bad.any():
            break
        ha[bad] = rng.randint(-1, 2, (int(bad.sum()), H))
    else:
        raise AssertionError("ppo_heads_minibatch: could not move mu away from +-1.1")
    v = hc @ w_v + b_v[0]
    assert np.abs(mu).max() < 8 and np.abs(v).max() < 8
    h = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16)  # noqa: E731
    heads = dict(hidden_a=h(ha), hidden_c=h(hc), w_mu=h(w_mu), b_mu=h(b_mu), w_v=h(w_v), b_v=h(b_v))
    return heads, ppo_minibatch(B, A, seed, mu=h(mu), values=h(v))


# ---- the comparison rule of the float64-referenced kernel tests (test_ppo_loss_gpu.py, test_learner_kernels_gpu.py)
def field_check(tag, seen, fails, what, field, got, r64, r32, zeros=False, err_32=None):
    """max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64| for one output field; its figures printed
    under `tag` and the largest err_kernel / err_f32 and err_kernel / bar kept in seen[field].  err_32: the float32
    reference's error where the caller has it from more than this one draw (one-number outputs)."""
    got, r64, r32 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, r64, r32))
    assert got.shape == r64.shape == r32.shape, (what, field)
    err_k = float(np.abs(got - r64).max())
    err_32 = float(np.abs(r32 - r64).max()) if err_32 is None else float(err_32)
    bar = 4.0 * err_32 + 4.0 * 2.0 ** -23 * float(np.abs(r64).max())
    r32_ratio = err_k / err_32 if err_32 > 0 else (0.0 if err_k == 0 else float("inf"))
    print(f"[{tag}] {what} {field}: err_kernel {err_k:.3e} err_f32 {err_32:.3e} ratio {r32_ratio:.3g} "
          f"bar {bar:.3e} max|ref| {np.abs(r64).max():.3e}")
    s = seen.setdefault(field, [0.0, 0.0])
    s[0], s[1] = max(s[0], r32_ratio if np.isfinite(r32_ratio) else 0.0), max(s[1], err_k / bar if bar > 0 else 0.0)
    if not np.isfinite(got).all() or not err_k <= bar:
        fails.append(f"{what} {field}: err_kernel {err_k:.3e} > bar {bar:.3e} (err_f32 {err_32:.3e})")
    if zeros and not np.array_equal(got == 0, r64 == 0):
        fails.append(f"{what} {field}: zero pattern differs at {np.nonzero((got == 0) != (r64 == 0))[0][:8].tolist()}")


def np64(t):
    """float64 numpy of a tensor (any device / dtype) or of a list of Python floats."""
    import torch
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def bits(t):
    """The tensor's bit patterns as integers, on the CPU."""
    import torch
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    import torch
    return torch.equal(bits(a), bits(b))


# ---- inputs of the learner's bookkeeping kernels (test_learner_oracle.py asserts what is claimed here;
# ---- test_learner_kernels_gpu.py relies on it)
# the shapes of tests/test_learner_kernels_gpu.py (rl_rms_normalize rows x cols, rl_policy_kl M x A, rl_act_heads N, H, A)
RMS_SHAPES = [(1, 3), (2, 1), (63, 5), (64, 8), (65, 256), (4097, 7), (1000, 255)]
KL_SHAPES = [(1, 1), (255, 12), (257, 12), (1000, 8), (65537, 2)]
ACT_HEADS_SHAPES = [(1, 1, 1), (15, 3, 1), (17, 5, 12), (33, 128, 12), (16, 130, 64)]
RMS_KINDS = ("unit", "offset", "small", "constant", "outlier")  # column c is of kind c % 5
RMS_OFFSET, RMS_SMALL, RMS_CONSTANT = 1.0e4, 1.0e-4, 3.25
RMS_CLAMP_MARGIN = 1e-3  # |y| within this of 5: the clamp may go either way in f32


def rms_kinds(cols):
    return np.arange(cols) % len(RMS_KINDS)


def rms_input(rows, cols, seed=0):
    """x [rows][cols] f32 with the column kinds mixed (column c: RMS_KINDS[c % 5]): N(0.3, 1); RMS_OFFSET + N(0, 1)
    (the mean 10^4 standard deviations away); RMS_SMALL N(0, 1); the constant RMS_CONSTANT (M2 == 0); N(0, 1) with
    every 49th row (r + seed) % 49 == 0 at +-300, the sign alternating (about 7 standard deviations of the column: past the
    clamp)."""
    import torch
    rng = np.random.RandomState(3000 + seed)
    z = rng.normal(size=(rows, cols))
    k = rms_kinds(cols)[None, :]
    r = np.arange(rows)[:, None]
    far = ((r + seed) % 49 == 0)
    x = np.where(k == 0, 0.3 + z, np.where(k == 1, RMS_OFFSET + z, np.where(k == 2, RMS_SMALL * z, np.where(
        k == 3, RMS_CONSTANT, np.where(far, 300.0 * np.where(((r + seed) // 49) % 2 == 0, 1.0, -1.0), z)))))
    return torch.from_numpy(x.astype(np.float32))


def rms_state(cols, count, seed=0):
    """Float64 running moments a long run over rms_input's columns would hold, at `count` samples."""
    import torch
    rng = np.random.RandomState(3500 + seed)
    k = rms_kinds(cols)
    mean = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [0.3, RMS_OFFSET, 0.0, RMS_CONSTANT, 0.0])
    var = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [1.0, 1.0, RMS_SMALL ** 2, 1e-12, 1.0 + 9.0e4 / 49])
    mean = mean + 1e-3 * np.sqrt(var) * rng.normal(size=cols)
    return torch.from_numpy(mean), torch.from_numpy(var * (1.0 + 1e-3 * rng.normal(size=cols))), float(count)


def opt_state(n, step, seed=0):
    """(p, m, v) f32 [n] of an Adam run at `step`: p = 0.1 N(0, 1) with every 5th element exactly 0 (there the stored
    parameter carries the step alone); step 0: zero moments; later: m = 1e-3 N(0, 1), v = 1e-6 U(0.5, 2)."""
    import torch
    rng = np.random.RandomState(4000 + seed)
    p = 0.1 * rng.normal(size=n)
    p[::5] = 0.0
    m = np.zeros(n) if step == 0 else 1e-3 * rng.normal(size=n)
    v = np.zeros(n) if step == 0 else 1e-6 * rng.uniform(0.5, 2.0, size=n)
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (p, m, v))


def opt_grad(n, seed, scale=None):
    """A gradient [n] f32 = (scale or 1) 10^U(-5, -2) N(0, 1): sqrt(v) runs from far above eps = 1e-8 to 1e3 eps."""
    import torch
    rng = np.random.RandomState(4500 + seed)
    g = rng.normal(size=n) * 10.0 ** rng.uniform(-5.0, -2.0, size=n) * (scale or 1.0)
    return torch.from_numpy(g.astype(np.float32))


KL_SIGMA_MODES = ("log", "row", "full")  # one log-sigma row (stride 0), one sigma row (stride 0), [M][A] sigmas
KL_KINDS = ("far", "near", "same")


def kl_inputs(M, A, kind="far", sigma_mode="log", half=False, seed=0):
    """dict(mu_new [M][A] fp16 / f32, sigma_new [A] or [M][A] f32 (its log for "log"), mu_old, sigma_old [M][A] f32,
    sigma_is_log, sigma_row_stride).  far: mu_old = mu_new + 0.1 N(0, 1), sigma_old = sigma_new (1 + 0.05 N(0, 1));
    near: mu_old = mu_new + 1e-3 N(0, 1) and equal sigmas; same: mu_old == mu_new exactly, equal sigmas."""
    import torch
    assert kind in KL_KINDS and sigma_mode in KL_SIGMA_MODES
    rng = np.random.RandomState(5000 + seed)
    mu_new = torch.from_numpy(rng.uniform(-1.0, 1.0, (M, A))).to(torch.float16 if half else torch.float32)
    ls = rng.uniform(-0.7, 0.3, (M, A) if sigma_mode == "full" else (A,))
    sg_in = torch.from_numpy(ls if sigma_mode == "log" else np.exp(ls)).to(torch.float32)
    s0 = np.broadcast_to(np.exp(sg_in.double().numpy()) if sigma_mode == "log" else sg_in.double().numpy(), (M, A))
    dmu = dict(far=0.1, near=1e-3, same=0.0)[kind] * rng.normal(size=(M, A))
    mu_old = torch.from_numpy(mu_new.double().numpy() + dmu).to(torch.float32)
    s1 = s0 * (1.0 + 0.05 * rng.normal(size=(M, A))) if kind == "far" else s0
    return dict(mu_new=mu_new, sigma_new=sg_in.contiguous(), mu_old=mu_old,
                sigma_old=torch.from_numpy(np.array(s1)).to(torch.float32),
                sigma_is_log=int(sigma_mode == "log"), sigma_row_stride=A if sigma_mode == "full" else 0)


def kl_scheduler_cases(kl):
    """(threshold, lr, expected lr) around a float64 KL: every threshold puts 2 thr and thr / 2 at a factor of 2
    from the KL, and both clamps (1e-6, 1e-2) are reached."""
    return [(kl / 4, 3e-4, 3e-4 / 1.5), (kl * 4, 3e-4, 3e-4 * 1.5), (kl, 3e-4, 3e-4), (kl / 4, 1.2e-6, 1e-6),
            (kl / 4, 1e-6, 1e-6), (kl * 4, 8e-3, 1e-2), (kl * 4, 1e-2, 1e-2)]


def act_heads_inputs(N, H, A, seed=0, sharp=False):
    """Real-valued act-forward head inputs: hidden [N][2H + 4] f32 (actor columns [0, H), critic [H, 2H), the pad
    NaN: never to be read), w_mu [A][H], b_mu [A], w_v [H], b_v [1], noise [N][A], logstd [A], and the value
    RunningMeanStd's float64 moments vmean, vvar [1].  The raw value has a standard deviation of about 4 (both sides
    of +-5).  sharp: logstd = -5 and b_mu = +-1e3, so |mu| ~ 1e3 against sigma = 0.0067."""
    import torch
    rng = np.random.RandomState(6000 + seed)
    hid = np.full((N, 2 * H + 4), np.nan)
    hid[:, :2 * H] = rng.normal(size=(N, 2 * H))
    w_mu = rng.normal(size=(A, H)) / np.sqrt(H)
    b_mu = np.where(np.arange(A) % 2 == 0, 1.0, -1.0) * 1.0e3 if sharp else 0.1 * rng.normal(size=A)
    w_v = 4.0 * rng.normal(size=H) / np.sqrt(H)
    b_v = rng.normal(size=1)
    logstd = np.full(A, -5.0) if sharp else rng.uniform(-1.0, 0.5, A)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32)  # noqa: E731
    return dict(hidden=t(hid), w_mu=t(w_mu), b_mu=t(b_mu), w_v=t(w_v), b_v=t(b_v), noise=t(rng.normal(size=(N, A))),
                logstd=t(logstd), vmean=torch.tensor([0.731], dtype=torch.float64),
                vvar=torch.tensor([2.37], dtype=torch.float64))


def colsum_inputs(rows, cols, half, seed=0):
    """(g [rows][cols] fp16 / f32 = N(0, 1), grad [cols] f32 = N(0, 1): a nonzero gradient to accumulate onto)."""
    import torch
    rng = np.random.RandomState(7000 + seed)
    g = torch.from_numpy(rng.normal(size=(rows, cols))).to(torch.float16 if half else torch.float32)
    return g, torch.from_numpy(rng.normal(size=cols)).to(torch.float32)


# ---- the matrix-core Linear + ELU kernels (test_linear_oracle.py asserts what is claimed here;
# ---- test_linear_kernels_gpu.py relies on it)
def elementwise_bound(ref64, S, terms, out_half):
    """Per element: h + (terms + 2) 2^-24 S + 4 2^-24 |ref64|.  (terms + 2) 2^-24 S: the forward error bound of an f32
    dot product of `terms` products summed in any order (S = the same sum on absolute values), two more roundings for
    the bias and the epilogue; 4 f32 ulp for expm1f; h: half the fp16 spacing at fp16(ref64) when the output is
    rounded to fp16 (0 for f32 outputs; where fp16(ref64) is infinite the bound is infinite: the caller judges
    overflow by its pattern)."""
    ref64, S = np.asarray(ref64, dtype=np.float64), np.asarray(S, dtype=np.float64)
    u = 2.0 ** -24
    bound = (terms + 2) * u * S + 4.0 * u * np.abs(ref64)
    if out_half:
        with np.errstate(over="ignore", invalid="ignore"):
            r16 = ref64.astype(np.float16)
            fin = np.isfinite(r16)
            # the spacing of the binade |fp16(ref64)| lies in (at a power of two: the wider side, which its rounding
            # interval reaches half of), 2^-24 in the subnormals
            _, e = np.frexp(np.where(fin, np.abs(r16), 0).astype(np.float64))
            h = 0.5 * np.maximum(np.ldexp(1.0, e - 11), 2.0 ** -24)
        bound = bound + np.where(fin, h, np.inf)
    return bound


def elementwise_check(tag, seen, fails, what, field, got, ref64, S, terms, out_half, act=False):
    """Every element of one output field: |got - ref64| <= elementwise_bound (ref64 unrounded).  act: the field went
    through ELU, which is 1-Lipschitz, so the dot product's bound holds for it unchanged (it only labels the
    figures).  Prints the largest err / bound under `tag`, keeps it in seen[field], and returns (that ratio, the
    fraction of elements beyond the bound)."""
    got, ref64 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, ref64))
    bound = elementwise_bound(ref64, np.asarray(S, dtype=np.float64).reshape(-1), terms, out_half)
    assert got.shape == ref64.shape == bound.shape, (what, field)
    err = np.abs(got - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst, beyond = float(ratio.max()), float((ratio > 1.0).mean())
    print(f"[{tag}] {what} {field}{' (ELU)' if act else ''}: elementwise err / bound <= {worst:.3g} over {got.size} "
          f"elements, {beyond:.3%} beyond, terms {terms}")
    seen[field] = max(seen.get(field, 0.0), worst if np.isfinite(worst) else 0.0)
    if not worst <= 1.0:
        at = int(np.argmax(ratio))
        fails.append(f"{what} {field}: elementwise err / bound {worst:.3g} at flat index {at} (got {got[at]!r}, ref "
                     f"{ref64[at]!r}, bound {bound[at]:.3e}); {beyond:.3%} of the elements beyond the bound")
    return worst, beyond


def linear_inputs(M, K, N, seed=0, G=1):
    """x [G][M][K] ~ 1.5 N(0, 1), w [G][N][K] ~ N(0, 0.08 sqrt(188 / K)), bias [G][N] ~ 0.1 N(0, 1): drawn in f32
    (x32, w32, b32: what the f32 kernel gets) and rounded to fp16 (x, w, b).  The pre-activations have a standard
    deviation of about 1.65 at every K and straddle 0."""
    import torch
    rng = np.random.RandomState(9000 + seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    x32 = t(1.5 * rng.normal(size=(G, M, K)))
    w32 = t(0.08 * np.sqrt(188.0 / K) * rng.normal(size=(G, N, K)))
    b32 = t(0.1 * rng.normal(size=(G, N)))
    return dict(x32=x32, w32=w32, b32=b32, x=x32.to(torch.float16), w=w32.to(torch.float16), b=b32.to(torch.float16))


LIN_SPECIAL_Y = (("zero", 0.0), ("negzero", -0.0), ("minus_one", -1.0), ("tiny_neg", -2.0 ** -24), ("max", 65504.0))


def linear_special_elements(M, N):
    """{name: (value, rows, cols)}: the elements of y that linear_bwd_inputs overwrites.  Special i takes the whole
    of row 1 + i and the two elements (16 + 3 i, (5 + 37 i) % N) and (M - 1 - i, (N - 1 - 11 i) % N)."""
    out = {}
    for i, (name, v) in enumerate(LIN_SPECIAL_Y):
        rows = np.concatenate([np.full(N, 1 + i), [16 + 3 * i, M - 1 - i]])
        cols = np.concatenate([np.arange(N), [(5 + 37 * i) % N, (N - 1 - 11 * i) % N]])
        out[name] = (v, rows, cols)
    return out


def linear_single_term_column(i, N):
    """The one column where dy of special row 1 + i is nonzero (every special but minus_one)."""
    return (7 + 13 * i) % N


def linear_bwd_inputs(M, K, N, seed=0, G=1):
    """linear_inputs plus y [G][M][N] = the float64 reference's fp16 ELU output on them (a real layer output) with
    the elements of linear_special_elements overwritten, and dy [G][M][N] ~ N(0, 1) in fp16.  In the special rows
    of 0, -0, the largest fp16 below 0 and 65504, dy is zero except at linear_single_term_column: dZ has one nonzero
    term there, so that row of dx is one exact product rounded once.  The row of -1 keeps its random dy: its dZ and
    its row of dx are exactly 0."""
    import torch
    from oracle import linear_oracle as LO
    d = linear_inputs(M, K, N, seed, G)
    rng = np.random.RandomState(9500 + seed)
    y = torch.stack([LO.linear_fwd(d["x"][g], d["w"][g], d["b"][g], True)[1] for g in range(G)])
    dy = torch.from_numpy(rng.normal(size=(G, M, N))).to(torch.float16)
    for i, (name, (v, rows, cols)) in enumerate(linear_special_elements(M, N).items()):
        y[:, rows, cols] = torch.tensor(v, dtype=torch.float16)
        if name != "minus_one":
            c = linear_single_term_column(i, N)
            keep = dy[:, 1 + i, c].clone()
            dy[:, 1 + i, :] = 0
            dy[:, 1 + i, c] = torch.where(keep == 0, torch.ones_like(keep), keep)
    d.update(y=y, dy=dy)
    return d


def _lin(M, N, K, G=1, **kw):
    return dict(M=M, N=N, K=K, G=G, **kw)


# rl_linear_fwd(_g): y_off = element offset of y in its 16-byte aligned buffer; ldx / ldy 0 = dense; gaps: the
# grouped layout with every stride distinct (see test_linear_kernels_gpu._fwd_layout)
LIN_FWD_CASES = (
    [_lin(64, 128, K) for K in (4, 36, 60, 64, 68, 128, 132, 188, 196)]            # stage edges of kNtStep = 64
    + [_lin(128, 384, 68), _lin(192, 128, 36, ldx=44)]                               # N not a power of two; ldx > K
    + [_lin(M, 128, 36) for M in (320, 576, 832)] + [_lin(320, 384, 36)]             # 5, 9, 13, 15 tiles (1, 3 above)
    + [_lin(4096, 1024, 36), _lin(1024, 512, 36, G=8), _lin(3968, 1024, 36)]         # 128-row form, grouped, just under
    + [_lin(128, 128, 68, y_off=4), _lin(128, 128, 68, ldy=132),                     # direct-store arm
       _lin(128, 128, 68, G=2, ldy=264, y_gstride=132),                              # ... in group 1 only
       _lin(128, 128, 68, G=3, gaps=True)])
LIN_F32_CASES = (
    [_lin(64, 64, K, kstep=ks) for K in (4, 28, 32, 36, 60, 64, 68, 188) for ks in ("32", "64")]
    + [_lin(512, 4096, 36), _lin(2112, 1024, 36)]                                    # 512 / 528 tiles: default stage 64 / 32
    + [_lin(128, 64, 36, G=3, ldy=200, y_gstride=68)]
    + [_lin(192, 64, 36), _lin(576, 64, 36), _lin(320, 192, 36)])                    # 3, 9, 15 tiles (1 above)
LIN_DX_CASES = (
    [_lin(128, N, 128, lddx=ld) for N in (128, 384) for ld in (128, 132, 136)]
    + [_lin(4096, 128, 1024), _lin(3968, 128, 1024), _lin(128, 128, 128, G=3, gaps=True)])
LIN_DW_SPLITS = ((128, 2), (128, 1), (384, 2), (384, 1), (1024, 16))  # rows_per_split 64, 128, 192, 384, 64
LIN_DW_N = (128, 384)
LIN_DW_K = (4, 124, 128, 132, 188)
SPLITK_PARTS = (1, 15, 16, 17, 33)
SPLITK_N = (4, 260, 1539)
TRANSPOSE_SHAPES = ((1, 4), (33, 36), (128, 188))


def linear_fwd_tiles(c, f32=False):
    """Workgroups of a forward case, as the entry points choose their tiles (csrc/rl_linear.hip)."""
    if f32:
        return (c["M"] // 64) * (c["N"] // 64) * c["G"]
    big = (c["M"] // 128) * (c["N"] // 128) * c["G"]
    return big if big >= 256 and c["M"] % 128 == 0 else (c["M"] // 64) * (c["N"] // 128) * c["G"]


def linear_dx_tiles(c):
    big = (c["M"] // 128) * (c["K"] // 128) * c["G"]
    return big if big >= 256 else (c["M"] // 64) * (c["K"] // 128) * c["G"]


# ---- the AnymalTerrain / UsefulHound tail kernels (test_task_oracle.py asserts what is claimed here;
# ---- test_task_kernels_gpu.py relies on it)
TAIL_KINDS = ("ordinary", "base_contact", "knee_one", "knee_many", "shoulder", "tie_norm", "tie_z", "stumble_one",
              "stumble_many", "first_contact", "contact_zero_air", "small_cmd", "prog_at", "prog_below",
              "timeout_reset", "heading_above_pi", "heading_below_minus_pi", "c2_high", "c2_low", "reward_clip",
              "timeout_only")  # env e is of kind e % len(TAIL_KINDS)
TAIL_MARGIN = 1e-3  # every kind keeps this relative distance from every threshold it does not sit on
TAIL_T = 1000       # max_episode_length
TAIL_HEADING_DIFF = {"heading_above_pi": 5.0, "heading_below_minus_pi": -4.0, "c2_high": 2.5, "c2_low": -2.5}
TAIL_BODIES = dict(anymal=dict(nb=13, base=0, knees=(2, 5, 8, 11), feet=(3, 6, 9, 12)),
                   hound=dict(nb=24, base=0, knees=(2, 5, 8, 11), feet=(3, 6, 9, 12), shoulders=(14, 15, 16, 17)))


def tail_kinds(N):
    return np.arange(N) % len(TAIL_KINDS)


def tail_params(N, nd, hound=False, **over):
    """gt_anymal_params as a dict (oracle/task_oracle.py; tests fill the ctypes struct from it): AnymalTerrain.yaml's
    shape with every reward scale nonzero, so that every term counts."""
    bd = TAIL_BODIES["hound" if hound else "anymal"]
    na = nd + 6 if hound else nd
    dt = 0.02
    scales = dict(s_termination=-2.0, s_lin_vel_xy=3.0, s_lin_vel_z=-4.0, s_ang_vel_z=0.5, s_ang_vel_xy=-0.05,
                  s_orient=-0.3, s_torque=-0.00002, s_joint_acc=-0.0005, s_base_height=-0.7, s_air_time=1.0,
                  s_collision=-1.0, s_stumble=-2.0, s_action_rate=-0.01, s_hip=-0.2)
    leg = [0.03, 0.4, -0.8, 0.03, -0.4, 0.8, -0.03, 0.4, -0.8, -0.03, -0.4, 0.8, 0.1, -0.1, 0.2, -0.2]
    p = dict(num_envs=N, num_dofs=nd, num_bodies=bd["nb"], num_obs=12 + 2 * nd + 140 + na + (10 if hound else 0),
             base_index=bd["base"], num_feet=4, feet_idx=list(bd["feet"]), num_knees=4, knee_idx=list(bd["knees"]),
             hip_dofs=[0, 3, 6, 9], allow_knee_contacts=0, max_episode_length=TAIL_T, dt=dt,
             lin_vel_scale=2.0, ang_vel_scale=0.25, dof_pos_scale=1.0, dof_vel_scale=0.05, height_meas_scale=5.0,
             default_dof_pos=leg[:nd] + [0.0] * (16 - nd),
             base_init_state=[0.0, 0.0, 0.62, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    p.update({k: v * dt for k, v in scales.items()})
    p.update(over)
    return p


def tail_hound(N, seed=0, num_shoulders=4):
    """The gt_anymal_hound fields the statements read (oracle/task_oracle.py), with eef [N][13] rigid-body rows."""
    rng = np.random.RandomState(8500 + seed)
    return dict(num_actions=18, num_shoulders=num_shoulders, shoulder_idx=list(TAIL_BODIES["hound"]["shoulders"]),
                arm_default=[0.0, 0.5, -0.5, 0.0, 0.3, 0.0], arm_lower=[-0.2, 0.3, -0.7, -0.2, 0.1, -0.2],
                arm_upper=[0.2, 0.7, -0.3, 0.2, 0.5, 0.2], arm_noise2=1.0,
                eef_rows=rng.normal(size=(N, 13)).astype(np.float32),
                arm_commands=rng.uniform(-1, 1, (N, 3)).astype(np.float32))


def _quat_rotate64(q, v):
    u, w = q[:, :3], q[:, 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def tail_inputs(N, nd, seed=0, hound=False):
    """(params, bufs, kinds) for gt_anymal_post_physics_a / _b: env e is of kind TAIL_KINDS[e % K].  Every env tracks
    its command (reward decisively positive) with small torques, small forces on every body and feet either loaded
    (fz 2..50) or free; on top of that, per kind: the base at (0, 0, 3); knee 0 / every knee at (0, 2, 0); a shoulder
    at (2, 0, 0) (terminates only in the Hound form); base and knee 0 at exactly (0, 1, 0) (norm 1.0: no contact);
    every foot at exactly (0, 0, 1) (neither contact nor stumble); foot 0 / every foot at (4, 4, +-0.5) (stumble);
    every foot loaded with air time 0.3 / with air time 0; |command| = 0.05 with first contacts (the air-time gate);
    progress + 1 = T - 1 / T - 2; the time-out flag with a base contact / alone; command heading - heading =
    TAIL_HEADING_DIFF (+5: beyond pi, wrapped; -4: below -pi, kept by C fmod and clamped at -1 where a floored
    remainder gives +1; +-2.5: the clamp alone); torques of 2000 (the reward clips at 0).  All f32, timeout_buf bool."""
    rng = np.random.RandomState(8000 + seed)
    K = len(TAIL_KINDS)
    kind = tail_kinds(N)
    is_ = lambda name: kind == TAIL_KINDS.index(name)  # noqa: E731
    p = tail_params(N, nd, hound)
    bd = TAIL_BODIES["hound" if hound else "anymal"]
    na, nb = (nd + 6 if hound else nd), bd["nb"]
    root = np.zeros((N, 13))
    root[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    root[:, 2] = rng.uniform(0.45, 0.65, N)
    axis = rng.normal(size=(N, 3))
    axis[:, 2] *= 0.0
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    tilt, yaw = rng.uniform(0, 0.25, N), rng.uniform(-3.0, 3.0, N)
    qt = np.concatenate([axis * np.sin(tilt / 2)[:, None], np.cos(tilt / 2)[:, None]], 1)
    qy = np.stack([np.zeros(N), np.zeros(N), np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    # q = yaw * tilt (Hamilton product, xyzw)
    a, b = qy, qt
    q = np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                  a[:, 3] * b[:, 1] - a[:, 0] * b[:, 2] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0],
                  a[:, 3] * b[:, 2] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3],
                  a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], 1)
    root[:, 3:7] = q
    va = rng.uniform(-np.pi, np.pi, N)
    blv = np.concatenate([rng.uniform(0.3, 1.0, (N, 1)) * np.stack([np.cos(va), np.sin(va)], 1),
                          rng.normal(0, 0.05, (N, 1))], 1)
    blv[is_("small_cmd"), :2] = 0.05 * np.array([0.6, 0.8])
    bav = np.concatenate([rng.normal(0, 0.3, (N, 2)), rng.uniform(-0.4, 0.4, (N, 1))], 1)
    root[:, 7:10] = _quat_rotate64(q, blv)
    root[:, 10:13] = _quat_rotate64(q, bav)
    root = root.astype(np.float32)
    q32 = root[:, 3:7].astype(np.float64)
    fwd = _quat_rotate64(q32, np.tile([1.0, 0.0, 0.0], (N, 1)))
    heading = np.arctan2(fwd[:, 1], fwd[:, 0])
    diff = 2.0 * bav[:, 2] + rng.uniform(-0.02, 0.02, N)
    for name, v in TAIL_HEADING_DIFF.items():
        diff = np.where(is_(name), v + rng.uniform(-0.05, 0.05, N), diff)
    cmd = np.zeros((N, 4))
    cmd[:, :2] = blv[:, :2] + rng.uniform(-0.02, 0.02, (N, 2))
    cmd[is_("small_cmd"), :2] = 0.05 * np.array([0.6, 0.8])
    cmd[:, 2] = rng.uniform(-1, 1, N)
    cmd[:, 3] = heading + diff
    cf = rng.uniform(-0.2, 0.2, (N, nb, 3))
    feet, knees = list(bd["feet"]), list(bd["knees"])
    loaded = rng.rand(N, 4) < 0.5
    air = np.where(rng.rand(N, 4) < 0.5, rng.uniform(0.02, 0.6, (N, 4)), 0.0)
    for k in range(4):
        cf[:, feet[k], 2] = np.where(loaded[:, k], rng.uniform(2.0, 50.0, N), cf[:, feet[k], 2])
    cf[is_("base_contact") | is_("timeout_reset"), bd["base"]] = [0.0, 0.0, 3.0]
    cf[is_("knee_one"), knees[0]] = [0.0, 2.0, 0.0]
    for k in knees:
        cf[is_("knee_many"), k] = [0.0, 2.0, 0.0]
    cf[is_("shoulder"), TAIL_BODIES["hound"]["shoulders"][1] if hound else 1] = [2.0, 0.0, 0.0]
    cf[is_("tie_norm"), bd["base"]] = [0.0, 1.0, 0.0]
    cf[is_("tie_norm"), knees[0]] = [0.0, 1.0, 0.0]
    for k in range(4):
        cf[is_("tie_z"), feet[k]] = [0.0, 0.0, 1.0]
        cf[is_("stumble_many"), feet[k]] = [4.0, 4.0, -0.5 if k % 2 else 0.5]
        m = is_("first_contact") | is_("contact_zero_air") | is_("small_cmd")
        cf[m, feet[k], 2] = 3.0 + k
        air[is_("first_contact") | is_("small_cmd"), k] = 0.3 + 0.1 * k
        air[is_("contact_zero_air"), k] = 0.0
    cf[is_("stumble_one"), feet[0]] = [4.0, 4.0, 0.5]
    tq = rng.uniform(-20, 20, (N, na))
    tq[is_("reward_clip")] = 2000.0
    act = rng.uniform(-1, 1, (N, na))
    lact = act + rng.uniform(-0.2, 0.2, (N, na))
    dof = np.zeros((N, na, 2))
    default = np.asarray(p["default_dof_pos"])[:nd]
    dof[:, :nd, 0] = default + rng.uniform(-0.2, 0.2, (N, nd))
    dof[:, nd:, 0] = rng.uniform(-0.5, 0.5, (N, na - nd))
    dof[:, :, 1] = rng.normal(0, 1.0, (N, na))
    lqd = dof[:, :nd, 1] + rng.normal(0, 0.5, (N, nd))
    prog = rng.randint(0, TAIL_T - 100, N).astype(np.int64)
    prog[is_("prog_at")] = TAIL_T - 2
    prog[is_("prog_below")] = TAIL_T - 3
    timeout = is_("timeout_reset") | is_("timeout_only")
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)  # noqa: E731
    bufs = dict(root_states=root, contact_forces=f(cf), dof_state=f(dof), torques=f(tq), actions=f(act),
                last_actions=f(lact), last_dof_vel=f(lqd), commands=f(cmd), feet_air_time=f(air), progress_buf=prog,
                randomize_buf=rng.randint(0, 5000, N).astype(np.int64), timeout_buf=timeout.copy(),
                reset_buf=np.zeros(N, dtype=np.uint8), episode_sums=tail_episode_sums(N, seed),
                noise_scale=f(rng.uniform(0.0, 0.2, p["num_obs"])), clip_obs=np.inf, measured_heights=None)
    assert K == len(TAIL_KINDS)
    return p, bufs, kind


def tail_episode_sums(N, seed=0):
    """episode_sums [13][N] f32 ~ N(0, 0.5) (tail_inputs' own; seeds 0..15 give the err_f32 of episode_out)."""
    return np.random.RandomState(8100 + seed).normal(0, 0.5, (13, N)).astype(np.float32)


def tail_heights(N, seed=0):
    """measured_heights [N][140] for post_b: root z - 0.5 - h runs from about -1.6 to 1.6, so the +-1 clip binds on
    both sides and not at all."""
    rng = np.random.RandomState(8700 + seed)
    return rng.uniform(-1.5, 1.5, (N, 140)).astype(np.float32)


def reset_masks_cases(N):
    """{name: uint64 mask words [ceil(N / 64)]}, hand-built (not made by post_a): none, all, first, last, alternating
    and, for N > 4096 (more than 64 words: the second pass of the prefix and of the staging loop), flagged envs in
    the last wave only and in the first and last waves.  Bits at and beyond N are 0."""
    W = (N + 63) // 64
    full = lambda n: np.uint64((1 << n) - 1)  # noqa: E731
    allm = np.full(W, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    allm[W - 1] = full(N - 64 * (W - 1))
    one = lambda e: np.uint64(1) << np.uint64(e & 63)  # noqa: E731
    first, last = np.zeros(W, np.uint64), np.zeros(W, np.uint64)
    first[0] = one(0)
    last[(N - 1) >> 6] = one(N - 1)
    cases = dict(none=np.zeros(W, np.uint64), all=allm, first=first, last=last,
                 alternating=allm & np.uint64(0x5555555555555555))
    if N > 4096:
        lw = np.zeros(W, np.uint64)
        lw[W - 1] = allm[W - 1]
        fl = lw.copy()
        fl[0] = np.uint64(0x8000000000000421)
        cases.update(last_wave=lw, first_and_last_wave=fl)
    return cases


def popcount(masks):
    return int(sum(bin(int(w)).count("1") for w in np.asarray(masks).view(np.uint64)))


def reset_draws(k, nd, seed=0, terrain=False, hound=False):
    """The uniforms of one reset (u_pos, u_vel [k][nd], u_cmd_* [k], u_root_xy [k][2], u_arm [k][6]) and
    AnymalTerrain's torch_rand_float maps.  Every fourth row draws a command below the 0.25 gate; u_arm's rows run
    through 0.02 and 0.98 (the arm clamp at both limits with tail_hound's arm_noise2 = 1 and limits of +-0.2)."""
    rng = np.random.RandomState(8800 + seed)
    u = lambda *s: rng.uniform(0.0, 1.0, s).astype(np.float32)  # noqa: E731
    d = dict(u_pos=u(k, nd), u_vel=u(k, nd), u_cmd_x=u(k), u_cmd_y=u(k), u_cmd_h=u(k),
             pos_range=1.0, pos_lower=0.5, vel_range=0.2, vel_lower=-0.1, cmd_x_range=2.0, cmd_x_lower=-1.0,
             cmd_y_range=2.0, cmd_y_lower=-1.0, cmd_h_range=6.28, cmd_h_lower=-3.14)
    small = np.arange(k) % 4 == 1
    d["u_cmd_x"][small] = np.float32(0.55)  # (0.1, 0.06): norm 0.117 < 0.25
    d["u_cmd_y"][small] = np.float32(0.53)
    extra = {}
    if terrain:
        extra["u_root_xy"] = u(k, 2)
    if hound:
        ua = u(k, 6)
        ua[np.arange(k) % 3 == 0] = np.float32(0.02)
        ua[np.arange(k) % 3 == 1] = np.float32(0.98)
        extra["u_arm"] = ua
    return d, extra


TERRAIN_STATES = 7  # odd: the alternating mask reaches every state


def terrain_reset_inputs(N, ids=None, seed=0, update_levels=1, batch_norm=0.4):
    """gt_anymal_terrain_reset's fields for N envs on a 5 x 3 tile grid (env_length 8: a tile is left beyond 4 m; 20 s
    episodes) for a reset of the envs `ids` (default: all).  The commands of the envs in `ids` have norm
    batch_norm / sqrt(len(ids)) each, so that torch.norm over all of them is batch_norm and the level-down threshold
    0.25 * 20 * batch_norm: 2 m at 0.4 (below the tile's 4 m), 10 m at 2.0 (beyond it: every env that leaves its tile
    also moves down, net 0).  Every other env commands 10 m/s: counting it would put the threshold beyond any walk.
    Env e is of state e % 7 by the distance it walked from its origin -- 0: 0.05 m (down); 1: 0.05 m on level 0 (clip
    at 0); 2: 5 m (up, or net 0); 3: 5 m on the top level (wraps to 0, or net 0); 4: 3 m (neither, or down);
    5: 1 m (down by the batch's norm; by its own command's, 5 * batch_norm / sqrt(k), only for k < 5); 6: as 0.
    Returns (fields, root_xy [N][2], cmd_xy [N][2], state); root x, y and commands go into the buffers."""
    rng = np.random.RandomState(8900 + seed)
    rows, cols = 5, 3
    state = np.arange(N) % TERRAIN_STATES
    ids = np.arange(N) if ids is None else np.asarray(ids)
    levels = rng.randint(1, rows - 1, N).astype(np.int64)
    levels[state == 1] = 0
    levels[state == 3] = rows - 1
    types = rng.randint(0, cols, N).astype(np.int64)
    to = rng.uniform(-20, 20, (rows, cols, 3)).astype(np.float32)
    eo = to[levels, types].copy()
    walked = np.select([state == 0, state == 1, state == 2, state == 3, state == 4], [0.05, 0.05, 5.0, 5.0, 3.0], 1.0)
    ang = rng.uniform(-3, 3, N)
    root_xy = eo[:, :2] + walked[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    cmd_xy = np.tile([6.0, 8.0], (N, 1))
    ca = rng.uniform(-3, 3, len(ids))
    cmd_xy[ids] = batch_norm / np.sqrt(max(len(ids), 1)) * np.stack([np.cos(ca), np.sin(ca)], 1)
    t = dict(terrain_levels=levels, terrain_types=types, env_origins=eo, terrain_origins=to, env_rows=rows,
             env_cols=cols, update_levels=update_levels, env_length=8.0, max_episode_length_s=20.0, xy_range=1.0,
             xy_lower=-0.5)
    return t, root_xy.astype(np.float32), cmd_xy.astype(np.float32), state


HEIGHTS_SHAPES = ((1, 1), (3, 140), (37, 7))  # (N, num_points)
HEIGHTS_MAP = dict(rows=48, cols=37, border=1.0, hs=0.1, vs=0.005)
HEIGHTS_NEAR = 1e-4  # cells: closer to an integer, f32 may truncate to either neighbour


def heights_inputs(N, num_points, seed=0):
    """(samples int16 [48][37] with distinct values, border, hs, vs, root_states [N][13], points [N][np][3]).  Probe
    (e, k) is of kind (e * np + k) % 7 by where it lands before clipping: 0-1 the interior; 2-5 up to 3 cells beyond
    the x-low, x-high, y-low, y-high border of the map; 6: within one cell below 0 after the border shift (truncation
    goes to cell 0, toward zero).  Envs alternate yaw-only and full (tilted) quaternions; the kernel and the reference
    use the yaw of (0, 0, qz, qw) normalised either way."""
    rng = np.random.RandomState(9900 + seed)
    m = HEIGHTS_MAP
    rows, cols, border, hs = m["rows"], m["cols"], m["border"], m["hs"]
    samples = (rng.permutation(rows * cols).astype(np.int64) - rows * cols // 2).astype(np.int16).reshape(rows, cols)
    root = np.zeros((N, 13))
    root[:, 0] = rng.uniform(0.5, rows * hs - 2 * border + 0.5, N)
    root[:, 1] = rng.uniform(0.5, cols * hs - 2 * border + 0.5, N)
    root[:, 2] = 0.6
    yaw = rng.uniform(-3.1, 3.1, N)
    qz, qw = np.sin(yaw / 2), np.cos(yaw / 2)
    full = np.arange(N) % 2 == 1
    root[:, 3] = np.where(full, 0.2, 0.0)
    root[:, 4] = np.where(full, -0.1, 0.0)
    s = np.sqrt(1.0 - root[:, 3] ** 2 - root[:, 4] ** 2)
    root[:, 5], root[:, 6] = qz * s, qw * s
    kindp = (np.arange(N * num_points) % 7).reshape(N, num_points)
    X, Y = rows * hs, cols * hs  # the map's extent in shifted coordinates
    u = lambda: rng.uniform(0, 1, (N, num_points))  # noqa: E731
    tx = np.select([kindp == 2, kindp == 3, kindp == 6], [-3 * hs * u(), X + 3 * hs * u(), -hs * (0.05 + 0.9 * u())],
                   X * u())
    ty = np.select([kindp == 4, kindp == 5, kindp == 6], [-3 * hs * u(), Y + 3 * hs * u(), -hs * (0.05 + 0.9 * u())],
                   Y * u())
    # world target = shifted - border; the probe in the base's yaw frame
    dx, dy = tx - border - root[:, 0:1], ty - border - root[:, 1:2]
    c, sn = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    pts = np.stack([c * dx + sn * dy, -sn * dx + c * dy, rng.uniform(-0.1, 0.1, (N, num_points))], -1)
    return (samples, border, hs, m["vs"], root.astype(np.float32), np.ascontiguousarray(pts, dtype=np.float32), kindp)
