"""The runtime-sized kernel (gs_generic.hip, kernel_variant 4) with convex-hull ground contacts, self-collision of
filter-0 actors and force sensors.

Before, a robot with no compiled topology could have none of the three: gs_sim_set_model / gs_sim_set_self_collision
/ gs_sim_set_force_sensors refused them on variant 4.  Here the compiled robots that use them are forced onto the
runtime-sized kernel (GS_PHYSICS_KERNEL=generic) and checked against the fp64 oracle with the bars of their
compiled-kernel tests (tests/helpers.py assert_close_or_explained, max_env_frac 0.02; the oracle's TGS is solver_type
3), the self-contact pools are compared slot by slot, and hulls built in the test have closed-form answers.
"""
import os

import numpy as np
import pytest
import torch

from oracle.oracle import OracleSim
from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _simulate(kind, n, params, root, dof, tau, mu, nd, steps=1, self_collide=None):
    gym, sim = H.make_gpu_sim(kind, n, params, self_collide=self_collide)
    assert sim.kernel_variant == 4, sim.kernel_variant
    H.load_state_into(sim, root, dof, mu)
    for _ in range(steps):
        sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
        gym.simulate(sim)
    gym.refresh_net_contact_force_tensor(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, nd)
    g_cf = sim.contact_tensor.cpu().numpy().astype(np.float64).reshape(n, -1, 3)
    return gym, sim, g_root, g_dof, g_cf


def _oparams(params, solver_type):
    return dict(params, solver_type=solver_type), dict(params, solver_type=3 if solver_type == 1 else 0)


# ---------------------------------------------------------------- 1. UsefulHound on the runtime-sized kernel
@pytest.mark.gpu
@pytest.mark.parametrize("solver_type", [0, 1])
def test_useful_hound_runs_on_the_runtime_kernel(solver_type, monkeypatch):
    """UsefulHound forced onto the runtime-sized kernel: 512 random states (H.hound_states seed 5, the seed of
    tests/test_hound_gpu.py::test_hound_one_simulate_matches_oracle), self-collision on, one simulate, state and
    per-link contact forces against the fp64 oracle.  253 pairs (4 broadphase rounds, the last partial), the 8-slot
    pool, 112 candidates of which 28 are the 7 arm hulls' slots (1503 hull vertices), flat cylinders, kept
    fixed-joint links, GS_MIN_RESPONSE.

    The 2 % cap on these inputs, checked on the CPU with the host backend (compiled `hound` topology, the same float
    solver source) against the oracle: PGS 3 of 512 envs beyond tolerance, TGS 3 of 512 (cap: 10), none
    unexplained."""
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    n = 512
    art, flat = H.hound()
    assert flat["npair"] == 253 and flat["npool"] == 8 and int((np.asarray(flat["cdyn"]) >= 0).sum()) == 28
    assert len(flat["hverts"]) == 1503 and flat["nc"] == 112
    params, oparams = _oparams(H.HOUND_PARAMS, solver_type)
    root, dof, tau, mu = H.hound_states(n, seed=5)
    gym, sim, g_root, g_dof, g_cf = _simulate("hound", n, params, root, dof, tau, mu, 18)
    assert sim.self_collide
    o_root, o_dof, o_cf, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, nc=24)
    assert np.abs(o_cf).sum() > 0
    # the pairs are in effect: without them the oracle ends elsewhere
    x_root, x_dof, _, _ = H.oracle_run(dict(flat, self_collide=0), oparams, root, dof, tau, mu, 64, nc=24)
    assert np.abs(x_dof[:, :, 1] - o_dof[:, :, 1]).max() > 0.1

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        r, d, c, _ = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, nc=24)
        return H.state_fields(r, d, c)
    H.assert_close_or_explained(H.state_fields(g_root, g_dof, g_cf), H.state_fields(o_root, o_dof, o_cf), rerun,
                                max_env_frac=0.02, what=f"hound runtime-sized kernel vs oracle (solver {solver_type})")


# ---------------------------------------------------------------- 2. self-contact pools
def _pools_match(pools, o_pool, o_cnt, npool, what):
    """Same count per env, the same body pairs in the same slots, nothing beyond npool; separations within 1e-5 m
    and normals within a small angle (the bars of tests/test_host_backend.py::
    test_self_contact_pools_match_oracle_in_float)."""
    g_pool, g_cnt = pools
    assert g_pool.shape[1] == npool and g_cnt.max() <= npool
    np.testing.assert_array_equal(g_cnt, o_cnt, err_msg=what)
    ang, sep = [], []
    for e in range(len(o_cnt)):
        k = o_cnt[e]
        np.testing.assert_array_equal(g_pool[e, :k, 8:10], o_pool[e, :k, 8:10], err_msg=f"{what} env {e}")
        assert not g_pool[e, k:].any(), (what, e)  # no slot written beyond the count
        for j in range(k):
            ang.append(np.degrees(np.arccos(np.clip(np.dot(o_pool[e, j, 3:6], g_pool[e, j, 3:6]), -1.0, 1.0))))
            sep.append(abs(o_pool[e, j, 6] - g_pool[e, j, 6]))
    ang, sep = np.array(ang), np.array(sep)
    H.parity_report(f"{what}: {ang.size} contacts, separation error max {sep.max():.3g}, normal angle q99 "
                    f"{np.quantile(ang, 0.99):.3g} max {ang.max():.3g} deg")
    assert sep.max() <= 1e-5, (what, sep.max())
    assert np.quantile(ang, 0.99) <= 0.1 and ang.max() <= 2.0, (what, np.quantile(ang, 0.99), ang.max())
    return ang.size


def _overflowing(flat, params, root, dof, mu):
    """Envs whose contacts in pair order exceed the pool (the oracle with a 16-slot pool finds them all); the real
    pool must be the first npool of them."""
    npool = int(flat["npool"])
    wide, wcnt = OracleSim(dict(flat, npool=16), params).self_contacts(root, dof, mu)
    pool, cnt = OracleSim(flat, params).self_contacts(root, dof, mu)
    over = np.nonzero(wcnt > npool)[0]
    for e in over:
        assert cnt[e] == npool
        np.testing.assert_array_equal(pool[e], wide[e, :npool])
    return over


@pytest.mark.gpu
def test_runtime_kernel_self_contact_pools_match_oracle(monkeypatch):
    """gs_debug_self_contacts on variant 4 against the oracle's pools: crossed-leg ANYmal states (4 slots; a second
    batch with the wide perturbations that fill the pool, some with more contacts than slots, so that dropping in
    pair order is exercised) and 256 UsefulHound states (8 slots, GJK pairs)."""
    from tests.test_self_collision import crossed_leg_states
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    art, flat = H.anymal()
    a = crossed_leg_states(96)
    b = crossed_leg_states(32, seed=5, min_contacts=4, spread=1.8, pool=200)
    root, dof, mu = (np.concatenate([x[i], y[i]]) for x, y in [(a, b)] for i in (0, 1, 3))
    over = _overflowing(flat, H.ANYMAL_PARAMS, root, dof, mu)
    assert over.size >= 1, "no env whose contacts exceed the pool: pick other states"
    n = root.shape[0]
    gym, sim = H.make_gpu_sim("anymal", n, H.ANYMAL_PARAMS)
    assert sim.kernel_variant == 4
    H.load_state_into(sim, root, dof, mu)
    o_pool, o_cnt = OracleSim(flat, H.ANYMAL_PARAMS).self_contacts(root, dof, mu)
    assert _pools_match(H.sim_self_contacts(sim, 0), o_pool, o_cnt, 4, "anymal runtime-sized pools") > n

    art, flat = H.hound()
    n = 256
    root, dof, _, mu = H.hound_states(n, seed=9)
    gym, sim = H.make_gpu_sim("hound", n, H.HOUND_PARAMS)
    assert sim.kernel_variant == 4
    H.load_state_into(sim, root, dof, mu)
    o_pool, o_cnt = OracleSim(flat, H.HOUND_PARAMS).self_contacts(root, dof, mu)
    assert _pools_match(H.sim_self_contacts(sim, 0), o_pool, o_cnt, 8, "hound runtime-sized pools") > n


# ---------------------------------------------------------------- 3. ANYmal, filter 0
@pytest.mark.gpu
@pytest.mark.parametrize("solver_type", [0, 1])
def test_anymal_self_collision_on_the_runtime_kernel(solver_type, monkeypatch):
    """256 crossed-leg ANYmal states, collision filter 0, one simulate against the oracle (state and contact
    forces)."""
    from tests.test_self_collision import crossed_leg_states
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    n = 256
    art, flat = H.anymal()
    params, oparams = _oparams(H.ANYMAL_PARAMS, solver_type)
    root, dof, tau, mu = crossed_leg_states(n)
    gym, sim, g_root, g_dof, g_cf = _simulate("anymal", n, params, root, dof, tau, mu, 12)
    assert sim.self_collide
    o_root, o_dof, o_cf, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, nc=13)
    x_root, x_dof, _, _ = H.oracle_run(dict(flat, self_collide=0), oparams, root, dof, tau, mu, 64, nc=13)
    assert np.abs(x_dof[:, :, 1] - o_dof[:, :, 1]).max() > 0.1

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        r, d, c, _ = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, nc=13)
        return H.state_fields(r, d, c)
    H.assert_close_or_explained(H.state_fields(g_root, g_dof, g_cf), H.state_fields(o_root, o_dof, o_cf), rerun,
                                max_env_frac=0.02,
                                what=f"anymal filter 0 runtime-sized kernel vs oracle (solver {solver_type})")


@pytest.mark.gpu
def test_runtime_kernel_self_contacts_conserve_momentum_and_push_legs_apart(monkeypatch):
    """The rule of tests/test_self_collision.py::test_self_contacts_conserve_momentum_and_push_legs_apart on variant
    4: zero gravity, no ground, no torque -- the self-contact impulses are internal (the total linear momentum after
    one simulate equals that of the same step without self-collision, to float rounding), and legs pressed into
    each other separate within 200 simulates."""
    from oracle import kinematics_oracle as KO
    from tests.test_self_collision import crossed_leg_states
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    n = 24
    art, flat = H.anymal()
    root, dof, tau, mu = crossed_leg_states(n)
    params = dict(H.ANYMAL_PARAMS, gravity=[0.0, 0.0, 0.0], has_ground=0)
    zero = np.zeros((n, 12))
    c0, k0 = OracleSim(flat, params).self_contacts(root, dof, mu)
    assert (k0 > 0).all() and c0[:, 0, 6].min() < -0.005

    def momentum(r, d):
        r0, d0 = root.copy(), dof.copy()
        r0[:, 7:13] = r[:, 7:13]
        d0[:, :, 1] = d[:, :, 1]
        rb, _, _ = KO.batch(flat, r0, d0)
        return (flat["mass"][None, :, None] * rb[:, 7:10].reshape(n, flat["nr"], 3)).sum(1)

    gym, sim, r_on, d_on, _ = _simulate("anymal", n, params, root, dof, zero, mu, 12)
    _, _, r_off, d_off, _ = _simulate("anymal", n, params, root, dof, zero, mu, 12, self_collide=False)
    p_on, p_off = momentum(r_on, d_on), momentum(r_off, d_off)
    free = (np.abs(d_on[:, :, 1]) < 0.999 * flat["vmax"]).all(1) & (np.abs(d_off[:, :, 1]) < 0.999 * flat["vmax"]).all(1)
    assert free.sum() >= n // 2
    assert np.abs(d_off - d_on).max() > 1e-3  # the pairs are in effect
    # float32 solver: the impulses' response is a Cholesky solve of the nv = 18 mass matrix, backward stable to
    # nv * eps32 * |M| |v| per row; for the momentum rows |M| |v| is at most the robot's mass times the fastest
    # link's speed (the oracle's fp64 check of the same rule uses 1e-9)
    speed = max(np.abs(KO.batch(flat, r, d)[0][:, 7:10]).max() for r, d in ((r_on, d_on), (r_off, d_off)))
    bound = 18 * 2.0 ** -24 * float(np.sum(flat["mass"])) * max(1.0, speed)
    assert np.abs(p_on - p_off)[free].max() <= bound, (np.abs(p_on - p_off)[free].max(), bound)
    for _ in range(200):
        gym.simulate(sim)
    torch.cuda.synchronize()
    c1, k1 = H.sim_self_contacts(sim, 0)
    deepest0 = c0[:, 0, 6]
    deepest1 = np.where(k1 > 0, np.where(np.arange(4)[None] < k1[:, None], c1[:, :, 6], 1.0).min(1), 1.0)
    pressed = deepest0 < -0.005
    assert pressed.sum() >= n // 4
    assert (deepest1[pressed] > deepest0[pressed]).all() and deepest1.min() > -0.01


# ---------------------------------------------------------------- 4. hull known answers
def _write_hull_urdf(tmp_path, points):
    """A free body whose only collision shape is the STL hull of `points`, with a light collision-free tail on a
    hinge (the articulation has one dof)."""
    from scipy.spatial import ConvexHull
    hull = ConvexHull(points)
    rec = np.zeros(len(hull.simplices), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["v"] = points[hull.simplices].astype(np.float32)
    (tmp_path / "blob.stl").write_bytes(b"\0" * 80 + len(rec).to_bytes(4, "little") + rec.tobytes())
    (tmp_path / "blob.urdf").write_text(
        '<robot name="blob"><link name="body"><inertial><mass value="1.0"/>'
        '<inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial>'
        '<collision><geometry><mesh filename="blob.stl"/></geometry></collision></link>'
        '<link name="tail"><inertial><origin xyz="0 0 0.05"/><mass value="0.05"/>'
        '<inertia ixx="1e-4" iyy="1e-4" izz="1e-4" ixy="0" ixz="0" iyz="0"/></inertial></link>'
        '<joint name="hinge" type="revolute"><parent link="body"/><child link="tail"/><origin xyz="0 0 0"/>'
        '<axis xyz="0 1 0"/><limit lower="-3" upper="3" effort="10" velocity="50"/></joint></robot>')


def _hull_sim(tmp_path, points, n, params, mu_ground):
    """(flat, gym, sim) of `n` envs of the hull body, loaded from the URDF: no compiled topology matches it."""
    from isaacgymenv_amd.isaacgym import gymapi
    _write_hull_urdf(tmp_path, points)
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.dt, sp.substeps, sp.up_axis = params["dt"], params["substeps"], gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(*params["gravity"])
    sp.use_gpu_pipeline = sp.physx.use_gpu = True
    sp.physx.num_position_iterations, sp.physx.num_velocity_iterations = params["pos_iters"], params["vel_iters"]
    sp.physx.contact_offset, sp.physx.rest_offset = params["contact_offset"], params["rest_offset"]
    sp.physx.max_depenetration_velocity = params["max_depen_vel"]
    sp.physx.contact_collection = gymapi.ContactCollection(1)
    sp.physx.solver_type = 0
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.static_friction = mu_ground
    gym.add_ground(sim, plane)
    opts = gymapi.AssetOptions()
    opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
    asset = gym.load_asset(sim, str(tmp_path), "blob.urdf", opts)
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 8)
        gym.create_actor(env, asset, gymapi.Transform(), "blob", i, 1, 0)
    gym.prepare_sim(sim)
    assert sim.kernel_variant == 4
    return asset.flat, gym, sim


def _quat_to_mat(q):
    from oracle import kinematics_oracle as KO
    return KO.quat_to_mat(q)


HULL_PARAMS = dict(H.ANYMAL_PARAMS, contact_offset=0.002, ground_friction=0.0)


@pytest.mark.gpu
def test_runtime_kernel_hull_contact_is_the_lowest_vertex(tmp_path):
    """A hull of more than 64 vertices (several vertex rounds) falling at random orientations with its lowest vertex
    1 mm above a frictionless ground and every other vertex beyond contact_offset: the one contact row brings the
    lowest vertex's vertical velocity to -separation / h exactly (PGS, one row), whichever vertex round holds it.
    A wrong vertex, or none, leaves that velocity at the free fall's."""
    rng = np.random.RandomState(0)
    pts = rng.normal(size=(150, 3))
    pts = 0.5 * pts / np.linalg.norm(pts, axis=1, keepdims=True)
    n = 64
    flat, gym, sim = _hull_sim(tmp_path, pts, n, HULL_PARAMS, 0.0)
    hv = np.asarray(flat["hverts"])[:, :3].astype(np.float32).astype(np.float64)
    assert len(hv) > 128 and flat["nd"] == 1
    root = np.zeros((n, 13))
    dof = np.zeros((n, 1, 2))
    lows, k = [], 0
    while k < n:  # orientations whose second-lowest vertex is clear of contact_offset
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        z = (hv @ _quat_to_mat(q).T)[:, 2]
        order = np.argsort(z)
        if z[order[1]] - z[order[0]] < 0.004:
            continue
        root[k, 3:7] = q
        root[k, 2] = 0.001 - z[order[0]]
        lows.append(int(order[0]))
        k += 1
    assert max(lows) >= 128 and min(lows) < 64  # first, middle and last vertex rounds hold a lowest vertex
    root[:, 7:10] = rng.normal(0, 0.3, (n, 3)) + [0.0, 0.0, -3.0]
    root[:, 10:13] = rng.normal(0, 0.5, (n, 3))
    mu = np.zeros((n, flat["ns"]))
    H.load_state_into(sim, root, dof, mu)
    gym.simulate(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 1)
    h = HULL_PARAMS["dt"]
    for e in range(n):
        x = _quat_to_mat(root[e, 3:7]) @ hv[lows[e]]
        vz = g_root[e, 9] + np.cross(g_root[e, 10:13], x)[2]
        free = root[e, 9] - 9.81 * h + np.cross(root[e, 10:13], x)[2]
        assert free < -1.0  # (the vertex approaches far faster than the row allows: the row is what stops it)
        assert abs(vz - (-0.001 / h)) < 2e-3, (e, lows[e], vz)
    o_root, o_dof, _, _ = H.oracle_run(flat, HULL_PARAMS, root, dof, np.zeros((n, 1)), mu, 64)
    np.testing.assert_allclose(g_root[:, 7:], o_root[:, 7:], atol=5e-3, rtol=5e-3)
    np.testing.assert_allclose(g_root[:, :7], o_root[:, :7], atol=2e-5)


@pytest.mark.gpu
def test_runtime_kernel_hull_face_on_ground_contacts_at_its_corners(tmp_path):
    """A box-shaped hull (its mesh has face-interior points too) lying 1 mm inside the ground on a face, its four bottom corners
    at exactly the same height -- an exact tie between the deepest vertices, which the lowest index wins -- and
    rolling about x: the contacts are the face's corners, so the descending corners stop (their vertical velocity
    goes to 0) and the state matches the oracle's, whose row order follows the same tie-break."""
    corners = np.array([[x, y, z] for x in (-0.125, 0.125) for y in (-0.0625, 0.0625) for z in (-0.03125, 0.03125)])
    extra = np.array([[0.0, 0.0, 0.03125], [0.0625, 0.0, -0.03125], [0.0, 0.03125, 0.03125]])
    n = 8
    # (24 velocity iterations: the two descending corners' rows are coupled, one sweep leaves a residual)
    params = dict(H.ANYMAL_PARAMS, ground_friction=0.0, vel_iters=24)
    flat, gym, sim = _hull_sim(tmp_path, np.concatenate([corners, extra]), n, params, 0.0)
    hv = np.asarray(flat["hverts"])[:, :3]
    bottom = [i for i in range(len(hv)) if hv[i, 2] < 0 and abs(abs(hv[i, 0]) - 0.125) < 1e-9 and
              abs(abs(hv[i, 1]) - 0.0625) < 1e-9]
    assert len(bottom) == 4 and len({float(np.float32(hv[i, 2])) for i in bottom}) == 1
    o = OracleSim(flat, params)
    sel = o.hull_select(0, np.eye(3), np.zeros(3), rootz=0.03125 - 0.001)
    assert sorted(sel.tolist()) == sorted(bottom) and sel[0] == min(bottom)
    root = np.zeros((n, 13))
    root[:, 2] = 0.03125 - 0.001
    root[:, 6] = 1.0
    root[:, 10] = np.linspace(0.5, 2.0, n) * np.where(np.arange(n) % 2, 1.0, -1.0)
    dof = np.zeros((n, 1, 2))
    mu = np.zeros((n, flat["ns"]))
    H.load_state_into(sim, root, dof, mu)
    gym.simulate(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 1)
    for e in range(n):
        vz = np.array([g_root[e, 9] + np.cross(g_root[e, 10:13], hv[i])[2] for i in bottom])
        down = np.array([np.cross(root[e, 10:13], hv[i])[2] for i in bottom]) < 0
        assert down.sum() == 2 and np.abs(vz[down]).max() < 2e-3 and vz.min() > -2e-3, (e, vz)
    o_root, o_dof, _, _ = H.oracle_run(flat, params, root, dof, np.zeros((n, 1)), mu, 64)
    np.testing.assert_allclose(g_root[:, 7:], o_root[:, 7:], atol=5e-3, rtol=5e-3)
    np.testing.assert_allclose(g_root[:, :7], o_root[:, :7], atol=2e-5)


@pytest.mark.gpu
def test_runtime_kernel_replays_the_cylinder_ground_case(monkeypatch):
    """tests/golden/hound_cylinder_ground_case.npz (a leg cylinder's end near the ground under a spinning robot, arm
    hulls and self-collision present) on variant 4, at the bars of
    tests/test_host_backend.py::test_cylinder_end_near_ground_is_not_skipped."""
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    z = np.load(os.path.join(GOLDEN, "hound_cylinder_ground_case.npz"))
    root, dof, mu, tau = z["root"], z["dof"], z["mu"], z["tau"]
    art, flat = H.hound()
    for params in (H.HOUND_PARAMS, dict(H.HOUND_PARAMS, pos_iters=1, vel_iters=0)):
        _, sim, g_root, g_dof, _ = _simulate("hound", 1, params, root, dof, tau, mu, 18)
        o_root, o_dof, _, _ = H.oracle_run(flat, params, root, dof, tau, mu, nc=24)
        np.testing.assert_allclose(g_dof[:, :, 0], o_dof[:, :, 0], atol=2e-6)
        np.testing.assert_allclose(g_dof[:, :, 1], o_dof[:, :, 1], atol=5e-4, rtol=1e-4)
        np.testing.assert_allclose(g_root[:, 7:], o_root[:, 7:], atol=5e-4, rtol=1e-4)


# ---------------------------------------------------------------- 5. force sensors
def _ant(n, root, dof, tau, mu, steps):
    gym, sim = H.make_gpu_sim("ant", n, H.ANT_PARAMS)
    assert sim.kernel_variant == 4 and sim.num_sensors == 4
    H.load_state_into(sim, root, dof, mu)
    for _ in range(steps):
        sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
        gym.simulate(sim)
    gym.refresh_force_sensor_tensor(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 8)
    assert tuple(sim.sensor_tensor.shape) == (n * 4, 6)
    return g_root, g_dof, sim.sensor_tensor.cpu().numpy().astype(np.float64).reshape(n, 4, 6)


@pytest.mark.gpu
def test_ant_force_sensors_on_the_runtime_kernel(monkeypatch):
    """Ant forced onto the runtime-sized kernel, 256 random states with joint limits active (dofs up to 0.05 rad
    beyond them): state and the [N * 4, 6] sensor tensor after one simulate against the oracle, at the bars of
    tests/test_ant_physics_gpu.py::test_ant_one_simulate_matches_oracle."""
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    n = 256
    art, flat = H.ant()
    root, dof, tau, mu = H.ant_states(n, seed=3)
    assert ((dof[:, :, 0] < flat["lower"]) | (dof[:, :, 0] > flat["upper"])).any()
    g_root, g_dof, g_sens = _ant(n, root, dof, tau, mu, 1)
    o_root, o_dof, _, o_sens = H.oracle_run(flat, H.ANT_PARAMS, root, dof, tau, mu, 64, nsens=4,
                                            sensor_bodies=H.ANT_FEET)
    assert np.abs(o_sens).max() > 1.0

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        o_r, o_d, _, o_s = H.oracle_run(flat, H.ANT_PARAMS, r, d, tau[idx], mu[idx], bits, nsens=4,
                                        sensor_bodies=H.ANT_FEET)
        return H.state_fields(o_r, o_d, sens=o_s)
    H.assert_close_or_explained(H.state_fields(g_root, g_dof, sens=g_sens), H.state_fields(o_root, o_dof, sens=o_sens),
                                rerun, max_env_frac=0.02, what="ant runtime-sized kernel, state and sensors")


@pytest.mark.gpu
def test_ant_force_sensors_rollout_on_the_runtime_kernel(monkeypatch):
    """20 simulates at zero torque from the reference's start pose: trajectory and foot sensors follow the oracle's,
    at the bars of tests/test_ant_physics_gpu.py::test_ant_rest_rollout_tracks_oracle."""
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    n, steps = 32, 20
    art, flat = H.ant()
    root = np.zeros((n, 13)); root[:, 2] = 0.44; root[:, 6] = 1.0
    dof = np.zeros((n, 8, 2)); dof[:, :, 0] = np.clip(0.0, flat["lower"], flat["upper"])
    tau = np.zeros((n, 8))
    mu = np.full((n, flat["ns"]), 1.5)
    g_root, g_dof, g_sens = _ant(n, root, dof, tau, mu, steps)
    o_root, o_dof, _, o_sens = H.oracle_run(flat, H.ANT_PARAMS, root, dof, tau, mu, 64, steps, nsens=4,
                                            sensor_bodies=H.ANT_FEET)
    np.testing.assert_allclose(g_root[:, 0:3], o_root[:, 0:3], atol=2e-3)
    np.testing.assert_allclose(g_dof[:, :, 0], o_dof[:, :, 0], atol=2e-3)
    np.testing.assert_allclose(g_sens, o_sens, atol=0.05, rtol=2e-2)
