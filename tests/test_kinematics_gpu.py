"""The link-kinematics kernel (gs_kinematics.hip, k_kinematics) at the C ABI against the float64 oracle, on every shipped
asset: Cartpole, ANYmal, Ant, Hound, Hound_new, the arm and Franka fixtures, and the Humanoid's mass matrix.

Cases, bars and conditions: tests/kinematics_cases.py (pinned on the CPU by tests/test_kinematics_cpu.py).  Every call
goes through gs_sim_refresh_rigid_body / _jacobian / _mass_matrix on sim.handle into a buffer of the test's own that
lies inside a larger allocation of 0xA5 bytes -- 64 before it, and after it 64 plus the size of three envs, where the
idle waves of a tail block would write if the kernel let them.

* parity at N = 1, 3 (one partial block), 5 (a full block and a tail block with three idle waves) and 130 (33 blocks,
  26 envs of each kind: upright, tumbled, dofs over their whole ranges, dofs on their bounds, at rest): every offered
  tensor at the bars, the full [N, nr, 6, nv] Jacobian with the root row; unit quaternions, w >= 0 on the links, the
  root's quaternion bit for bit, exact zeros at rest;
* each entry point writes its own tensor and nothing else, twice the same bits;
* the fast sine at the largest angles the assets allow: Cartpole's pole over [-2 pi, 2 pi] against the analytic row,
  Hound_new and the Franka with every dof at +-lower and +-upper;
* the tensors follow a simulate on the same stream;
* what Houndarm, Manipulator and UsefulHound read on the real simulator equals the oracle's slice found by link name;
* refusals: the per-link tensors of an asset with hidden links, an unprepared sim, a null output.

Report lines (H.parity_report): kernel error / bar and float32-oracle error / bar per asset and field, the Shepperd
branch counts of the compared links, the worst sweep error by |theta|, the file's wall time.
"""
import os
import time

import numpy as np
import pytest
import torch

from oracle import kinematics_oracle as KO
from tests import arm_cases as A
from tests import helpers as H
from tests import kinematics_cases as KC
from tests import manip_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = {}  # (asset, field) -> (kernel error / bar, float32 oracle error / bar), the largest over the sizes


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for (asset, field), (r, r32) in sorted(SEEN.items()):
        H.parity_report(f"[kinematics] {asset} {field}: kernel error / bar {r:.3f}, float32 oracle error / bar {r32:.3f}")
    H.parity_report(f"[kinematics] tests/test_kinematics_gpu.py wall time {time.perf_counter() - t0:.1f} s")


def _sync():
    torch.cuda.synchronize()


def _stream(sim):
    return sim.stream()


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("n", KC.SIZES)
@pytest.mark.parametrize("asset", tuple(KC.ASSETS))
def test_parity_with_the_float64_oracle(asset, n):
    gym, sim = KC.ASSETS[asset].gpu_sim(n)
    ratios, ratios32 = KC.check_parity(asset, sim, n, DEV, _stream(sim), _sync)
    for f, r in ratios.items():
        old = SEEN.get((asset, f), (0.0, 0.0))
        SEEN[(asset, f)] = (max(old[0], r), max(old[1], ratios32[f]))
    assert max(ratios32.values()) <= 0.5, ratios32
    if n == KC.NMAX and "rb" in KC.ASSETS[asset].offered:
        H.parity_report(f"[kinematics] {asset}: Shepperd branches of the compared link rotations (trace, x, y, z) "
                        f"{KC.branch_counts(asset).tolist()}")


# ---------------------------------------------------------------- one tensor per call, the same bits twice
@pytest.mark.parametrize("asset", ("hound", "franka", "humanoid"))
def test_each_entry_point_writes_its_own_tensor_only(asset):
    n = 5
    a = KC.ASSETS[asset]
    gym, sim = a.gpu_sim(n)
    root, dof = KC.states(asset, n)
    KC.load(sim, root, dof)
    g = KC.Guarded(asset, n, DEV)
    # the C entry points take any of the three tensors, whatever the Python API offers for the asset
    for name in ("rb", "jac", "mm"):
        before = {k: g.bytes(k) for k in ("rb", "jac", "mm")}
        assert KC.refresh(sim, name, g.ptr(name), _stream(sim)) == 0, KC.last_error()
        _sync()
        for k in ("rb", "jac", "mm"):
            if k != name:
                assert np.array_equal(g.bytes(k), before[k]), f"{KC.ENTRY[name]} changed the {k} buffer"
        assert g.guards_intact(name) and not np.array_equal(g.bytes(name), before[name])
        assert g.unwritten(name) == 0 and np.isfinite(g.numpy(name)).all()
    first = {k: g.bytes(k) for k in ("rb", "jac", "mm")}
    for name in ("rb", "jac", "mm"):
        assert KC.refresh(sim, name, g.ptr(name), _stream(sim)) == 0
    _sync()
    for k in ("rb", "jac", "mm"):
        assert np.array_equal(g.bytes(k), first[k]), f"{k}: a second call on the same state changed bits"


# ---------------------------------------------------------------- the fast sine at the largest angles
def test_cartpole_pole_sweep_known_answer():
    gym, sim = KC.ASSETS["cartpole"].gpu_sim(KC.SWEEP_ANGLES)
    worst, at = KC.check_sweep_known_answer(sim, DEV, _stream(sim), _sync)
    H.parity_report(f"[kinematics] cartpole pole sweep over +-2 pi against the analytic row: worst error / bar "
                    f"{worst:.3f} at |theta| = {at:.3f}")


@pytest.mark.parametrize("asset", ("hound_new", "franka"))
def test_every_dof_at_its_bounds_in_both_signs(asset):
    a = KC.ASSETS[asset]
    flat = a.model()[1]
    root, dof = KC.bound_sweep(asset)
    n = root.shape[0]
    assert n == 4 * flat["nd"]
    top = float(np.abs(dof[:, :, 0]).max())
    assert top > (6.28 if asset == "hound_new" else 3.75)
    gym, sim = a.gpu_sim(n)
    KC.load(sim, root, dof)
    g = KC.run_all(asset, sim, n, DEV, _stream(sim))
    _sync()
    rb, jac, mm = KC.outputs(asset, g)
    o_rb, o_jac, o_mm = KO.batch(flat, root, dof)
    ref = (o_rb.reshape(n, flat["nr"], 13), o_jac, o_mm)
    swept = np.abs(dof[:, :, 0]).max(axis=1)
    per_env = np.array([max(KC.field_ratios(asset, rb[e:e + 1], jac[e:e + 1], mm[e:e + 1],
                                            tuple(x[e:e + 1] for x in ref)).values()) for e in range(n)])
    worst = int(np.argmax(per_env))
    H.parity_report(f"[kinematics] {asset} every dof at +-lower, +-upper (|theta| up to {top:.3f}): worst error / bar "
                    f"{per_env[worst]:.3f} at |theta| = {swept[worst]:.3f}")
    assert per_env.max() <= 1.0, (per_env[worst], swept[worst])


# ---------------------------------------------------------------- freshness
@pytest.mark.parametrize("asset", ("hound", "arm"))
def test_tensors_follow_a_simulate_on_the_same_stream(asset):
    n = 5
    a = KC.ASSETS[asset]
    flat = a.model()[1]
    gym, sim = a.gpu_sim(n)
    root, dof = KC.states(asset, n)
    KC.load(sim, root, dof)
    gym.simulate(sim)
    g = KC.run_all(asset, sim, n, DEV, _stream(sim))  # no synchronize in between: stream order alone
    _sync()
    after_root, after_dof = H.read_state(sim, flat["nd"])
    assert np.abs(after_dof[:, :, 0] - dof[:, :, 0]).max() > 1e-3, "the simulate must move the joints"
    rb, jac, mm = KC.outputs(asset, g)

    def ratios(r, d):
        o_rb, o_jac, o_mm = KO.batch(flat, r, d)
        return KC.field_ratios(asset, rb, jac, mm, (o_rb.reshape(n, flat["nr"], 13), o_jac, o_mm))

    fresh, stale = ratios(after_root, after_dof), ratios(np.asarray(root), np.asarray(dof))
    assert max(fresh.values()) <= 1.0, fresh
    assert stale["pos"] > 10.0 and stale["jac"] > 10.0, stale  # and not the state before the simulate


# ---------------------------------------------------------------- what the tasks read
def _child_link_of(art, joint):
    """Index of the link that `joint` connects to its parent, by name."""
    return next(i for i, l in enumerate(art.link_table()) if l.joint_name == joint)


def _set_through_the_tensor_api(env, root, dof):
    """Root (floating bases) and dof states through the gym tensor API."""
    from isaacgymenv_amd.isaacgym import gymtorch
    gym, sim = env.gym, env.sim
    dof_t = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    dof_t.view(dof.shape).copy_(torch.from_numpy(np.asarray(dof, dtype=np.float32)))
    gym.set_dof_state_tensor(sim, gymtorch.unwrap_tensor(dof_t))
    if root is not None:
        root_t = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
        root_t.view(root.shape).copy_(torch.from_numpy(np.asarray(root, dtype=np.float32)))
        gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(root_t))


def _kind_states(asset, kinds, n):
    kind = KC.kinds_of(asset, KC.NMAX)
    idx = np.nonzero(np.isin(kind, kinds))[0][:n]
    root, dof = KC.states(asset, KC.NMAX)
    return root[idx], dof[idx]


def _oracle_of_the_sim(sim, flat, n):
    """The float64 oracle on the state the sim holds now."""
    root, dof = H.read_state(sim, flat["nd"])
    o_rb, o_jac, o_mm = KO.batch(flat, root, dof)
    return root, dof, o_rb.reshape(n, flat["nr"], 13), o_jac, o_mm


def _fixed_base_task_reads(env, asset, joint, nd):
    n = env.num_envs
    art, flat = KC.ASSETS[asset].model()
    _, dof = _kind_states(asset, ("limits",), n)
    _set_through_the_tensor_api(env, None, dof)
    env._refresh()
    _sync()
    root, got_dof, o_rb, o_jac, o_mm = _oracle_of_the_sim(env.sim, flat, n)
    assert np.array_equal(got_dof, np.asarray(dof)), "the sim holds the dof state that was set"
    link = _child_link_of(art, joint)
    assert art.link_names()[link] == env.eef_link_name
    j = env.j_eef.cpu().numpy().astype(np.float64)
    m = env.mm.cpu().numpy().astype(np.float64)
    e = env.eef_state.cpu().numpy().astype(np.float64)
    assert j.shape == (n, 6, nd) and m.shape == (n, nd, nd) and e.shape == (n, 13)
    out = {"j_eef": KC.ratio(j, o_jac[:, link], KC.BAR_POS), "mm": KC.mm_ratio(asset, m, o_mm),
           "eef pos": KC.ratio(e[:, 0:3], o_rb[:, link, 0:3], KC.BAR_POS),
           "eef quat": KC.quat_ratio(e[:, 3:7], o_rb[:, link, 3:7]),
           "eef vel": KC.ratio(e[:, 7:13], o_rb[:, link, 7:13], KC.BAR_VEL)}
    assert max(out.values()) <= 1.0, out
    # and no other link's row would do: the neighbouring rows lie far outside the bar
    for other in (link - 1,):
        assert KC.ratio(j, o_jac[:, other], KC.BAR_POS) > 10.0
    return out


def test_houndarm_reads_the_end_links_slices(monkeypatch):
    from tests.test_houndarm_gpu import _gpu_env
    env = _gpu_env(np.load(os.path.join(A.GOLDEN, "houndarm.npz")), 5, monkeypatch)
    out = _fixed_base_task_reads(env, "arm", "joint6", 6)
    H.parity_report("[kinematics] Houndarm j_eef / mm / eef_state against the oracle's end_link: " +
                    ", ".join(f"{k} {v:.3f}" for k, v in out.items()))


def test_manipulator_reads_the_last_links_slices(monkeypatch):
    from tests.test_manipulator_gpu import _gpu_env
    env = _gpu_env(np.load(os.path.join(M.GOLDEN, "manipulator.npz")), 5, monkeypatch)
    out = _fixed_base_task_reads(env, "franka", "panda_joint7", 7)
    H.parity_report("[kinematics] Manipulator j_eef / mm / eef_state against the oracle's panda_link7: " +
                    ", ".join(f"{k} {v:.3f}" for k, v in out.items()))


def test_useful_hound_reads_its_slices(monkeypatch):
    """UsefulHound's OSC inputs on tumbled bases with the dofs over their whole ranges.  The reference's quirks are
    kept: its Jacobian slice takes the six BASE columns, and on a floating base the tensor keeps
    the root row, so the index of joint6 selects the row of joint6's parent link (link6), not of end_link; the
    end-effector state is end_link's, which the task acquires and never refreshes."""
    from tests.test_hound_gpu import _make
    n = 5
    env = _make(n, monkeypatch)
    art, flat = KC.ASSETS["hound"].model()
    root, dof = _kind_states("hound", ("tumbled",), n)
    api_root = np.asarray(root).copy()  # the API's root velocity is the root link COM's: only poses matter to the set
    _set_through_the_tensor_api(env, api_root, dof)
    gym, sim = env.gym, env.sim
    gym.refresh_jacobian_tensors(sim)      # the task's own refreshes (post_physics_step) ...
    gym.refresh_mass_matrix_tensors(sim)
    gym.refresh_rigid_body_state_tensor(sim)  # ... and the one it never makes
    _sync()
    got_root, got_dof, o_rb, o_jac, o_mm = _oracle_of_the_sim(sim, flat, n)
    assert np.array_equal(got_dof, np.asarray(dof)) and np.array_equal(got_root[:, 0:3], np.asarray(root)[:, 0:3])
    np.testing.assert_allclose(got_root[:, 3:7], np.asarray(root)[:, 3:7], atol=3e-7)  # (the set normalises it)
    assert (got_root[:, 6] < 0).any(), "a root quaternion with w < 0 among the tumbled envs"
    names = art.link_names()
    child = _child_link_of(art, "joint6")
    assert names[child] == "end_link" and env.eef_index == child
    parent = art.link_table()[child].parent
    parent = names.index(parent) if isinstance(parent, str) else int(parent)
    assert names[parent] == "link6"
    j = env._j_eef.cpu().numpy().astype(np.float64)
    m = env._mm.cpu().numpy().astype(np.float64)
    e = env._eef_state.cpu().numpy().astype(np.float64)
    d = np.sqrt(np.einsum("nii->ni", o_mm))[:, -6:]
    out = {"_j_eef": KC.ratio(j, o_jac[:, parent, :, :6], KC.BAR_POS),
           "_mm": float((np.abs(m - o_mm[:, -6:, -6:]) / (KC.M_BAR * d[:, :, None] * d[:, None, :])).max()),
           "_eef pos": KC.ratio(e[:, 0:3], o_rb[:, child, 0:3], KC.BAR_POS),
           "_eef quat": KC.quat_ratio(e[:, 3:7], o_rb[:, child, 3:7]),
           "_eef vel": KC.ratio(e[:, 7:13], o_rb[:, child, 7:13], KC.BAR_VEL)}
    assert max(out.values()) <= 1.0, out
    assert KC.ratio(j, o_jac[:, child, :, :6], KC.BAR_POS) > 10.0  # (the child's row is a different one)
    H.parity_report("[kinematics] UsefulHound _j_eef (link6, base columns) / _mm / _eef_state (end_link): " +
                    ", ".join(f"{k} {v:.3f}" for k, v in out.items()))


# ---------------------------------------------------------------- refusals
def test_hidden_links_refuse_the_per_link_tensors():
    gym, sim = KC.ASSETS["humanoid"].gpu_sim(2)
    for call in (lambda: gym.acquire_rigid_body_state_tensor(sim), lambda: gym.acquire_jacobian_tensor(sim, "humanoid"),
                 lambda: gym.acquire_net_contact_force_tensor(sim)):
        with pytest.raises(NotImplementedError, match="9 hidden links"):
            call()
    mm = gym.acquire_mass_matrix_tensor(sim, "humanoid")
    assert tuple(mm.tensor.shape) == (2, 27, 27)


def test_entry_points_refuse_an_unprepared_sim_and_a_null_output():
    from isaacgymenv_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.use_gpu_pipeline = True
    sp.physx.use_gpu = True
    bare = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    assert bare is not None and bare.handle and not bare.prepared
    g = KC.Guarded("cartpole", 2, DEV)
    for name, entry in KC.ENTRY.items():
        assert KC.refresh(bare, name, g.ptr(name), None) != 0
        assert entry in KC.last_error() and "not prepared" in KC.last_error()
    _, sim = KC.ASSETS["cartpole"].gpu_sim(2)
    for name, entry in KC.ENTRY.items():
        assert KC.refresh(sim, name, None, _stream(sim)) != 0
        assert entry in KC.last_error() and "null output" in KC.last_error()
    _sync()
    for name in KC.ENTRY:
        assert g.untouched(name)
