"""Manipulator (tasks/manipulator.py), the loader rules it needs, and libgymtask's new entry points, CPU side.

The torch path of the task, driven by tests/manip_cases.ManipFakeGym, against a recording of the reference's own
tasks/manipulator.py on the same fake (tests/golden/make_golden_manipulator.py): reset, progress, time-outs and the
generator state are identical, observations, rewards, commands and the dof state agree at rtol 1e-5 / atol 2e-6.  The
two config files against the reference's parsed values; the refusals.  The loader on files written here: a URDF that
goes on after its root element, Wavefront .obj collision meshes, mass properties from collision geometry; the packed
models keep the masses they had.  The packed Franka.  The oracle's own float32 run stays inside the cap the GPU physics
test uses.  The ctypes mirrors against the header, and the entry points' parameter checks.
"""
import copy
import ctypes
import glob
import json
import os
import shutil
import subprocess
import warnings
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch
import yaml

from isaacgymenv_amd.isaacgym import _assets, gymapi
from tests import helpers as H
from tests import manip_cases as M
from tests.test_hound_terrain_cpu import _resolved_leaves, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "isaacgymenv_amd", "isaacgymenvs", "cfg")


def _fixture():
    return np.load(os.path.join(M.GOLDEN, "manipulator.npz"))


def _cfg(d):
    return M.point_at_fixture(yaml.safe_load(str(d["cfg_yaml"])))


def make_on_fake(monkeypatch, cfg=None):
    """(env, fixture): the task built on the fake from the fixture's config, at the fixture's seed."""
    from isaacgymenv_amd.isaacgymenvs.tasks import manipulator
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    d = _fixture()
    fake = M.ManipFakeGym(seed=M.FAKE_SEED)
    monkeypatch.setattr(gymapi, "acquire_gym", lambda: fake)
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        env = manipulator.Manipulator(copy.deepcopy(cfg or _cfg(d)), "cpu", "cpu", -1, True, False, False)
    return env, d


# ---------------------------------------------------------------- the task against the recording
def test_torch_path_matches_the_reference(monkeypatch):
    env, d = make_on_fake(monkeypatch)
    print(M.assert_fixture_conditions(d))
    tol = dict(rtol=1e-5, atol=2e-6)
    assert env.num_obs == 10 and env.num_actions == 6 and env._kernels is None and env.num_dofs == 7
    assert env.eef_index == int(d["eef_index"]) == 7 and env.hand_joint_index == 6
    assert env.max_episode_length == int(d["max_episode_length"]) == 12
    np.testing.assert_array_equal(env.dof_lower_limits.numpy(), d["dof_lower"])
    np.testing.assert_array_equal(env.dof_upper_limits.numpy(), d["dof_upper"])
    np.testing.assert_array_equal(env.effort_limits.numpy(), d["effort_limits"])
    np.testing.assert_array_equal(env.kd.numpy(), d["kd"])
    np.testing.assert_array_equal(env.kd_null.numpy(), d["kd_null"])
    assert env.kp_null.shape == (7,) and env.j_eef.shape[1:] == (6, 7) and env.mm.shape[1:] == (7, 7)
    # the reference asks for the gripper's bodies, which the truncated URDF does not hold, and never uses them
    assert env.gym.find_actor_rigid_body_handle(env.envs[0], 0, "panda_hand") == -1
    M.stagger(env)
    np.testing.assert_array_equal(env.commands.numpy(), d["init_commands"])  # (draw order of the initial reset)
    np.testing.assert_array_equal(env.dof_state.view(-1, 7, 2).numpy(), d["init_dof_state"])
    np.testing.assert_array_equal(env.reset_buf.numpy(), d["init_reset"])
    np.testing.assert_array_equal(env.progress_buf.numpy(), d["init_progress"])
    n = env.num_envs
    worst = used = 0.0
    for t in range(d["actions"].shape[0]):
        M.place_commands(env)
        np.testing.assert_array_equal(env.j_eef.numpy(), d["ctl_jac"][t], err_msg=f"control inputs step {t}")
        np.testing.assert_array_equal(env.mm.numpy(), d["ctl_mm"][t], err_msg=f"control inputs step {t}")
        np.testing.assert_allclose(env.dof_state.view(n, 7, 2).numpy(), d["ctl_dof"][t], err_msg=f"dof state in {t}",
                                   **tol)
        obs, rew, reset, extras = env.step(torch.from_numpy(d["actions"][t]))
        assert reset.dtype == torch.int64
        np.testing.assert_array_equal(reset.numpy(), d["reset"][t], err_msg=f"reset step {t}")
        np.testing.assert_array_equal(extras["time_outs"].numpy().astype(np.int64), d["time_outs"][t])
        np.testing.assert_array_equal(env.progress_buf.numpy(), d["progress"][t], err_msg=f"progress step {t}")
        flagged = d["in_reset"][t] != 0
        # a reset writes the same draws: identical there; elsewhere the fake integrates the float32 torques
        np.testing.assert_array_equal(env.dof_state.view(n, 7, 2).numpy()[flagged], d["dof_state"][t][flagged],
                                      err_msg=f"reset dof state step {t}")
        dof_now = env.dof_state.view(n, 7, 2).numpy()
        used = max(used, float((np.abs(dof_now - d["dof_state"][t]) / (2e-6 + 1e-5 * np.abs(d["dof_state"][t]))).max()))
        np.testing.assert_allclose(env.commands.numpy(), d["commands"][t], err_msg=f"commands step {t}", **tol)
        np.testing.assert_allclose(env.dof_state.view(n, 7, 2).numpy(), d["dof_state"][t], err_msg=f"dof step {t}",
                                   **tol)
        np.testing.assert_allclose(obs["obs"].numpy(), d["obs"][t], err_msg=f"obs step {t}", **tol)
        np.testing.assert_allclose(rew.numpy(), d["rew"][t], err_msg=f"reward step {t}", **tol)
        got = env.sim.force.view(n, 7).numpy()[~flagged]
        worst = max(worst, float(np.abs(got - d["torques"][t][~flagged]).max()))
    np.testing.assert_array_equal(torch.get_rng_state().numpy(), d["final_rng_state"])
    # (another LAPACK build rounds the float32 inverses differently, and the fake integrates the torques)
    print(f"largest torque difference to the recording: {worst:.3g}; the dof state uses {used:.3g} of its tolerance")


def test_generator_state_before_each_reset_matches(monkeypatch):
    """The same torch draws from the same generator state: the state before every post_physics_step."""
    env, d = make_on_fake(monkeypatch)
    M.stagger(env)
    for t in range(d["actions"].shape[0]):
        M.place_commands(env)
        env.pre_physics_step(torch.clamp(torch.from_numpy(d["actions"][t]), -1.0, 1.0))
        env.gym.simulate(env.sim)
        np.testing.assert_array_equal(torch.get_rng_state().numpy(), d["in_rng_state"][t], err_msg=f"step {t}")
        np.testing.assert_array_equal(env.reset_buf.numpy(), d["in_reset"][t])
        env.post_physics_step()


def test_restatement_is_stored_and_its_two_algorithms_agree():
    """The GPU test's reference is what the generator computed, and the bound it is held to is attainable: a LAPACK
    inverse and a Gauss-Jordan elimination give the same float64 torques to 1e-8 max(1, |ref|) on the recorded inputs,
    four orders inside the kernel's 1e-4."""
    d = _fixture()
    again = np.stack([M.restatement(d, t) for t in range(d["torques"].shape[0])])
    np.testing.assert_allclose(again, d["torques64"], rtol=1e-12, atol=1e-12)
    gap = M.algorithm_gap(d)
    print(f"restatement, LAPACK vs Gauss-Jordan: {gap:.3g} max(1, |ref|)")
    assert gap <= M.ALGORITHM_BOUND
    a = np.random.RandomState(0).normal(size=(5, 7, 7)) + 3 * np.eye(7)
    np.testing.assert_allclose(M.gauss_jordan_inverse(a) @ a, np.broadcast_to(np.eye(7), a.shape), atol=1e-12)
    err = np.abs(d["torques"] - d["torques64"]) / np.maximum(1.0, np.abs(d["torques64"]))
    assert np.median(err) < 1e-4, np.median(err)


def test_posture_term_acts_in_the_null_space():
    """With 7 dofs the projector 1 - J^T M_eef J M^-1 is not zero: in float64 a posture error changes the torques and
    leaves J M^-1 u where it was."""
    d = _fixture()
    big = np.full(7, 1e30)
    args = (d["ctl_actions"][0], d["ctl_jac"][0], d["ctl_mm"][0], d["ctl_eef"][0], d["ctl_dof"][0], big)
    u0 = M.osc_float64(*args)
    u1 = M.osc_float64(*args, default=np.asarray(M.DEFAULT_POSE) + 0.3)
    J, Mm = d["ctl_jac"][0].astype(np.float64), d["ctl_mm"][0].astype(np.float64)
    acc = lambda u: (J @ np.linalg.inv(Mm) @ u[..., None])[..., 0]  # noqa: E731
    assert np.abs(u1 - u0).max() > 1.0
    np.testing.assert_allclose(acc(u1), acc(u0), rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------- configs, registry, refusals
def test_config_values_match_the_reference():
    with open(os.path.join(M.GOLDEN, "manipulator_cfg.json")) as f:
        ref = json.load(f)
    with open(os.path.join(CFG, "task", "Manipulator.yaml")) as f:
        _same(yaml.safe_load(f), ref["task"], "task")
    with open(os.path.join(CFG, "train", "ManipulatorPPO.yaml")) as f:
        _same(yaml.safe_load(f), ref["train"], "train")
    from isaacgymenv_amd.isaacgymenvs.config import compose
    c = compose("config", ["task=Manipulator", "num_envs=64", "sim_device=cuda:0"])
    _resolved_leaves(c["task"], ref["task"], "task")
    _resolved_leaves(c["train"], ref["train"], "train")
    t = c["task"]
    assert t["name"] == "Manipulator" and t["env"]["numEnvs"] == 64 and t["sim"]["use_gpu_pipeline"] is True
    assert t["env"]["episodeLength"] == 1000 and t["env"]["frankaDofNoise"] == 0.25
    assert t["env"]["randomCommandPositionRanges"] == {"x": [-0.5, 0.5], "y": [-0.5, 0.5], "z": [0.2, 0.6]}
    assert c["train"]["params"]["config"]["name"] == "Manipulator"
    assert c["train"]["params"]["config"]["num_actors"] == 64
    assert compose("config", ["task=Manipulator"])["task"]["env"]["numEnvs"] == 8192


def test_task_is_registered():
    from isaacgymenv_amd.isaacgymenvs.tasks import isaacgym_task_map
    from isaacgymenv_amd.isaacgymenvs.tasks.manipulator import Manipulator
    assert isaacgym_task_map["Manipulator"] is Manipulator


def test_missing_asset_names_the_two_config_keys(monkeypatch, tmp_path):
    cfg = _cfg(_fixture())
    cfg["env"]["asset"] = {"assetRoot": str(tmp_path), "assetFileNameFranka": "nothing_here.urdf"}
    with pytest.raises(FileNotFoundError) as e:
        make_on_fake(monkeypatch, cfg)
    assert "env.asset.assetRoot" in str(e.value) and "env.asset.assetFileNameFranka" in str(e.value)


def test_joint_tor_and_randomize_are_refused(monkeypatch):
    d = _fixture()
    cfg = _cfg(d)
    cfg["env"]["controlType"] = "joint_tor"
    with pytest.raises(NotImplementedError, match="Manipulator controlType joint_tor"):
        make_on_fake(monkeypatch, cfg)
    cfg = _cfg(d)
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="randomi"):
        make_on_fake(monkeypatch, cfg)


def test_manipulator_on_the_cpu_is_refused_with_the_runtime_kernel_message(monkeypatch):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        with pytest.raises(RuntimeError, match="runtime-sized kernel is a GPU kernel"):
            isaacgymenvs.make(seed=0, task="Manipulator", num_envs=4, sim_device="cpu", rl_device="cpu", headless=True,
                              force_render=False,
                              overrides=["pipeline=cpu", f"task.env.asset.assetRoot={M.GOLDEN}",
                                         f"task.env.asset.assetFileNameFranka={M.MANIP_MODEL}"])


# ---------------------------------------------------------------- the loader, on files written here
CUBE = [(x, y, z) for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]
TETRA = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]


def _write_obj(path, vertices, extra=True):
    lines = ["# a comment", "o thing"] if extra else []
    lines += [f"v {x} {y} {z}" for x, y, z in vertices]
    if extra:  # record types the reader ignores, 'vn' and 'vt' among them
        lines += ["vn 0 0 1", "vt 0.5 0.5", "f 1 2 3", "s off", "usemtl none"]
    path.write_text("\n".join(lines) + "\n")


def _urdf(collision="", inertial="", tail=""):
    return f"""<?xml version="1.0"?>
<robot name="thing">
  <link name="base"/>
  <link name="part">{inertial}{collision}</link>
  <joint name="hinge" type="revolute">
    <parent link="base"/><child link="part"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" effort="10" velocity="5"/>
  </joint>
</robot>{tail}"""


def _mesh(name, scale=None):
    s = f' scale="{scale}"' if scale else ""
    return f'<collision><geometry><mesh filename="{name}"{s}/></geometry></collision>'


def _part(tmp_path, text, **options):
    """(raw model, the moving body) of a URDF text written to tmp_path, on a fixed base at density 1000."""
    path = tmp_path / "thing.urdf"
    path.write_text(text)
    raw = _assets.parse_urdf(str(path))
    art = _assets.build_articulation(raw, dict(fix_base_link=True, density=1000.0, **options))
    return raw, art.bodies[1]


def test_urdf_with_content_after_the_root(tmp_path):
    tail = '\n<!-- gripper -->\n  <link name="hand">\n <!-- <visual> --> </visual>\n</link>\n</robot>\n'
    text = _urdf(tail=tail)
    path = tmp_path / "thing.urdf"
    path.write_text(text)
    with pytest.raises(ET.ParseError):
        ET.parse(str(path))
    raw = _assets.parse_urdf(str(path))
    assert raw.link_order == ["base", "part"] and [j.name for j in raw.joints] == ["hinge"]
    # a well-formed file takes the path it took
    path.write_text(_urdf())
    assert _assets.parse_urdf(str(path)).link_order == ["base", "part"]
    # no </robot> at all, and a first <robot> that is itself ill-formed: the original error
    for bad in (text.replace("</robot>", ""), _urdf(tail=tail).replace('<link name="base"/>', "<link <")):
        path.write_text(bad)
        with pytest.raises(ET.ParseError) as e:
            _assets.parse_urdf(str(path))
        with pytest.raises(ET.ParseError) as direct:
            ET.parse(str(path))
        assert str(e.value) == str(direct.value)


def test_obj_cube_collides_as_its_hull_and_weighs_its_volume(tmp_path):
    _write_obj(tmp_path / "cube.obj", CUBE + [(0.5, 0.5, 0.5), (0.25, 0.5, 0.75)])  # interior points are no vertices
    raw, body = _part(tmp_path, _urdf(_mesh("cube.obj")))
    shape = raw.links["part"].shapes[0]
    assert shape.kind == _assets.SHAPE_CONVEX and raw.links["part"].dropped_meshes == []
    hull = np.asarray(shape.size).reshape(-1, 3)
    assert sorted(map(tuple, hull)) == sorted(CUBE)
    np.testing.assert_allclose(body.mass, 1000.0, rtol=1e-9)
    np.testing.assert_allclose(body.com, [0.5, 0.5, 0.5], rtol=1e-9)
    np.testing.assert_allclose(body.inertia, np.eye(3) * 1000.0 / 6.0, rtol=1e-9, atol=1e-9 * 1000.0 / 6.0)
    # scale applies to the vertices: half the edge, an eighth of the mass
    raw, body = _part(tmp_path, _urdf(_mesh("cube.obj", "0.5 0.5 0.5")))
    np.testing.assert_allclose(body.mass, 125.0, rtol=1e-9)
    np.testing.assert_allclose(body.com, [0.25, 0.25, 0.25], rtol=1e-9)


def test_tetrahedron_against_its_closed_form(tmp_path):
    """The unit right tetrahedron: volume 1/6, centroid (1/4, 1/4, 1/4), second moments about the origin
    int x^2 = 1/60, int x y = 1/120."""
    _write_obj(tmp_path / "tet.obj", TETRA, extra=False)
    raw, body = _part(tmp_path, _urdf(_mesh("tet.obj")))
    rho, vol, c = 1000.0, 1.0 / 6.0, 0.25
    xx, xy = rho * (1.0 / 60.0 - vol * c * c), rho * (1.0 / 120.0 - vol * c * c)
    want = np.full((3, 3), -xy)
    np.fill_diagonal(want, 2.0 * xx)
    np.testing.assert_allclose(body.mass, rho * vol, rtol=1e-9)
    np.testing.assert_allclose(body.com, [c, c, c], rtol=1e-9)
    np.testing.assert_allclose(body.inertia, want, rtol=1e-9, atol=1e-12)


def test_flat_obj_and_unknown_formats_are_dropped(tmp_path):
    _write_obj(tmp_path / "flat.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0.3, 0.2, 0)])
    _write_obj(tmp_path / "three.obj", TETRA[:3])
    (tmp_path / "mesh.dae").write_text("<COLLADA/>")
    for name in ("flat.obj", "three.obj", "mesh.dae", "absent.obj"):
        raw, body = _part(tmp_path, _urdf(_mesh(name)))
        assert raw.links["part"].shapes == [] and raw.links["part"].dropped_meshes == [name]
        assert body.mass == 1e-3  # a shapeless link keeps the floor


def test_primitives_combine_about_the_common_centre(tmp_path):
    """Two unit boxes side by side are one 2 x 1 x 1 box; a sphere's closed form."""
    box = '<collision><origin xyz="{} 0 0"/><geometry><box size="1 1 1"/></geometry></collision>'
    raw, body = _part(tmp_path, _urdf(box.format(-0.5) + box.format(0.5)))
    m = 2000.0
    np.testing.assert_allclose(body.mass, m, rtol=1e-12)
    np.testing.assert_allclose(body.com, np.zeros(3), atol=1e-12)
    np.testing.assert_allclose(np.diag(body.inertia), [m * 2 / 12, m * 5 / 12, m * 5 / 12], rtol=1e-12)
    raw, body = _part(tmp_path, _urdf('<collision><origin xyz="0 0 2"/><geometry><sphere radius="0.1"/></geometry>'
                                      '</collision>'))
    ms = 1000.0 * 4.0 / 3.0 * np.pi * 1e-3
    np.testing.assert_allclose(body.mass, ms, rtol=1e-12)
    np.testing.assert_allclose(body.com, [0, 0, 2], atol=1e-12)
    np.testing.assert_allclose(body.inertia, np.eye(3) * 0.4 * ms * 0.01, rtol=1e-12, atol=1e-15)


def test_declared_inertial_wins_and_a_shapeless_link_keeps_the_floor(tmp_path):
    _write_obj(tmp_path / "cube.obj", CUBE)
    inertial = ('<inertial><origin xyz="0 0 0.1"/><mass value="2.5"/>'
                '<inertia ixx="0.1" iyy="0.2" izz="0.3" ixy="0" ixz="0" iyz="0"/></inertial>')
    raw, body = _part(tmp_path, _urdf(_mesh("cube.obj"), inertial))
    assert body.mass == 2.5 and len(body.shapes) == 1
    np.testing.assert_array_equal(body.com, [0, 0, 0.1])
    np.testing.assert_array_equal(np.diag(body.inertia), [0.1, 0.2, 0.3])
    raw, body = _part(tmp_path, _urdf())
    assert body.mass == 1e-3 and np.array_equal(body.inertia, np.eye(3) * 1e-6)
    # the welded root of a fixed base keeps the floor whatever its shapes (Cartpole's slider); a free root does not
    text = _urdf().replace('<link name="base"/>', f'<link name="base">{_mesh("cube.obj")}</link>')
    (tmp_path / "rooted.urdf").write_text(text)
    raw = _assets.parse_urdf(str(tmp_path / "rooted.urdf"))
    assert _assets.build_articulation(raw, dict(fix_base_link=True)).bodies[0].mass == 1e-3
    np.testing.assert_allclose(_assets.build_articulation(raw, dict(fix_base_link=False)).bodies[0].mass, 1000.0,
                               rtol=1e-9)
    np.testing.assert_allclose(_assets.build_articulation(raw, dict(fix_base_link=False, density=10.0)).bodies[0].mass,
                               10.0, rtol=1e-9)


def _shipped_models():
    packed = os.path.join(ROOT, "isaacgymenv_amd", "assets")
    return sorted(glob.glob(os.path.join(packed, "*.model.json"))) + [
        os.path.join(M.GOLDEN, "open_manipulator_p.model.json")]


@pytest.mark.parametrize("path", _shipped_models(), ids=os.path.basename)
def test_shipped_models_keep_their_masses(path):
    """Every body's mass is the sum of its links' declared masses, or the 1 g floor: the new rule changes none.  Each
    model with the base its task gives it (Cartpole's slider, the welded root of a fixed base, is the one
    shape-bearing link without an inertial among them)."""
    with open(path) as f:
        raw = _assets.RawModel.from_json(json.load(f))
    fixed = os.path.basename(path) in ("cartpole.model.json", "open_manipulator_p.model.json")
    for collapse in (False, True):
        art = _assets.build_articulation(raw, dict(fix_base_link=fixed, collapse_fixed_joints=collapse))
        declared = {n: (l.inertial.mass if l.inertial is not None else 0.0) for n, l in raw.links.items()}
        children = {}
        for j in raw.joints:
            children.setdefault(j.parent, []).append(j)

        def welded(name):
            total = declared[name]
            for j in children.get(name, []):
                if j.kind == _assets.JOINT_FIXED:
                    total += welded(j.child)
            return total
        for b in art.bodies:
            want = welded(b.name)
            assert b.mass == pytest.approx(want if want > 0 else 1e-3, rel=1e-12), (b.name, b.mass, want)


# ---------------------------------------------------------------- the packed Franka
def test_packed_franka_loads():
    gym = gymapi.acquire_gym()
    opts = gymapi.AssetOptions()
    for k, v in M.MANIP_OPTS.items():
        setattr(opts, k, v)
    asset = gym.load_asset(None, M.GOLDEN, M.MANIP_MODEL, opts)
    assert gym.get_asset_rigid_body_count(asset) == 8 and gym.get_asset_dof_count(asset) == 7
    assert gym.get_asset_rigid_body_names(asset) == [f"panda_link{i}" for i in range(8)]
    props = gym.get_asset_dof_properties(asset)
    assert props["hasLimits"].all()
    np.testing.assert_array_equal(props["effort"], np.asarray(M.EFFORT, np.float32))
    lower, upper = [-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973], [2.8973, 1.7628, 2.8973, -0.0698,
                                                                                     2.8973, 3.7525, 2.8973]
    np.testing.assert_allclose(props["lower"], lower, rtol=1e-6)
    np.testing.assert_allclose(props["upper"], upper, rtol=1e-6)
    art = asset.art
    assert art.num_shapes == 8 and all(len(b.shapes) == 1 and len(b.shapes[0].size) >= 12 for b in art.bodies)
    assert sum(len(b.shapes[0].size) // 3 for b in art.bodies) <= 2048  # the runtime-sized kernel's hull vertices
    with open(os.path.join(M.GOLDEN, M.MANIP_MODEL)) as f:
        packed = json.load(f)
    assert all(l["inertial"] is None and not l["dropped_meshes"] for l in packed["links"])
    masses = [b.mass for b in art.bodies[1:]]
    print("moving link masses [kg]:", np.round(masses, 3), "sum", round(sum(masses), 3))
    # a sanity bracket around the real arm's 18 kg, not a measurement
    assert all(m > 0.05 for m in masses) and 5.0 < sum(masses) < 40.0
    assert art.bodies[0].mass == 1e-3  # the welded root
    for b in art.bodies[1:]:
        assert np.linalg.eigvalsh(b.inertia).min() > 0


@pytest.mark.parametrize("solver,steps", M.PHYSICS_CASES)
def test_oracle_float32_run_stays_inside_the_gpu_comparison_cap(solver, steps):
    """The GPU test compares the Franka on the runtime-sized kernel with the zero-gravity oracle through
    assert_close_or_explained(max_env_frac=0.02); the oracle's own float32 build must pass the same check on the chosen
    seed, or the cap would be asking the kernel for more than float32 gives."""
    n = 64
    art, flat = M.franka()
    root, dof, tau, mu = M.franka_states(n, seed=M.PHYSICS_SEED)
    oparams = dict(M.MANIP_PARAMS, solver_type=3 if solver == "tgs" else 0, gravity=[0.0, 0.0, 0.0])
    assert oparams["pos_iters"] == 8 and oparams["contact_offset"] == 0.005
    r64, d64, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, steps)
    r32, d32, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 32, steps)

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        out = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, steps)
        return H.state_fields(out[0], out[1])
    H.assert_close_or_explained(H.state_fields(r32, d32), H.state_fields(r64, d64), rerun, max_env_frac=0.02,
                                what=f"oracle float32 vs float64, Franka without gravity ({solver}, {steps} simulates)")
    assert np.abs(d64[:, :, 0] - dof[:, :, 0]).max() > 1e-3  # the states move: the comparison is not of a rest pose
    # and gravity matters on these states: the oracle with gravity leaves the zero-gravity result
    g64 = H.oracle_run(flat, dict(oparams, gravity=[0.0, 0.0, -9.81]), root, dof, tau, mu, 64, steps)[1]
    assert np.abs(g64[:, :, 1] - d64[:, :, 1]).max() > 0.1
    # (the GPU test's flag-off check: nine envs in ten leave the zero-gravity result by ten tolerances)
    at, rt = H.STATE_TOL["qd"]
    off = np.abs(g64[:, :, 1] - d64[:, :, 1]) / (at + rt * np.abs(d64[:, :, 1]))
    assert (off.max(axis=1) > 10.0).mean() > 0.9


# ---------------------------------------------------------------- the C ABI
def test_manip_struct_layouts_match_the_header(tmp_path):
    """gcc's sizeof / offsetof of the gt_manip_* structs against the ctypes mirrors (tests/test_abi.py's method)."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from isaacgymenv_amd import gymtask
    mirrors = {"gt_manip_params": gymtask.GtManipParams, "gt_manip_reset_args": gymtask.GtManipResetArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gymtask.h"', "int main(void) {"]
    expect = []
    for cname, py in mirrors.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        expect.append(ctypes.sizeof(py))
        for f in py._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {f[0]}));')
            expect.append(getattr(py, f[0]).offset)
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == expect
    assert len(gymtask.GtManipParams().dof_default) == 8 and len(gymtask.GtManipParams().kp) == 6


def test_manip_entry_points_refuse_bad_parameters():
    """The entry points validate what indexes memory before any launch, so the refusals need no GPU."""
    from isaacgymenv_amd import gymtask
    L = gymtask.lib()
    assert L.gt_abi_version() == 6
    keep = (ctypes.c_float * 64)()
    addr = ctypes.addressof(keep)

    def params(**over):
        p = gymtask.GtManipParams()
        p.num_envs, p.nd, p.num_links, p.jac_row, p.eef_link, p.effort_stride = 4, 7, 8, 6, 7, 7
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def control(p, *bufs):
        bufs = bufs or (addr,) * 7
        return L.gt_osc_control(ctypes.byref(p), *bufs, None)

    for bad in (dict(nd=5), dict(nd=8), dict(nd=0), dict(eef_link=8), dict(jac_row=8), dict(jac_row=-1),
                dict(effort_stride=6), dict(num_envs=0)):
        assert control(params(**bad)) != 0, bad
        assert "gt_osc_control" in L.gt_last_error().decode()
    assert control(params(nd=6, effort_stride=5)) != 0
    for missing in range(7):  # each null buffer
        bufs = [addr] * 7
        bufs[missing] = None
        assert control(params(), *bufs) != 0, missing
    assert L.gt_osc_control(None, *(addr,) * 7, None) != 0

    b = gymtask.GtArmBuffers()
    for name, _ in gymtask.GtArmBuffers._fields_:
        if name != "seq":
            setattr(b, name, addr)

    def reset(p, numels, k=2, null=None, buffers=b):
        r = gymtask.GtManipResetArgs()
        for name in ("dof_state", "commands", "pos_control", "effort_control", "progress_buf", "env_ids_out"):
            setattr(r, name, None if name == null else addr)
        for i, numel in enumerate(numels):
            r.plan[i].numel = numel
        return L.gt_manip_reset_flagged(ctypes.byref(p), ctypes.byref(buffers), k, ctypes.byref(r), None)

    for numels in ((2, 2, 2, 12), (2, 2, 2, 13), (2, 2, 1, 14), (14, 2, 2, 2)):  # not k, k, k, 7k
        assert reset(params(), numels) != 0, numels
        assert "k x 7" in L.gt_last_error().decode()
    assert reset(params(nd=6, effort_stride=7), (2, 2, 2, 14)) != 0  # the reset is the 7-dof one
    assert reset(params(), (5, 5, 5, 35), k=5) != 0  # more than num_envs
    assert reset(params(), (2, 2, 2, 14), null="dof_state") != 0
    assert reset(params(), (2, 2, 2, 14), null="env_ids_out") != 0
    nomask = gymtask.GtArmBuffers()
    nomask.reset_buf = addr
    assert reset(params(), (2, 2, 2, 14), buffers=nomask) != 0
    assert reset(params(), (0, 0, 0, 0), k=0) == 0  # nothing flagged: no launch, no error
    assert {"gt_osc_control", "gt_manip_reset_flagged"} <= set(gymtask.EXPORTED_SYMBOLS)
