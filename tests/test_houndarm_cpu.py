"""Houndarm (tasks/hound_arm.py) and the simulator's gravity switch, CPU side.

The torch path of the task, driven by tests/arm_cases.ArmFakeGym, against a recording of the reference's own
tasks/hound_arm.py on the same fake (tests/golden/make_golden_houndarm.py): reset, progress, commands and the reset
dof state must be identical (the same torch draws from the same generator state), observations and rewards within
rtol 1e-5 / atol 2e-6, torques within 1e-4.  The two config files against the reference's parsed values.  The packed
arm model opens as an asset file; a missing asset names the two config keys; joint_tor and randomize are refused; a
filter-0 fixed-base actor warns once.  AssetOptions.disable_gravity on libgymsim's host backend: a tilted Cartpole at
rest stays where it is, and falls with the flag off.
"""
import copy
import ctypes
import json
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch
import yaml

from isaacgymenv_amd.isaacgym import gymapi
from tests import arm_cases as A
from tests import helpers as H
from tests.test_hound_terrain_cpu import _resolved_leaves, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "isaacgymenv_amd", "isaacgymenvs", "cfg")


def _fixture():
    return np.load(os.path.join(A.GOLDEN, "houndarm.npz"))


def _cfg(d):
    return A.point_at_fixture(yaml.safe_load(str(d["cfg_yaml"])))


def make_on_fake(monkeypatch, cfg=None):
    """(env, fixture): the task built on the fake from the fixture's config, at the fixture's seed."""
    from isaacgymenv_amd.isaacgymenvs.tasks import hound_arm
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    d = _fixture()
    fake = A.ArmFakeGym(seed=A.FAKE_SEED)
    monkeypatch.setattr(gymapi, "acquire_gym", lambda: fake)
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        env = hound_arm.Houndarm(copy.deepcopy(cfg or _cfg(d)), "cpu", "cpu", -1, True, False, False)
    return env, d


def test_torch_path_matches_the_reference(monkeypatch):
    env, d = make_on_fake(monkeypatch)
    A.assert_fixture_conditions(d)
    assert env.num_obs == 10 and env.num_actions == 6 and env._kernels is None
    assert env.eef_index == int(d["eef_index"]) and env.max_episode_length == int(d["max_episode_length"]) == 12
    np.testing.assert_array_equal(env.dof_lower_limits.numpy(), d["dof_lower"])
    np.testing.assert_array_equal(env.dof_upper_limits.numpy(), d["dof_upper"])
    np.testing.assert_array_equal(env.effort_limits.numpy(), d["effort_limits"])
    np.testing.assert_array_equal(env.kd.numpy(), d["kd"])
    np.testing.assert_array_equal(env.kd_null.numpy(), d["kd_null"])
    A.stagger(env)
    np.testing.assert_array_equal(env.commands.numpy(), d["init_commands"])  # (draw order of the initial reset)
    np.testing.assert_array_equal(env.dof_state.view(-1, 6, 2).numpy(), d["init_dof_state"])
    np.testing.assert_array_equal(env.reset_buf.numpy(), d["init_reset"])
    np.testing.assert_array_equal(env.progress_buf.numpy(), d["init_progress"])
    n = env.num_envs
    worst = 0.0
    for t in range(d["actions"].shape[0]):
        A.place_commands(env)
        np.testing.assert_array_equal(env.j_eef.numpy(), d["ctl_jac"][t], err_msg=f"control inputs step {t}")
        obs, rew, reset, extras = env.step(torch.from_numpy(d["actions"][t]))
        assert reset.dtype == torch.int64
        np.testing.assert_array_equal(reset.numpy(), d["reset"][t], err_msg=f"reset step {t}")
        np.testing.assert_array_equal(extras["time_outs"].numpy().astype(np.int64), d["time_outs"][t])
        np.testing.assert_array_equal(env.progress_buf.numpy(), d["progress"][t], err_msg=f"progress step {t}")
        np.testing.assert_array_equal(env.commands.numpy(), d["commands"][t], err_msg=f"commands step {t}")
        flagged = d["in_reset"][t] != 0
        np.testing.assert_array_equal(env.dof_state.view(n, 6, 2).numpy()[flagged], d["dof_state"][t][flagged],
                                      err_msg=f"reset dof state step {t}")
        np.testing.assert_allclose(obs["obs"].numpy(), d["obs"][t], rtol=1e-5, atol=2e-6, err_msg=f"obs step {t}")
        np.testing.assert_allclose(rew.numpy(), d["rew"][t], rtol=1e-5, atol=2e-6, err_msg=f"reward step {t}")
        # (the effort tensor of a just-reset env is zeroed by reset_idx: the recording took it before the simulate)
        np.testing.assert_allclose(env.sim.force.view(n, 6).numpy()[~flagged], d["torques"][t][~flagged], rtol=1e-4,
                                   atol=1e-4, err_msg=f"torques step {t}")
        worst = max(worst, float(np.abs(env.sim.force.view(n, 6).numpy()[~flagged] - d["torques"][t][~flagged]).max()))
    np.testing.assert_array_equal(torch.get_rng_state().numpy(), d["final_rng_state"])
    print(f"largest torque difference to the recording: {worst:.3g}")


def test_generator_state_before_each_reset_matches(monkeypatch):
    """The same torch draws from the same generator state: the state before every post_physics_step."""
    env, d = make_on_fake(monkeypatch)
    A.stagger(env)
    for t in range(d["actions"].shape[0]):
        A.place_commands(env)
        env.pre_physics_step(torch.clamp(torch.from_numpy(d["actions"][t]), -1.0, 1.0))
        env.gym.simulate(env.sim)
        np.testing.assert_array_equal(torch.get_rng_state().numpy(), d["in_rng_state"][t], err_msg=f"step {t}")
        np.testing.assert_array_equal(env.reset_buf.numpy(), d["in_reset"][t])
        env.post_physics_step()


def test_float64_restatement_tracks_the_recorded_torques():
    """The fixture's float64 OSC against the reference's float32 torques on well-conditioned envs, and the restatement
    recomputed here equals the stored one (the GPU test's reference is what the generator computed)."""
    d = _fixture()
    again = np.stack([A.osc_float64(d["ctl_actions"][t], d["ctl_jac"][t], d["ctl_mm"][t], d["ctl_eef"][t],
                                    d["ctl_dof"][t], d["effort_limits"]) for t in range(d["torques"].shape[0])])
    np.testing.assert_allclose(again, d["torques64"], rtol=1e-12, atol=1e-12)
    err = np.abs(d["torques"] - d["torques64"]) / np.maximum(1.0, np.abs(d["torques64"]))
    assert np.median(err) < 1e-4, np.median(err)


def test_config_values_match_the_reference():
    with open(os.path.join(A.GOLDEN, "houndarm_cfg.json")) as f:
        ref = json.load(f)
    with open(os.path.join(CFG, "task", "Houndarm.yaml")) as f:
        _same(yaml.safe_load(f), ref["task"], "task")
    with open(os.path.join(CFG, "train", "HoundarmPPO.yaml")) as f:
        _same(yaml.safe_load(f), ref["train"], "train")
    from isaacgymenv_amd.isaacgymenvs.config import compose
    c = compose("config", ["task=Houndarm", "num_envs=64", "sim_device=cuda:0"])
    _resolved_leaves(c["task"], ref["task"], "task")
    _resolved_leaves(c["train"], ref["train"], "train")
    t = c["task"]
    assert t["name"] == "Houndarm" and t["env"]["numEnvs"] == 64 and t["sim"]["use_gpu_pipeline"] is True
    assert c["train"]["params"]["config"]["name"] == "Houndarm" and c["train"]["params"]["config"]["num_actors"] == 64
    assert c["train"]["params"]["network"]["separate"] is False
    assert c["train"]["params"]["network"]["mlp"]["units"] == [256, 128, 64]
    assert compose("config", ["task=Houndarm"])["task"]["env"]["numEnvs"] == 8192


def test_task_is_registered():
    from isaacgymenv_amd.isaacgymenvs.tasks import isaacgym_task_map
    from isaacgymenv_amd.isaacgymenvs.tasks.hound_arm import Houndarm
    assert isaacgym_task_map["Houndarm"] is Houndarm


def test_load_asset_opens_the_packed_model():
    gym = gymapi.acquire_gym()
    opts = gymapi.AssetOptions()
    for k, v in A.ARM_OPTS.items():
        setattr(opts, k, v)
    asset = gym.load_asset(None, A.GOLDEN, A.ARM_MODEL, opts)
    assert gym.get_asset_rigid_body_count(asset) == 7 and gym.get_asset_dof_count(asset) == 6
    assert gym.get_asset_rigid_body_names(asset)[-1] == "end_link"
    props = gym.get_asset_dof_properties(asset)
    assert props["hasLimits"].all()
    np.testing.assert_array_equal(props["lower"], np.full(6, -1.57, np.float32))
    np.testing.assert_array_equal(props["upper"], np.full(6, 1.57, np.float32))
    np.testing.assert_array_equal(props["effort"], np.full(6, 1000.0, np.float32))
    # the STL colliders are packed as their hull vertices: one hull per link
    assert asset.art.num_shapes == 7 and len(asset.flat["hverts"]) > 100


def test_missing_asset_names_the_two_config_keys(monkeypatch, tmp_path):
    d = _fixture()
    cfg = _cfg(d)
    cfg["env"]["asset"] = {"assetRoot": str(tmp_path), "assetFileNamehoundarm": "nothing_here.urdf"}
    with pytest.raises(FileNotFoundError) as e:
        make_on_fake(monkeypatch, cfg)
    assert "env.asset.assetRoot" in str(e.value) and "env.asset.assetFileNamehoundarm" in str(e.value)


def test_joint_tor_and_randomize_are_refused(monkeypatch):
    d = _fixture()
    cfg = _cfg(d)
    cfg["env"]["controlType"] = "joint_tor"
    with pytest.raises(NotImplementedError, match="joint_tor"):
        make_on_fake(monkeypatch, cfg)
    cfg = _cfg(d)
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="randomi"):
        make_on_fake(monkeypatch, cfg)


def _actors(kind, filter_, n=3):
    """n envs of one actor each on a fake sim (actor bookkeeping is gymapi's own pure-Python part)."""
    fake = A.ArmFakeGym()
    sim = fake.create_sim()
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    if kind == "arm":
        opts.collapse_fixed_joints = False
        asset = fake.load_asset(sim, A.GOLDEN, A.ARM_MODEL, opts)
    else:
        asset = fake.load_asset(sim, "/nonexistent", "urdf/cartpole.urdf", opts)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for i in range(n):
            env = fake.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 2)
            fake.create_actor(env, asset, gymapi.Transform(), kind, i, filter_, 0)
    return [x for x in w if issubclass(x.category, gymapi.PhysicsDeviationWarning)]


def test_fixed_base_actor_with_filter_0_warns_once():
    w = _actors("arm", 0)
    assert len(w) == 1 and "fixed-base" in str(w[0].message) and "DESIGN.md section 6" in str(w[0].message)
    assert _actors("arm", 1) == []
    assert _actors("cartpole", 1) == []  # Cartpole's own filter: silent


def _cartpole_after(disable_gravity, steps=20):
    n = 2
    gym, sim = A.make_sim("cartpole", n, H.CARTPOLE_PARAMS, disable_gravity, host=True)
    assert sim.kernel_variant == 3 and sim.disable_gravity is disable_gravity
    root, dof, mu = A.tilted_cartpole(n)
    H.load_state_into(sim, root, dof, mu)
    sim.dof_force.zero_()
    for _ in range(steps):
        gym.simulate(sim)
    return sim, dof, H.read_state(sim, 2)[1]


def test_disable_gravity_on_the_host_backend():
    """A tilted pole at rest with no effort.  Without gravity the bias force of a resting articulation is exactly
    zero, so are the accelerations, and the solver has no contact or limit row to satisfy: the velocity never leaves
    zero, and the bound on the state is zero, not a tolerance.  With gravity the pole falls."""
    sim, start, end = _cartpole_after(True)
    np.testing.assert_array_equal(end, start.astype(np.float32).astype(np.float64))
    assert sim.cparams.gravity[2] == pytest.approx(-9.81)  # the sim parameter keeps its value
    _, start, end = _cartpole_after(False)
    assert abs(end[0, 1, 0] - start[0, 1, 0]) > 1e-2


@pytest.mark.parametrize("solver,steps", A.PHYSICS_CASES)
def test_oracle_float32_run_stays_inside_the_gpu_comparison_cap(solver, steps):
    """The GPU test compares the arm on the runtime-sized kernel with the zero-gravity oracle through
    assert_close_or_explained(max_env_frac=0.02); the oracle's own float32 build must pass the same check on the chosen
    seed, or the cap would be asking the kernel for more than float32 gives."""
    n = 64
    art, flat = A.arm()
    root, dof, tau, mu = A.arm_states(n, seed=A.PHYSICS_SEED)
    oparams = dict(A.ARM_PARAMS, solver_type=3 if solver == "tgs" else 0, gravity=[0.0, 0.0, 0.0])
    r64, d64, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 64, steps)
    r32, d32, _, _ = H.oracle_run(flat, oparams, root, dof, tau, mu, 32, steps)

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        out = H.oracle_run(flat, oparams, r, d, tau[idx], mu[idx], bits, steps)
        return H.state_fields(out[0], out[1])
    H.assert_close_or_explained(H.state_fields(r32, d32), H.state_fields(r64, d64), rerun, max_env_frac=0.02,
                                what=f"oracle float32 vs float64, arm without gravity ({solver}, {steps} simulates)")
    assert np.abs(d64[:, :, 0] - dof[:, :, 0]).max() > 1e-3  # the states move: the comparison is not of a rest pose
    # and gravity matters on these states: the oracle with gravity leaves the zero-gravity result
    g64 = H.oracle_run(flat, dict(oparams, gravity=[0.0, 0.0, -9.81]), root, dof, tau, mu, 64, steps)[1]
    assert np.abs(g64[:, :, 1] - d64[:, :, 1]).max() > 0.1


def test_disable_gravity_after_prepare_is_refused():
    from isaacgymenv_amd.isaacgym import _lib
    gym, sim = A.make_sim("cartpole", 2, H.CARTPOLE_PARAMS, False, host=True)
    L = _lib.lib()
    assert L.gs_sim_set_disable_gravity(sim.handle, 1) != 0
    assert "before gs_sim_prepare" in L.gs_last_error().decode()
    assert L.gs_abi_version() == 9
    # valid from gs_sim_create on
    h = L.gs_sim_create(-1, sim.cparams)
    assert h and L.gs_sim_set_disable_gravity(h, 1) == 0 and L.gs_sim_set_disable_gravity(h, 0) == 0
    L.gs_sim_destroy(h)


def test_houndarm_on_the_cpu_is_refused_with_the_runtime_kernel_message(monkeypatch):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        with pytest.raises(RuntimeError, match="runtime-sized kernel is a GPU kernel"):
            isaacgymenvs.make(seed=0, task="Houndarm", num_envs=4, sim_device="cpu", rl_device="cpu", headless=True,
                              force_render=False,
                              overrides=["pipeline=cpu", f"task.env.asset.assetRoot={A.GOLDEN}",
                                         f"task.env.asset.assetFileNamehoundarm={A.ARM_MODEL}"])


def test_arm_struct_layouts_match_the_header(tmp_path):
    """gcc's sizeof / offsetof of the gt_arm_* structs against the ctypes mirrors (tests/test_abi.py's method)."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from isaacgymenv_amd import gymtask
    mirrors = {"gt_arm_params": gymtask.GtArmParams, "gt_arm_buffers": gymtask.GtArmBuffers,
               "gt_arm_reset_args": gymtask.GtArmResetArgs}
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


def test_arm_entry_points_refuse_bad_parameters():
    """The entry points validate what indexes memory before any launch, so the refusals need no GPU."""
    from isaacgymenv_amd import gymtask
    L = gymtask.lib()
    assert L.gt_abi_version() == 6
    keep = (ctypes.c_float * 64)()
    addr = ctypes.addressof(keep)
    p = gymtask.GtArmParams()
    p.num_envs, p.num_links, p.jac_row, p.eef_link, p.effort_stride = 4, 7, 5, 7, 6  # eef one past the last link
    assert L.gt_arm_control(ctypes.byref(p), addr, addr, addr, addr, addr, addr, addr, None) != 0
    assert "gt_arm_control" in L.gt_last_error().decode()
    b = gymtask.GtArmBuffers()
    for name, _ in gymtask.GtArmBuffers._fields_:
        if name != "seq":
            setattr(b, name, addr)
    assert L.gt_arm_post_physics(ctypes.byref(p), ctypes.byref(b), None) != 0
    p.eef_link = 6
    r = gymtask.GtArmResetArgs()
    for name in ("dof_state", "commands", "pos_control", "effort_control", "progress_buf", "env_ids_out"):
        setattr(r, name, addr)
    for i, numel in enumerate((2, 2, 2, 11)):  # the last plan does not cover k x 6
        r.plan[i].numel = numel
    assert L.gt_arm_reset_flagged(ctypes.byref(p), ctypes.byref(b), 2, ctypes.byref(r), None) != 0
    assert "k x 6" in L.gt_last_error().decode()
