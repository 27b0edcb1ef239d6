"""Humanoid (tasks/humanoid.py), CPU side.

The torch path of the task, driven by tests/humanoid_cases.HumanoidFakeGym, against a recording of the reference's own
tasks/humanoid.py on the same fake (tests/golden/make_golden_humanoid.py): resets, progress, time-outs and the reset
dof state must be identical (the same torch draws from the same generator state, which also ends in the same place),
observations, potentials and rewards within Ant's tolerances (tests/test_golden_tasks.py: rtol 1e-5, atol 1e-6;
observations atol 2e-6).  The two config files against the
reference's parsed values; task.randomize and sim_device=cpu are refused; a missing asset names the two config keys.
"""
import copy
import json
import os
import warnings

import numpy as np
import pytest
import torch
import yaml

from isaacgymenv_amd.isaacgym import gymapi
from tests import humanoid_cases as HC
from tests.test_hound_terrain_cpu import _resolved_leaves, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "isaacgymenv_amd", "isaacgymenvs", "cfg")


def _fixture():
    return np.load(os.path.join(HC.GOLDEN, "humanoid.npz"))


def _cfg(d):
    return HC.point_at_fixture(yaml.safe_load(str(d["cfg_yaml"])))


def make_on_fake(monkeypatch, cfg=None):
    """(env, fixture): the task built on the fake from the fixture's config, at the fixture's seed."""
    from isaacgymenv_amd.isaacgymenvs.tasks import humanoid
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    d = _fixture()
    fake = HC.HumanoidFakeGym(seed=HC.FAKE_SEED)
    monkeypatch.setattr(gymapi, "acquire_gym", lambda: fake)
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    torch.manual_seed(42)
    env = humanoid.Humanoid(copy.deepcopy(cfg or _cfg(d)), "cpu", "cpu", -1, True, False, False)
    return env, d


def test_torch_path_matches_the_reference(monkeypatch):
    env, d = make_on_fake(monkeypatch)
    print("fixture cases:", HC.assert_fixture_conditions(d))
    n, nd = env.num_envs, HC.ND
    assert env.num_obs == 108 and env.num_actions == 21 and env._tail is None
    assert env.num_dof == int(d["num_dof"]) == 21 and env.num_bodies == int(d["num_bodies"]) == 16
    assert env.max_episode_length == int(d["max_episode_length"]) == HC.EPISODE_LENGTH
    np.testing.assert_array_equal(env.motor_efforts.numpy(), d["motor_efforts"])
    assert env.max_motor_effort == float(d["max_motor_effort"]) == 135.0
    np.testing.assert_array_equal(env.dof_limits_lower.numpy(), d["dof_limits_lower"])
    np.testing.assert_array_equal(env.dof_limits_upper.numpy(), d["dof_limits_upper"])
    np.testing.assert_array_equal(env.initial_dof_pos.numpy(), d["initial_dof_pos"])
    np.testing.assert_array_equal(env.initial_root_states.numpy(), d["initial_root_states"])
    assert float(env.initial_root_states[0, 2]) == np.float32(1.34)
    # the passive joint springs and dampers: every actor in DOF_MODE_POS with the MJCF's gains
    props = env.envs[-1].actors[0].dof_props
    assert (props["driveMode"] == gymapi.DOF_MODE_POS).all() and props["stiffness"][0] == 20.0 and props["damping"][0] == 5.0
    actions = np.asarray(d["actions"])
    for t in range(actions.shape[0]):
        if t == HC.STAGGER_STEP:
            HC.stagger(env)
        np.testing.assert_array_equal(env.reset_buf.numpy(), d["in_reset"][t], err_msg=f"flagged envs step {t}")
        obs, rew, reset, extras = env.step(torch.from_numpy(actions[t]))
        assert reset.dtype == torch.int64
        np.testing.assert_array_equal(reset.numpy(), d["out_reset"][t], err_msg=f"reset step {t}")
        np.testing.assert_array_equal(extras["time_outs"].numpy().astype(np.int64), d["time_outs"][t])
        np.testing.assert_array_equal(env.progress_buf.numpy(), d["progress"][t], err_msg=f"progress step {t}")
        # the dof state after reset_idx and the refreshes, the reset envs' draws included: exactly
        np.testing.assert_array_equal(env.dof_state.numpy(), d["in_dof"][t], err_msg=f"dof state step {t}")
        k = int(d["reset_count_in"][t])
        flagged = d["in_reset"][t] != 0
        want = d["initial_dof_pos"][flagged] + d["draw_positions"][t][:k]
        want = np.maximum(np.minimum(want, d["dof_limits_upper"]), d["dof_limits_lower"])
        np.testing.assert_array_equal(env.dof_state.view(n, nd, 2).numpy()[flagged, :, 0], want)
        np.testing.assert_allclose(obs["obs"].numpy(), d["out_obs"][t], rtol=1e-5, atol=2e-6, err_msg=f"obs step {t}")
        np.testing.assert_allclose(rew.numpy(), d["out_rew"][t], rtol=1e-5, atol=1e-6, err_msg=f"reward step {t}")
        np.testing.assert_allclose(env.potentials.numpy(), d["out_potentials"][t], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(env.prev_potentials.numpy(), d["out_prev_potentials"][t], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(env.up_vec.numpy(), d["out_up_vec"][t], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(env.heading_vec.numpy(), d["out_heading_vec"][t], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(torch.get_rng_state().numpy(), d["final_rng_state"])


def test_nonfinite_envs_end_as_fallen_ones():
    from isaacgymenv_amd.isaacgymenvs.tasks.humanoid import end_nonfinite_envs
    obs, rew, reset = torch.ones(4, 108), torch.tensor([1.0, float("nan"), 2.0, 3.0]), torch.zeros(4, dtype=torch.int64)
    obs[2, 7], obs[3, 100] = float("inf"), float("nan")
    end_nonfinite_envs(obs, rew, reset, -1.0)
    assert (obs[0] == 1).all() and (obs[1:] == 0).all()
    assert rew.tolist() == [1.0, -1.0, -1.0, -1.0] and reset.tolist() == [0, 1, 1, 1]


def test_config_values_match_the_reference():
    with open(os.path.join(HC.GOLDEN, "humanoid_cfg.json")) as f:
        ref = json.load(f)
    with open(os.path.join(CFG, "task", "Humanoid.yaml")) as f:
        _same(yaml.safe_load(f), ref["task"], "task")
    with open(os.path.join(CFG, "train", "HumanoidPPO.yaml")) as f:
        _same(yaml.safe_load(f), ref["train"], "train")
    from isaacgymenv_amd.isaacgymenvs.config import compose
    c = compose("config", ["task=Humanoid", "num_envs=64", "sim_device=cuda:0"])
    _resolved_leaves(c["task"], ref["task"], "task")
    _resolved_leaves(c["train"], ref["train"], "train")
    t = c["task"]
    assert t["name"] == "Humanoid" and t["env"]["numEnvs"] == 64 and t["sim"]["use_gpu_pipeline"] is True
    assert c["train"]["params"]["config"]["name"] == "Humanoid" and c["train"]["params"]["config"]["num_actors"] == 64
    assert c["train"]["params"]["network"]["mlp"]["units"] == [400, 200, 100]
    assert compose("config", ["task=Humanoid"])["task"]["env"]["numEnvs"] == 4096


def test_task_is_registered():
    from isaacgymenv_amd.isaacgymenvs.tasks import isaacgym_task_map
    from isaacgymenv_amd.isaacgymenvs.tasks.humanoid import Humanoid
    assert isaacgym_task_map["Humanoid"] is Humanoid


def test_missing_asset_names_the_two_config_keys(monkeypatch, tmp_path):
    cfg = _cfg(_fixture())
    cfg["env"]["asset"] = {"assetRoot": str(tmp_path), "assetFileName": "mjcf/nv_humanoid.xml"}
    with pytest.raises(FileNotFoundError) as e:
        make_on_fake(monkeypatch, cfg)
    assert "env.asset.assetRoot" in str(e.value) and "env.asset.assetFileName" in str(e.value)
    assert "tools/pack_assets.py" in str(e.value)


def test_randomize_is_refused(monkeypatch):
    cfg = _cfg(_fixture())
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="randomi"):
        make_on_fake(monkeypatch, cfg)


def test_humanoid_on_the_cpu_is_refused_with_the_runtime_kernel_message(monkeypatch):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", gymapi.PhysicsDeviationWarning)
        with pytest.raises(RuntimeError, match="runtime-sized kernel is a GPU kernel"):
            isaacgymenvs.make(seed=0, task="Humanoid", num_envs=4, sim_device="cpu", rl_device="cpu", headless=True,
                              force_render=False,
                              overrides=["pipeline=cpu", f"task.env.asset.assetRoot={HC.GOLDEN}",
                                         f"task.env.asset.assetFileName={HC.MODEL}"])


def test_humanoid_struct_layouts_match_the_header(tmp_path):
    """gcc's sizeof / offsetof of the gt_humanoid_* structs against the ctypes mirrors (tests/test_abi.py's method)."""
    import ctypes
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from isaacgymenv_amd import gymtask
    mirrors = {"gt_humanoid_params": gymtask.GtHumanoidParams, "gt_humanoid_buffers": gymtask.GtHumanoidBuffers,
               "gt_humanoid_reset_args": gymtask.GtHumanoidResetArgs}
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
    assert len(gymtask.GtHumanoidParams().dof_lower) == 32


def test_humanoid_entry_points_refuse_bad_parameters():
    """The entry points validate what indexes memory before any launch, so the refusals need no GPU."""
    import ctypes as C
    from isaacgymenv_amd import gymtask
    L = gymtask.lib()
    assert L.gt_abi_version() == 6  # additive entry points: the ABI number stays
    p, b, r = gymtask.GtHumanoidParams(), gymtask.GtHumanoidBuffers(), gymtask.GtHumanoidResetArgs()
    p.num_envs = 4
    for nd in (0, 33):
        p.num_dofs = nd
        assert L.gt_humanoid_post_physics(C.byref(p), C.byref(b), None) == -1
        assert b"num_dofs" in L.gt_last_error()
        assert L.gt_humanoid_reset_flagged(C.byref(p), C.byref(b), 1, C.byref(r), None) == -1
    p.num_dofs = 21
    assert L.gt_humanoid_post_physics(C.byref(p), C.byref(b), None) == -1  # null buffers
    assert L.gt_humanoid_reset_flagged(C.byref(p), C.byref(b), 1, C.byref(r), None) == -1
