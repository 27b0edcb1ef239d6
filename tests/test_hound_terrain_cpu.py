"""HoundTerrain without a GPU: the task's torch path against the reference's recording, its configuration against the
reference's parsed values, and the gymtask ABI 6 structs.

tests/golden/hound_terrain.npz (+ hound_terrain_tail.npz) is the reference's Hound_terrain.py on
tests/fakegym_hound.HoundFakeGym (tests/golden/make_golden_hound_terrain.py); hound_terrain_cfg.json is yaml.safe_load
of the reference's two config files.  Integer and bool outputs must be identical, floats within 1e-5 relative, as in
tests/test_golden_tasks.py.
"""
import copy
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from isaacgymenv_amd.isaacgym import gymapi
from tests.fakegym_hound import HoundFakeGym, assert_fixture_conditions, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(ROOT, "isaacgymenv_amd", "isaacgymenvs", "cfg")


def _close(a, b, what, rtol=1e-5, atol=1e-6):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol,
                               err_msg=what)


# ---------------------------------------------------------------- the task layer, torch path
def test_fixture_holds_every_termination_cause():
    c = assert_fixture_conditions(load_fixture())
    print("hound_terrain.npz cases:", c)


def test_hound_terrain_matches_reference(monkeypatch):
    """HoundTerrain on the fake (CPU pipeline, torch statements) step by step against the reference: link indices,
    the RNG order of the initial reset, done masks (shoulder, thigh, trunk, episode limit), the 0.48 m base-height
    term, the 188-wide observation with its noise draws, commands in HoundTerrain's ranges, episode extras."""
    d = load_fixture()
    assert_fixture_conditions(d)
    fake = HoundFakeGym()
    monkeypatch.setattr(gymapi, "acquire_gym", lambda: fake)
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    from isaacgymenv_amd.isaacgymenvs.tasks import isaacgym_task_map
    cfg = yaml.safe_load(str(d["cfg_yaml"]))
    assert cfg["env"]["learn"]["baseHeightRewardScale"] == -5.0 and cfg["env"]["learn"]["allowKneeContacts"] is True
    torch.manual_seed(42)
    env = isaacgym_task_map["HoundTerrain"](copy.deepcopy(cfg), "cpu", "cpu", -1, True, False, False)
    assert env._kernels is None, "the CPU pipeline runs the torch statements"
    _close(env.commands.numpy(), d["init_commands"], "commands after the initial reset (RNG order at init)")
    _close(env.dof_state.numpy(), d["init_dof_state"], "dof state after the initial reset")
    _close(env.root_states.numpy(), d["init_root_states"], "root states after the initial reset")
    for k in ("feet_indices", "knee_indices", "base_indices"):
        assert len(d[k]) == 4
        np.testing.assert_array_equal(getattr(env, k).numpy(), d[k], err_msg=k)
    assert int(env.base_index) == int(d["base_index"]) and env.max_episode_length == int(d["max_episode_length"])
    assert env.num_obs == 188 and env.contact_forces.shape[1] == 17 and env.num_dof == 12
    _close(env.noise_scale_vec.numpy(), d["noise_scale_vec"], "noise scale vector")
    _close(env.default_dof_pos[0].numpy(), d["default_dof_pos"], "default joint angles in dof order")
    terms = [str(t) for t in d["terms"]]
    for t in range(d["actions"].shape[0]):
        obs, rew, reset, extras = env.step(torch.from_numpy(d["actions"][t]))
        assert reset.dtype == torch.bool
        np.testing.assert_array_equal(reset.numpy().astype(np.int64), d["reset"][t], err_msg=f"reset step {t}")
        np.testing.assert_array_equal(extras["time_outs"].numpy().astype(np.int64), d["time_outs"][t])
        np.testing.assert_array_equal(env.progress_buf.numpy(), d["progress"][t], err_msg=f"progress step {t}")
        _close(rew.numpy(), d["rew"][t], f"reward step {t}")
        _close(obs["obs"].numpy(), d["obs"][t], f"obs step {t}")
        _close(env.commands.numpy(), d["commands"][t], f"commands step {t}")
        _close(env.feet_air_time.numpy(), d["feet_air_time"][t], f"feet air time step {t}")
        _close(np.stack([env.episode_sums[k].numpy() for k in terms]), d["episode_sums"][t], f"episode sums {t}")
        _close(env.root_states.numpy(), d["out_root"][t], f"root states step {t}")
        _close(env.dof_state.numpy(), d["out_dof"][t], f"dof state step {t}")
        assert int("episode" in extras) == int(d["ep_mask"][t])
        if d["ep_mask"][t]:
            got = np.array([float(extras["episode"]["rew_" + k]) for k in terms] +
                           [float(extras["episode"]["terrain_level"])])
            _close(got, d["ep_extras"][t], f"extras episode step {t}", rtol=1e-5, atol=1e-7)
        env.extras.pop("episode", None)


# ---------------------------------------------------------------- configuration
def _same(ours, ref, path=""):
    """ours == ref value by value: the same keys, lists of the same length, leaves equal (1 == 1.0, 0 == -0.0)."""
    if isinstance(ref, dict):
        assert isinstance(ours, dict) and sorted(ours) == sorted(ref), f"{path}: keys {sorted(ours)} != {sorted(ref)}"
        for k in ref:
            _same(ours[k], ref[k], f"{path}.{k}")
    elif isinstance(ref, list):
        assert isinstance(ours, list) and len(ours) == len(ref), f"{path}: {ours} != {ref}"
        for i, (a, b) in enumerate(zip(ours, ref)):
            _same(a, b, f"{path}[{i}]")
    else:
        assert type(ours) is type(ref) or (isinstance(ours, (int, float)) and isinstance(ref, (int, float))
                                            and not isinstance(ours, bool) and not isinstance(ref, bool)), \
            f"{path}: {ours!r} ({type(ours).__name__}) != {ref!r} ({type(ref).__name__})"
        assert ours == ref, f"{path}: {ours!r} != {ref!r}"


def _resolved_leaves(ours, ref, path=""):
    """The composed config against the fixture wherever the fixture's leaf is not a resolver string."""
    if isinstance(ref, dict):
        for k in ref:
            assert k in ours, f"{path}.{k} missing"
            _resolved_leaves(ours[k], ref[k], f"{path}.{k}")
    elif isinstance(ref, list):
        assert len(ours) == len(ref), path
        for i, (a, b) in enumerate(zip(ours, ref)):
            _resolved_leaves(a, b, f"{path}[{i}]")
    elif not (isinstance(ref, str) and "${" in ref):
        assert ours == ref, f"{path}: {ours!r} != {ref!r}"


def test_config_values_match_the_reference():
    with open(os.path.join(GOLDEN, "hound_terrain_cfg.json")) as f:
        ref = json.load(f)
    with open(os.path.join(CFG, "task", "HoundTerrain.yaml")) as f:
        _same(yaml.safe_load(f), ref["task"], "task")
    with open(os.path.join(CFG, "train", "HoundTerrainPPO.yaml")) as f:
        _same(yaml.safe_load(f), ref["train"], "train")
    from isaacgymenv_amd.isaacgymenvs.config import compose
    c = compose("config", ["task=HoundTerrain", "num_envs=64", "sim_device=cuda:0"])
    _resolved_leaves(c["task"], ref["task"], "task")
    _resolved_leaves(c["train"], ref["train"], "train")
    t = c["task"]
    assert t["name"] == "HoundTerrain" and t["env"]["numEnvs"] == 64 and t["sim"]["use_gpu_pipeline"] is True
    assert t["env"]["randomCommandVelocityRanges"] == {"linear_x": [-2.0, 2.0], "linear_y": [-1.0, 1.0],
                                                       "yaw": [-1.0, 1.0]}
    assert t["env"]["urdfAsset"]["file"] == "urdf/Hound_new/Hound.urdf"
    # the reference names this task's runs UsefulHound (HoundTerrainPPO.yaml:47); kept
    assert ref["train"]["params"]["config"]["name"] == "${resolve_default:UsefulHound,${....experiment}}"
    assert c["train"]["params"]["config"]["name"] == "UsefulHound"
    assert c["train"]["params"]["config"]["num_actors"] == 64
    # and differs from AnymalTerrain's settings in nothing else
    a = compose("config", ["task=AnymalTerrain", "num_envs=64", "sim_device=cuda:0"])["train"]
    a["params"]["config"]["name"] = "UsefulHound"
    a["params"]["config"]["full_experiment_name"] = c["train"]["params"]["config"]["full_experiment_name"]
    assert a == c["train"]


def test_cpu_pipeline_is_refused_with_the_runtime_kernel_message(monkeypatch):
    """sim_device=cpu through make(): no host solver exists for this topology and the runtime-sized kernel is a GPU
    kernel; libgymsim's own message reaches the caller.  (The trimesh refusal needs a GPU sim to be asked for at all:
    tests/test_hound_terrain_gpu.py.)"""
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    with pytest.raises(RuntimeError, match="runtime-sized kernel is a GPU kernel"):
        isaacgymenvs.make(seed=0, task="HoundTerrain", num_envs=4, sim_device="cpu", rl_device="cpu", headless=True,
                          force_render=False, overrides=["pipeline=cpu"])


# ---------------------------------------------------------------- gymtask ABI 6
@pytest.fixture(scope="module")
def built():
    from isaacgymenv_amd import build
    build.build(verbose=False)


def test_gymtask_abi_is_6(built):
    from isaacgymenv_amd import gymtask
    assert gymtask.lib().gt_abi_version() == 6


def test_variant_struct_layouts_match_the_header(tmp_path):
    """gcc's sizeof / offsetof of gt_anymal_variant and gt_anymal_buffers against the ctypes mirrors
    (tests/test_abi.py's method); the variant pointer is the last field of the buffers."""
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from isaacgymenv_amd import gymtask
    mirrors = {"gt_anymal_variant": gymtask.GtAnymalVariant, "gt_anymal_buffers": gymtask.GtAnymalBuffers}
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
    B = gymtask.GtAnymalBuffers
    assert B._fields_[-1][0] == "variant" and B.variant.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(B)
    assert [f[0] for f in gymtask.GtAnymalVariant._fields_] == ["base_height_target", "knees_terminate",
                                                                "num_term_links", "term_link_idx"]


def _params_and_buffers(gymtask, num_bodies=24, hound=None, variant=None):
    p = gymtask.GtAnymalParams()
    p.num_envs, p.num_dofs, p.num_bodies = 4, 12, num_bodies
    p.num_obs = 12 + 24 + 140 + (18 + 10 if hound is not None else 12)
    b = gymtask.GtAnymalBuffers()
    b.hound = ctypes.cast(ctypes.pointer(hound), ctypes.c_void_p) if hound is not None else None
    b.variant = ctypes.cast(ctypes.pointer(variant), ctypes.c_void_p) if variant is not None else None
    return p, b


def test_variant_with_hound_is_refused(built):
    """Every gt_anymal_* entry point validates its structs before it launches anything, so the refusals need no GPU:
    a variant together with the UsefulHound extension, and a variant whose links are not contact rows."""
    from isaacgymenv_amd import gymtask
    L = gymtask.lib()
    keep = (ctypes.c_float * 64)()
    h = gymtask.GtAnymalHound()
    h.num_actions, h.num_shoulders = 18, 4
    h.eef_state = h.arm_commands = h.pos_control = h.effort_control = ctypes.addressof(keep)
    v = gymtask.AnymalTailKernels._variant_struct((0.48, True, [1, 5, 9, 13]))
    assert (v.base_height_target, v.knees_terminate, v.num_term_links, list(v.term_link_idx)) == \
        (np.float32(0.48), 1, 4, [1, 5, 9, 13])
    p, b = _params_and_buffers(gymtask, hound=h, variant=v)
    calls = {"gt_anymal_post_physics_a": lambda: L.gt_anymal_post_physics_a(p, b, None),
             "gt_anymal_post_physics_ab": lambda: L.gt_anymal_post_physics_ab(p, b, None, None),
             "gt_anymal_post_physics_b": lambda: L.gt_anymal_post_physics_b(p, b, None, None, None),
             "gt_anymal_reset_flagged": lambda: L.gt_anymal_reset_flagged(p, b, 1, None, None, None, None, 1.0, None,
                                                                         None),
             "gt_anymal_reset_observe": lambda: L.gt_anymal_reset_observe(p, b, 1, None, None, None, 1.0, None, 0, None,
                                                                         1, 0, None, None, None, None, None)}
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.gt_last_error().decode()
        assert "gt_anymal_variant" in msg and "hound" in msg, (name, msg)
    # the same structs without the variant pass the struct checks (post_a then asks for its reset_count buffer)
    p, b = _params_and_buffers(gymtask, hound=h)
    assert L.gt_anymal_post_physics_a(p, b, None) != 0 and b"reset_count" in L.gt_last_error()
    # a variant alone passes them too; one that names a link beyond the contact rows does not
    p, b = _params_and_buffers(gymtask, num_bodies=17, variant=v)
    assert L.gt_anymal_post_physics_a(p, b, None) != 0 and b"reset_count" in L.gt_last_error()
    p, b = _params_and_buffers(gymtask, num_bodies=13, variant=v)
    assert L.gt_anymal_post_physics_a(p, b, None) != 0 and b"invalid gt_anymal_variant" in L.gt_last_error()
    with pytest.raises(ValueError, match="at most 4"):
        gymtask.AnymalTailKernels._variant_struct((0.48, True, [1, 2, 3, 4, 5]))
