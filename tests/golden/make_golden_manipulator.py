#!/usr/bin/env python3
"""Generate tests/golden/manipulator.npz and manipulator_cfg.json from the REFERENCE (dev container only).

manipulator.npz: the reference's tasks/manipulator.py driven through tests/manip_cases.ManipFakeGym (the packed
Franka: 8 bodies panda_link0..7, 7 dofs with the URDF's limits and efforts, -1 for the gripper bodies the truncated
URDF does not hold; a synthetic SPD M [N, 7, 7] and J [N, 8, 6, 7]), 32 envs x 30 steps with 12-step episodes and
frankaDofNoise 3.0 (0.25 in the task's config), so the reset's clamp engages on both bounds of a joint.  progress_buf
is staggered once after construction, and before each step every fourth env's command is put within 0.02 of its
end-effector.  Per step: what the step returns; the control inputs (actions, the panda_joint7 Jacobian row, the mass
matrix, the end-effector row, the dof state) and the effort tensor they produce, with the float64 restatement of the
controller on the same inputs; the flagged envs and the generator state before the reset, the commands and dof state
after it; the tail's inputs at compute_observations entry (after reset_idx and the refreshes).  The generator asserts
the cases the fixture must hold (manip_cases.assert_fixture_conditions), among them that two float64 algorithms for the
restatement agree to 1e-8 on the recorded inputs.

manipulator_cfg.json: yaml.safe_load of the reference's Manipulator.yaml and ManipulatorPPO.yaml (resolver strings
stay strings).

    python tests/golden/make_golden_manipulator.py
"""
from __future__ import annotations

import copy
import importlib
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)


def record():
    from tests import manip_cases as A
    fake = A.ManipFakeGym(seed=A.FAKE_SEED)
    mg.install_reference_stubs(fake)
    ref = importlib.import_module("isaacgymenvs.tasks.manipulator")
    cfg = A.fixture_cfg(A.N_ENVS)
    _np = mg._np
    torch.manual_seed(42)
    env = ref.Manipulator(A.point_at_fixture(copy.deepcopy(cfg)), "cpu", "cpu", -1, True, False, False)
    n = env.num_envs
    A.stagger(env)
    out = {"init_commands": _np(env.commands), "init_dof_state": _np(env._dof_state),
           "init_reset": _np(env.reset_buf), "init_progress": _np(env.progress_buf),
           "eef_index": np.array(int(env.handles["endpoint_tip"])),
           "max_episode_length": np.array(int(env.max_episode_length)),
           "dof_lower": _np(env.franka_dof_lower_limits), "dof_upper": _np(env.franka_dof_upper_limits),
           "effort_limits": _np(env._franka_effort_limits), "kd": _np(env.kd), "kd_null": _np(env.kd_null)}
    rng = np.random.RandomState(7)
    actions = (2.4 * rng.rand(A.STEPS, n, 6) - 1.2).astype(np.float32)  # beyond clipActions = 1
    names = ("obs", "rew", "reset", "time_outs", "progress", "commands", "dof_state", "torques", "torques64",
             "ctl_actions", "ctl_jac", "ctl_mm", "ctl_eef", "ctl_dof", "reset_count_in", "in_reset", "in_rng_state",
             "in_eef", "in_commands", "in_progress", "in_reset_buf")
    recs = {k: [] for k in names}
    orig_obs, orig_post, orig_pre = env.compute_observations, env.post_physics_step, env.pre_physics_step

    def traced_pre(a):
        for key, ten in (("ctl_jac", env._j_eef), ("ctl_mm", env._mm), ("ctl_eef", env._eef_state),
                         ("ctl_dof", env._dof_state.view(n, 7, 2))):
            recs[key].append(_np(ten))
        recs["ctl_actions"].append(_np(a))
        orig_pre(a)
        recs["torques"].append(_np(env._effort_control))
        recs["torques64"].append(A.osc_float64(recs["ctl_actions"][-1], recs["ctl_jac"][-1], recs["ctl_mm"][-1],
                                               recs["ctl_eef"][-1], recs["ctl_dof"][-1], out["effort_limits"],
                                               action_scale=env.action_scale))

    def traced_obs():
        env._refresh()
        for key, ten in (("in_eef", env._eef_state), ("in_commands", env.commands), ("in_progress", env.progress_buf),
                         ("in_reset_buf", env.reset_buf)):
            recs[key].append(_np(ten))
        return orig_obs()

    def traced_post():
        recs["in_reset"].append(_np(env.reset_buf))
        recs["reset_count_in"].append(int((env.reset_buf != 0).sum()))
        recs["in_rng_state"].append(torch.get_rng_state().numpy().copy())
        orig_post()

    env.compute_observations, env.post_physics_step, env.pre_physics_step = traced_obs, traced_post, traced_pre
    for t in range(A.STEPS):
        A.place_commands(env, "_eef_state")
        obs, rew, reset, extras = env.step(torch.from_numpy(actions[t]))
        assert reset.dtype == torch.int64
        recs["obs"].append(_np(obs["obs"]))
        recs["rew"].append(_np(rew))
        recs["reset"].append(_np(reset))
        recs["time_outs"].append(_np(extras["time_outs"]).astype(np.int64))
        recs["progress"].append(_np(env.progress_buf))
        recs["commands"].append(_np(env.commands))
        recs["dof_state"].append(_np(env._dof_state.view(n, 7, 2)))
    for k, v in recs.items():
        out[k] = np.stack([np.asarray(x) for x in v])
    out["final_rng_state"] = torch.get_rng_state().numpy().copy()
    out["actions"] = actions
    out["cfg_yaml"] = np.array(yaml.safe_dump(cfg))
    return out


def parsed_reference_configs():
    cfg_dir = os.path.join(mg.REF, "isaacgymenvs", "cfg")
    out = {}
    for key, rel in (("task", "task/Manipulator.yaml"), ("train", "train/ManipulatorPPO.yaml")):
        with open(os.path.join(cfg_dir, rel)) as f:
            out[key] = yaml.safe_load(f)
    return out


def main():
    from tests.manip_cases import assert_fixture_conditions
    with open(os.path.join(HERE, "manipulator_cfg.json"), "w") as f:
        json.dump(parsed_reference_configs(), f, indent=1, sort_keys=True)
        f.write("\n")
    d = record()
    print("cases:", assert_fixture_conditions(d))
    path = os.path.join(HERE, "manipulator.npz")
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
