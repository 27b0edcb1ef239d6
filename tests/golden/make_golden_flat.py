#!/usr/bin/env python3
"""Generate tests/golden/anymal_flat.npz, hound_flat.npz and flat_cfg.json from the REFERENCE (dev container only).

anymal_flat.npz / hound_flat.npz: the reference's tasks/anymal.py and tasks/hound.py driven through
tests/fakegym_flat.FlatFakeGym, 32 envs x 30 steps with 20-step episodes (episodeLength_s 0.4) and
torqueRewardScale -1e-4 (-2.5e-5 in the task's config), so the fake's large DOF forces push the reward below its
clip at 0.  Per step: what the step returns, and the tail's inputs at compute_observations entry (after reset_idx and
the four refreshes) and outputs, as make_golden_hound_terrain.py stores them; the reset's inputs (flagged envs, RNG
state) and the dof / root state and commands it leaves.  The generator asserts the cases the fixture must hold
(fakegym_flat.assert_fixture_conditions).

flat_cfg.json: yaml.safe_load of the reference's Anymal.yaml, Hound.yaml, AnymalPPO.yaml and HoundPPO.yaml (resolver
strings stay strings).

    python tests/golden/make_golden_flat.py
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

N_ENVS, STEPS = 32, 30
TORQUE_REWARD_SCALE = -1.0e-4


def flat_cfg(task: str, num_envs: int) -> dict:
    from isaacgymenv_amd.isaacgymenvs.config import compose
    cfg = compose("config", [f"task={task}", f"num_envs={num_envs}", "sim_device=cpu", "pipeline=cpu"])["task"]
    cfg["env"]["learn"]["episodeLength_s"] = 0.4
    cfg["env"]["learn"]["torqueRewardScale"] = TORQUE_REWARD_SCALE
    return cfg


def record(kind: str, num_envs=N_ENVS, steps=STEPS):
    from tests.fakegym_flat import FAKE_KW, TASKS, FlatFakeGym
    task = TASKS[kind][0]
    fake = FlatFakeGym(**FAKE_KW[kind])
    mg.install_reference_stubs(fake)
    ref = importlib.import_module("isaacgymenvs.tasks." + kind)
    cfg = flat_cfg(task, num_envs)
    _np = mg._np
    torch.manual_seed(42)
    env = getattr(ref, task)(copy.deepcopy(cfg), "cpu", "cpu", -1, True, False, False)
    out = {"init_commands": _np(env.commands), "init_dof_state": _np(env.dof_state),
           "init_reset": _np(env.reset_buf), "init_progress": _np(env.progress_buf),
           "knee_indices": _np(env.knee_indices), "feet_indices": _np(env.feet_indices),
           "base_index": np.array(int(env.base_index)), "max_episode_length": np.array(int(env.max_episode_length)),
           "default_dof_pos": _np(env.default_dof_pos[0]), "initial_root_states": _np(env.initial_root_states),
           "rew_scales": np.array([env.rew_scales[k] for k in ("lin_vel_xy", "ang_vel_z", "torque")])}
    rng = np.random.RandomState(7)
    actions = (2.4 * rng.rand(steps, num_envs, 12) - 1.2).astype(np.float32)  # beyond clipActions = 1
    names = ("obs", "rew", "reset", "time_outs", "progress", "commands", "dof_state", "root_states", "targets",
             "reset_count_in", "in_reset", "in_rng_state", "in_root", "in_dof", "in_contact", "in_torques", "in_actions",
             "in_commands", "in_progress", "out_obs", "out_rew", "out_reset", "out_rng_state")
    recs = {k: [] for k in names}
    orig_obs, orig_post = env.compute_observations, env.post_physics_step

    def traced_obs():
        for refresh in (env.gym.refresh_dof_state_tensor, env.gym.refresh_actor_root_state_tensor,
                        env.gym.refresh_net_contact_force_tensor, env.gym.refresh_dof_force_tensor):
            refresh(env.sim)
        for key, ten in (("in_root", env.root_states), ("in_dof", env.dof_state), ("in_contact", env.contact_forces),
                         ("in_torques", env.torques), ("in_actions", env.actions), ("in_commands", env.commands),
                         ("in_progress", env.progress_buf)):
            recs[key].append(_np(ten))
        recs["out_rng_state"].append(torch.get_rng_state().numpy().copy())  # where reset_idx left the generator
        orig_obs()

    def traced_post():
        recs["in_reset"].append(_np(env.reset_buf))
        recs["reset_count_in"].append(int((env.reset_buf != 0).sum()))
        recs["in_rng_state"].append(torch.get_rng_state().numpy().copy())
        orig_post()
        for key, ten in (("out_obs", env.obs_buf), ("out_rew", env.rew_buf), ("out_reset", env.reset_buf)):
            recs[key].append(_np(ten))

    env.compute_observations = traced_obs
    env.post_physics_step = traced_post
    for t in range(steps):
        obs, rew, reset, extras = env.step(torch.from_numpy(actions[t]))
        assert reset.dtype == torch.int64
        recs["obs"].append(_np(obs["obs"]))
        recs["rew"].append(_np(rew))
        recs["reset"].append(_np(reset))
        recs["time_outs"].append(_np(extras["time_outs"]).astype(np.int64))
        recs["progress"].append(_np(env.progress_buf))
        recs["commands"].append(_np(env.commands))
        recs["dof_state"].append(_np(env.dof_state))
        recs["root_states"].append(_np(env.root_states))
        recs["targets"].append(_np(env.sim.ptgt))
    for k, v in recs.items():
        out[k] = np.stack([np.asarray(x) for x in v])
    out["actions"] = actions
    out["cfg_yaml"] = np.array(yaml.safe_dump(cfg))
    return out


def parsed_reference_configs():
    cfg_dir = os.path.join(mg.REF, "isaacgymenvs", "cfg")
    out = {}
    for key, rel in (("Anymal", "task/Anymal.yaml"), ("Hound", "task/Hound.yaml"), ("AnymalPPO", "train/AnymalPPO.yaml"),
                     ("HoundPPO", "train/HoundPPO.yaml")):
        with open(os.path.join(cfg_dir, rel)) as f:
            out[key] = yaml.safe_load(f)
    return out


def main():
    from tests.fakegym_flat import TASKS, assert_fixture_conditions
    with open(os.path.join(HERE, "flat_cfg.json"), "w") as f:
        json.dump(parsed_reference_configs(), f, indent=1, sort_keys=True)
        f.write("\n")
    if len(sys.argv) < 2:  # one process per robot: the reference's modules bind the fake they were imported with
        import subprocess
        for kind in TASKS:
            subprocess.run([sys.executable, os.path.abspath(__file__), kind], check=True)
        return
    for kind in sys.argv[1:2]:
        d = record(kind)
        print(kind, "cases:", assert_fixture_conditions(d))
        path = os.path.join(HERE, TASKS[kind][1])
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
