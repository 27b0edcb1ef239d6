#!/usr/bin/env python3
"""Generate tests/golden/hound_terrain.npz, hound_terrain_tail.npz and hound_terrain_cfg.json from the REFERENCE
(dev container only).

hound_terrain.npz + hound_terrain_tail.npz (one recording; load_fixture in tests/fakegym_hound.py joins them): the
reference's Hound_terrain.py driven through tests/fakegym_hound.HoundFakeGym, recorded with the fields of
make_golden.record_anymal plus base_indices / base_index / max_episode_length / default_dof_pos.  32 envs x 30 steps
with a push every 5 steps, 20-step episodes, and baseHeightRewardScale -5.0 (0 in the task's config, where the 0.48 m
target could not show).  The generator asserts the cases the fixture must hold (fakegym_hound.assert_fixture_conditions).

hound_terrain_cfg.json: yaml.safe_load of the reference's HoundTerrain.yaml and HoundTerrainPPO.yaml (resolver
strings stay strings).

    python tests/golden/make_golden_hound_terrain.py
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


def hound_terrain_cfg(num_envs: int) -> dict:
    from isaacgymenv_amd.isaacgymenvs.config import compose
    cfg = compose("config", ["task=HoundTerrain", f"num_envs={num_envs}", "sim_device=cpu", "pipeline=cpu"])["task"]
    learn = cfg["env"]["learn"]
    learn["pushInterval_s"] = 0.1
    learn["episodeLength_s"] = 0.4
    learn["baseHeightRewardScale"] = -5.0
    return cfg


def record(num_envs=N_ENVS, steps=STEPS):
    from tests.fakegym_hound import HoundFakeGym
    fake = HoundFakeGym()
    mg.install_reference_stubs(fake)
    ref = importlib.import_module("isaacgymenvs.tasks.Hound_terrain")
    cfg = hound_terrain_cfg(num_envs)
    _np = mg._np
    torch.manual_seed(42)
    env = ref.HoundTerrain(copy.deepcopy(cfg), "cpu", "cpu", -1, True, False, False)
    out = {"init_commands": _np(env.commands), "init_dof_state": _np(env.dof_state),
           "init_root_states": _np(env.root_states), "feet_indices": _np(env.feet_indices),
           "knee_indices": _np(env.knee_indices), "base_indices": _np(env.base_indices),
           "base_index": np.array(int(env.base_index)), "max_episode_length": np.array(int(env.max_episode_length)),
           "noise_scale_vec": _np(env.noise_scale_vec), "default_dof_pos": _np(env.default_dof_pos[0])}
    rng = np.random.RandomState(7)
    actions = (2 * rng.rand(steps, num_envs, 12) - 1).astype(np.float32)
    terms = list(env.episode_sums.keys())
    names_in = ("in_root", "in_contact", "in_dof", "in_torques", "in_actions", "in_last_actions", "in_last_dof_vel",
                "in_commands", "in_feet_air_time", "in_progress", "in_episode_sums", "in_timeout", "in_timeout_is_long",
                "in_rng_state", "in_push")
    names_out = ("out_root", "out_dof", "out_last_actions", "out_last_dof_vel", "out_base_lin_vel", "out_base_ang_vel",
                 "out_projected_gravity")
    names_step = ("obs", "rew", "reset", "time_outs", "commands", "feet_air_time", "progress", "episode_sums",
                  "ep_extras", "ep_mask")
    recs = {k: [] for k in names_in + names_out + names_step}
    sums = lambda: np.stack([_np(env.episode_sums[k]) for k in terms])  # noqa: E731
    orig_post = env.post_physics_step

    def traced_post():
        sim = env.sim
        for key, val in (("in_root", _np(sim.root)), ("in_contact", _np(sim.cf).reshape(num_envs, -1, 3)),
                         ("in_dof", _np(env.dof_state)), ("in_torques", _np(env.torques)),
                         ("in_actions", _np(env.actions)), ("in_last_actions", _np(env.last_actions)),
                         ("in_last_dof_vel", _np(env.last_dof_vel)), ("in_commands", _np(env.commands)),
                         ("in_feet_air_time", _np(env.feet_air_time)), ("in_progress", _np(env.progress_buf)),
                         ("in_episode_sums", sums()), ("in_timeout", _np(env.timeout_buf).astype(np.int64)),
                         ("in_timeout_is_long", int(env.timeout_buf.dtype == torch.int64)),
                         ("in_rng_state", torch.get_rng_state().numpy().copy()),
                         ("in_push", int((env.common_step_counter + 1) % env.push_interval == 0))):
            recs[key].append(val)
        env.extras.pop("episode", None)
        orig_post()
        for key, ten in (("out_root", env.root_states), ("out_dof", env.dof_state),
                         ("out_last_actions", env.last_actions), ("out_last_dof_vel", env.last_dof_vel),
                         ("out_base_lin_vel", env.base_lin_vel), ("out_base_ang_vel", env.base_ang_vel),
                         ("out_projected_gravity", env.projected_gravity)):
            recs[key].append(_np(ten))

    env.post_physics_step = traced_post
    for t in range(steps):
        obs, rew, reset, extras = env.step(torch.from_numpy(actions[t]))
        assert reset.dtype == torch.bool
        recs["obs"].append(_np(obs["obs"]))
        recs["rew"].append(_np(rew))
        recs["reset"].append(_np(reset).astype(np.int64))
        recs["time_outs"].append(_np(extras["time_outs"]).astype(np.int64))
        recs["commands"].append(_np(env.commands))
        recs["feet_air_time"].append(_np(env.feet_air_time))
        recs["progress"].append(_np(env.progress_buf))
        recs["episode_sums"].append(sums())
        ep = extras.get("episode")
        recs["ep_mask"].append(int(ep is not None))
        recs["ep_extras"].append(np.array([float(ep["rew_" + k]) for k in terms] + [float(ep["terrain_level"])])
                                 if ep is not None else np.zeros(len(terms) + 1))
    for k, v in recs.items():
        out[k] = np.stack([np.asarray(x) for x in v])
    out["actions"] = actions
    out["terms"] = np.array(terms)
    out["cfg_yaml"] = np.array(yaml.safe_dump(cfg))
    return out


def parsed_reference_configs():
    cfg_dir = os.path.join(mg.REF, "isaacgymenvs", "cfg")
    with open(os.path.join(cfg_dir, "task", "HoundTerrain.yaml")) as f:
        task = yaml.safe_load(f)
    with open(os.path.join(cfg_dir, "train", "HoundTerrainPPO.yaml")) as f:
        train = yaml.safe_load(f)
    return {"task": task, "train": train}


def main():
    from tests.fakegym_hound import assert_fixture_conditions
    with open(os.path.join(HERE, "hound_terrain_cfg.json"), "w") as f:
        json.dump(parsed_reference_configs(), f, indent=1, sort_keys=True)
        f.write("\n")
    d = record()
    print("hound_terrain.npz cases:", assert_fixture_conditions(d))
    # two files, each below the repository's 1 MiB limit for a committed file: the tail's per-step inputs and
    # outputs (in_* / out_*, read by the GPU tail tests) apart from everything else
    tail = {k: v for k, v in d.items() if k.startswith(("in_", "out_"))}
    rest = {k: v for k, v in d.items() if k not in tail}
    for name, part in (("hound_terrain.npz", rest), ("hound_terrain_tail.npz", tail)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        print(name, os.path.getsize(path), {k: v.shape for k, v in part.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    main()
