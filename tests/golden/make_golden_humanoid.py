#!/usr/bin/env python3
"""Generate tests/golden/humanoid.npz and humanoid_cfg.json from the REFERENCE (dev container only).

humanoid.npz: the reference's tasks/humanoid.py driven through tests/humanoid_cases.HumanoidFakeGym, 32 envs x 30
steps with 12-step episodes staggered once (after the first step, which resets every env).  Ant's schema
(make_golden.py record_ant): per step what the step returns (its observations, rewards and resets are the tail's outputs), the tail's inputs at compute_observations entry
(after reset_idx and the refreshes; the DOF force tensor is one more input here, the action input is the clipped
action) and its outputs; and for the reset: the flagged envs at post_physics_step entry and the two torch_rand_float
draws; the generator's final state.  The generator
asserts the cases the fixture must hold (humanoid_cases.assert_fixture_conditions).

humanoid_cfg.json: yaml.safe_load of the reference's Humanoid.yaml and HumanoidPPO.yaml (resolver strings stay
strings).

    python tests/golden/make_golden_humanoid.py
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
    from tests import humanoid_cases as HC
    fake = HC.HumanoidFakeGym(seed=HC.FAKE_SEED)
    mg.install_reference_stubs(fake)
    ref = importlib.import_module("isaacgymenvs.tasks.humanoid")
    cfg = HC.fixture_cfg(HC.N_ENVS)
    _np = mg._np
    n, nd = HC.N_ENVS, HC.ND
    torch.manual_seed(42)
    env = ref.Humanoid(copy.deepcopy(cfg), "cpu", "cpu", -1, True, False, False)
    out = {"motor_efforts": _np(env.motor_efforts), "max_motor_effort": np.array(float(env.max_motor_effort)),
           "dof_limits_lower": _np(env.dof_limits_lower), "dof_limits_upper": _np(env.dof_limits_upper),
           "initial_dof_pos": _np(env.initial_dof_pos), "initial_root_states": _np(env.initial_root_states),
           "termination_height": np.array(float(env.termination_height)),
           "max_episode_length": np.array(int(env.max_episode_length)), "num_bodies": np.array(int(env.num_bodies)),
           "num_dof": np.array(int(env.num_dof))}
    rng = np.random.RandomState(17)
    actions = (2.4 * rng.rand(HC.STEPS, n, nd) - 1.2).astype(np.float32)  # beyond clipActions = 1
    # (kept under the size limit for a committed file: what a step returns is its tail's outputs, the tail's action
    # input is the clipped action, and of the generator only the final state is stored -- the draws pin the rest)
    names = ("time_outs", "progress", "reset_count_in", "in_reset", "draw_positions", "draw_velocities",
             "in_root", "in_dof", "in_sensors", "in_dof_force", "in_potentials", "in_progress",
             "in_reset_tail", "out_obs", "out_rew", "out_reset", "out_potentials", "out_prev_potentials", "out_up_vec",
             "out_heading_vec")
    recs = {k: [] for k in names}
    orig_obs, orig_post, orig_rand = env.compute_observations, env.post_physics_step, ref.torch_rand_float
    draws = []

    def traced_rand(lower, upper, shape, device):
        u = orig_rand(lower, upper, shape, device)
        draws.append(_np(u))
        return u

    ref.torch_rand_float = traced_rand

    def traced_obs():
        for refresh in (env.gym.refresh_dof_state_tensor, env.gym.refresh_actor_root_state_tensor,
                        env.gym.refresh_force_sensor_tensor, env.gym.refresh_dof_force_tensor):
            refresh(env.sim)
        for key, ten in (("in_root", env.root_states), ("in_dof", env.dof_state), ("in_sensors", env.vec_sensor_tensor),
                         ("in_dof_force", env.dof_force_tensor),
                         ("in_potentials", env.potentials), ("in_progress", env.progress_buf),
                         ("in_reset_tail", env.reset_buf)):
            recs[key].append(_np(ten))
        assert torch.equal(env.actions, torch.clamp(torch.from_numpy(actions[len(recs["in_root"]) - 1]), -1.0, 1.0))
        orig_obs()

    def traced_post():
        del draws[:]
        recs["in_reset"].append(_np(env.reset_buf))
        recs["reset_count_in"].append(int((env.reset_buf != 0).sum()))
        orig_post()
        pos, vel = np.full((n, nd), np.nan, np.float32), np.full((n, nd), np.nan, np.float32)
        if draws:  # the two draws of reset_idx, [k, 21] each, padded to [n, 21]
            pos[:len(draws[0])], vel[:len(draws[1])] = draws[0], draws[1]
        recs["draw_positions"].append(pos)
        recs["draw_velocities"].append(vel)
        for key, ten in (("out_obs", env.obs_buf), ("out_rew", env.rew_buf), ("out_reset", env.reset_buf),
                         ("out_potentials", env.potentials), ("out_prev_potentials", env.prev_potentials),
                         ("out_up_vec", env.up_vec), ("out_heading_vec", env.heading_vec)):
            recs[key].append(_np(ten))

    env.compute_observations = traced_obs
    env.post_physics_step = traced_post
    for t in range(HC.STEPS):
        if t == HC.STAGGER_STEP:
            HC.stagger(env)
        obs, rew, reset, extras = env.step(torch.from_numpy(actions[t]))
        assert reset.dtype == torch.int64
        assert np.array_equal(_np(obs["obs"]), recs["out_obs"][-1]) and np.array_equal(_np(rew), recs["out_rew"][-1])
        assert np.array_equal(_np(reset), recs["out_reset"][-1]) and np.array_equal(_np(env.dof_state), recs["in_dof"][-1])
        recs["time_outs"].append(_np(extras["time_outs"]).astype(np.int64))
        recs["progress"].append(_np(env.progress_buf))
    for k, v in recs.items():
        out[k] = np.stack([np.asarray(x) for x in v])
    out["actions"] = actions
    out["final_rng_state"] = torch.get_rng_state().numpy().copy()
    out["cfg_yaml"] = np.array(yaml.safe_dump(cfg))
    return out


def parsed_reference_configs():
    cfg_dir = os.path.join(mg.REF, "isaacgymenvs", "cfg")
    out = {}
    for key, rel in (("task", "task/Humanoid.yaml"), ("train", "train/HumanoidPPO.yaml")):
        with open(os.path.join(cfg_dir, rel)) as f:
            out[key] = yaml.safe_load(f)
    return out


def main():
    from tests import humanoid_cases as HC
    with open(os.path.join(HERE, "humanoid_cfg.json"), "w") as f:
        json.dump(parsed_reference_configs(), f, indent=1, sort_keys=True)
        f.write("\n")
    d = record()
    print("cases:", HC.assert_fixture_conditions(d))
    path = os.path.join(HERE, "humanoid.npz")
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
