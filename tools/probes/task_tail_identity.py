"""Bit identity of the task tails (libgymtask's kernels and their Python drivers in isaacgymenv_amd/gymtask.py) across
a change that must not touch a result: one sha256 line per task over the buffers the tail writes, after 40 env steps.

    python tools/probes/task_tail_identity.py [--n 130] [--steps 40] [--tasks Ant,Anymal,...]

Run it from a checkout of each of the two commits (the drivers are Python, so another library file alone is not
enough) and compare the lines: same kernels, same inputs, so every line must be equal.  Every task runs from seed 42
with a fixed action pattern and an episode shortened through the config to 10 steps, so four time-out resets (and
whatever the actions make fall) lie inside the run; AnymalTerrain runs on the plane and on the trimesh with the
curriculum on.  Hashed: obs_buf, rew_buf, reset_buf, progress_buf, dof_state, root_states, commands (where the task
has them), the driver's reset_masks and reset_count (its last word is the last done count) and the device generator's
final offset.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHORT = {"task.env.learn.episodeLength_s": 0.2}  # 10 steps of 0.02 s
TRIMESH = {"task.env.terrain.terrainType": "trimesh", "task.env.terrain.numLevels": 4, "task.env.terrain.numTerrains": 8,
           "task.env.terrain.curriculum": True}
TASKS = {"Ant": ("Ant", {"task.env.episodeLength": 10}), "Anymal": ("Anymal", SHORT), "Hound": ("Hound", SHORT),
         "AnymalTerrain_plane": ("AnymalTerrain", SHORT), "AnymalTerrain_trimesh": ("AnymalTerrain", dict(SHORT, **TRIMESH)),
         "UsefulHound": ("UsefulHound", SHORT), "HoundTerrain": ("HoundTerrain", SHORT)}
FIELDS = ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "dof_state", "root_states", "commands")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run(name, n, steps):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    import isaacgymenvs
    task, over = TASKS[name]
    vec_task.EXISTING_SIM = None
    torch.manual_seed(42)
    np.random.seed(42)  # the terrain tiles are drawn from numpy's global generator, which make() leaves alone
    env = isaacgymenvs.make(seed=42, task=task, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                            force_render=False, overrides=[f"{k}={v}" for k, v in over.items()])
    na = env.num_actions
    i = torch.arange(n * na, dtype=torch.float32, device="cuda:0").reshape(n, na)
    resets = 0
    for k in range(steps):
        _, _, done, _ = env.step(torch.sin(0.37 * i + 0.9 * k))
        resets += int(done.sum())
    torch.cuda.synchronize()
    drv = getattr(env, "_tail", None) or env._kernels
    parts = [f"{f} {sha(getattr(env, f))}" for f in FIELDS if hasattr(env, f)]
    parts += [f"reset_masks {sha(drv.reset_masks)}", f"reset_count {drv.reset_count.tolist()}",
              f"offset {torch.cuda.default_generators[0].get_offset()}"]
    return f"max_episode_length {env.max_episode_length} dones {resets} " + " ".join(parts)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=130)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--tasks", default=",".join(TASKS))
    a = ap.parse_args()
    for name in a.tasks.split(","):
        print(f"n={a.n} steps={a.steps} {name}: {run(name, a.n, a.steps)}", flush=True)
