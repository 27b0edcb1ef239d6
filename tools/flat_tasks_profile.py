"""Throughput of the flat-ground tasks (Anymal, Hound) and what their new pieces cost, on one GPU.

    python tools/flat_tasks_profile.py [--num-envs 4096] [--steps 1000] [--warmup 100] [--runs 3] [--out FILE]

1. env-steps/s of each task under bench.py's timed-region rules (warm-up steps, then `steps` steps of random actions
   from a pool prepared beforehand, one synchronize at each end), the fused tail and reset against the torch tail of
   the same task, interleaved, `runs` runs each;
2. the same for AnymalTerrain with GS_PHYSICS_KERNEL=lane (kernel_variant 1), the yardstick of a drive-carrying sim;
3. the bound DOF-force store on the one-env-per-lane ANYmal kernel: HIP-event time of 1000 gym.simulate launches
   with the tensor bound against unbound (the unbound sim launches the kernel without the store).
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(task, n):
    import isaacgymenvs
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    vec_task.EXISTING_SIM = None
    return isaacgymenvs.make(seed=42, task=task, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                             force_render=False)


def steps_per_s(env, pool, warmup, steps):
    import torch
    n = env.num_envs
    for i in range(warmup):
        env.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        env.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0)


def simulate_ms(bound, n, launches):
    """Mean HIP-event time of one gym.simulate of ANYmal with the flat task's drive gains (one env per lane)."""
    import numpy as np
    import torch
    from tests import helpers as H
    drives = (np.full(12, 1, dtype=np.int32), np.full(12, 85.0), np.full(12, 2.0))
    gym, sim = H.make_gpu_sim("anymal", n, dict(H.ANYMAL_PARAMS, dt=0.02, substeps=2), drives=drives)
    root, dof, tau, mu = H.anymal_states(n, seed=3)
    H.load_state_into(sim, root, dof, mu)
    if bound:
        gym.acquire_dof_force_tensor(sim)
    assert sim.kernel_variant == 1
    state0 = sim.state.clone()
    for _ in range(20):
        gym.simulate(sim)
    sim.state.copy_(state0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        gym.simulate(sim)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    out = {"num_envs": a.num_envs, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for task in ("Anymal", "Hound"):
        env = make(task, a.num_envs)
        pool = torch.empty((64, env.num_envs, env.num_actions), device="cuda:0").uniform_(-1, 1)
        tail = env._tail
        res = {"kernel_variant": int(env.sim.kernel_variant), "fused": [], "torch_tail": []}
        for _ in range(a.runs):  # interleaved on the same env
            for mode in ("fused", "torch_tail"):
                env._tail = tail if mode == "fused" else None
                res[mode].append(round(steps_per_s(env, pool, a.warmup, a.steps)))
        env._tail = tail
        out[task] = res
        del env
    os.environ["GS_PHYSICS_KERNEL"] = "lane"
    env = make("AnymalTerrain", a.num_envs)
    pool = torch.empty((64, env.num_envs, env.num_actions), device="cuda:0").uniform_(-1, 1)
    out["AnymalTerrain_lane"] = {"kernel_variant": int(env.sim.kernel_variant),
                                 "fused": [round(steps_per_s(env, pool, a.warmup, a.steps)) for _ in range(a.runs)]}
    del env
    os.environ.pop("GS_PHYSICS_KERNEL")
    ms = {"unbound": [], "bound": []}
    for _ in range(a.runs):  # interleaved
        for mode in ("unbound", "bound"):
            ms[mode].append(round(simulate_ms(mode == "bound", a.num_envs, a.launches), 4))
    out["anymal_lane_simulate_ms"] = ms
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
