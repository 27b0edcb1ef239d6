"""Throughput of the Humanoid task on one GPU, the fused tail and reset against the torch tail.

    python tools/humanoid_profile.py --asset-root DIR [--asset-file nv_humanoid.model.json] [--num-envs 4096]
                                     [--steps 1000] [--warmup 100] [--runs 3] [--out profiles/humanoid_profile.json]

env-steps/s and ms per step under bench.py's timed-region rules (warm-up steps, then `steps` steps of random actions
from a pool prepared beforehand, one synchronize at each end), the two modes interleaved on the same env, `runs` runs
each.  --asset-root / --asset-file name the body (the reference's mjcf/nv_humanoid.xml or a packed model of it; the
default is the test fixture).  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(n, asset_root, asset_file):
    import isaacgymenvs
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    vec_task.EXISTING_SIM = None
    return isaacgymenvs.make(seed=42, task="Humanoid", num_envs=n, sim_device="cuda:0", rl_device="cuda:0",
                             headless=True, force_render=False,
                             overrides=[f"task.env.asset.assetRoot={asset_root}",
                                        f"task.env.asset.assetFileName={asset_file}"])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asset-root", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--asset-file", default="nv_humanoid.model.json")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "humanoid_profile.json"))
    a = ap.parse_args()
    import torch
    env = make(a.num_envs, a.asset_root, a.asset_file)
    pool = torch.empty((64, env.num_envs, env.num_actions), device="cuda:0").uniform_(-1, 1)
    tail = env._tail
    out = {"task": "Humanoid", "num_envs": a.num_envs, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "kernel_variant": int(env.sim.kernel_variant),
           "self_collision_pairs": int(env.sim.asset.flat["npair"]), "fused": [], "torch_tail": []}
    for _ in range(a.runs):  # interleaved on the same env
        for mode in ("fused", "torch_tail"):
            env._tail = tail if mode == "fused" else None
            out[mode].append(round(steps_per_s(env, pool, a.warmup, a.steps)))
    env._tail = tail
    out["ms_per_step"] = {m: [round(1e3 * a.num_envs / v, 4) for v in out[m]] for m in ("fused", "torch_tail")}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
