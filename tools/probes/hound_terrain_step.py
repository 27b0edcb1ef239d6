"""Whole-step() time of HoundTerrain at 4096 envs beside AnymalTerrain forced onto the same physics kernel
(GS_PHYSICS_KERNEL=generic: the runtime-sized kernel, kernel_variant 4), GPU box probe.

Both envs live in one process and are timed in alternating windows (A B A B ...), each window `--steps` env steps of
random actions between two device events after `--warmup` steps of both; the figure is the median window, with the
spread of the windows beside it.  Episodes end and reset inside the windows; every 50th step's reset count is
summed into the line (HoundTerrain resets far more often under random actions: thigh and shoulder contacts end its
episodes).  One JSON line per task, and a summary line with the ratio.
    python tools/probes/hound_terrain_step.py [--envs 4096] [--steps 200] [--windows 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def make(task, n, kernel):
    import torch
    import isaacgymenvs
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    vec_task.EXISTING_SIM = None
    if kernel:
        os.environ["GS_PHYSICS_KERNEL"] = kernel
    else:
        os.environ.pop("GS_PHYSICS_KERNEL", None)
    torch.manual_seed(42)
    env = isaacgymenvs.make(seed=42, task=task, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                            force_render=False)
    os.environ.pop("GS_PHYSICS_KERNEL", None)
    return env


def window(env, acts, steps):
    import torch
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    resets = 0
    e0.record(s)
    for i in range(steps):
        _, _, reset, _ = env.step(acts[i % len(acts)])
        resets += int(reset.sum()) if i % 50 == 49 else 0  # (a sync every 50 steps: the count of that step only)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps, resets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    n = a.envs
    envs = {"HoundTerrain": make("HoundTerrain", n, None),
            "AnymalTerrain[generic]": make("AnymalTerrain", n, "generic")}
    for name, env in envs.items():
        assert env.sim.kernel_variant == 4, (name, env.sim.kernel_variant)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    acts = [2 * torch.rand((n, 12), device="cuda:0", generator=gen) - 1 for _ in range(16)]
    for env in envs.values():
        window(env, acts, a.warmup)
    ms = {k: [] for k in envs}
    rs = {k: 0 for k in envs}
    for _ in range(a.windows):
        for name, env in envs.items():
            t, r = window(env, acts, a.steps)
            ms[name].append(t)
            rs[name] += r
    lines = []
    for name, env in envs.items():
        med = statistics.median(ms[name])
        lines.append({"task": name, "envs": n, "kernel_variant": env.sim.kernel_variant,
                      "self_collide": bool(env.sim.self_collide), "steps_per_window": a.steps, "windows": a.windows,
                      "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[name]), 4),
                      "ms_per_step_max": round(max(ms[name]), 4), "env_steps_per_s_median": round(n / med * 1e3),
                      "resets_seen_in_sampled_steps": rs[name]})
    h, an = (statistics.median(ms[k]) for k in envs)
    lines.append({"summary": "HoundTerrain step() over AnymalTerrain step() on the runtime-sized kernel",
                  "ratio_of_medians": round(h / an, 3)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
