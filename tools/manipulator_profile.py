"""Throughput of the Manipulator task on one GPU, and of its lane-team controller against the one-env-per-lane one.

    python tools/manipulator_profile.py [--asset-root DIR] [--asset-file FILE] [--num-envs 8192] [--steps 1000]
                                        [--warmup 100] [--runs 3] [--launches 200] [--out FILE]

Whole step: the protocol of tools/houndarm_profile.py: warm-up steps, then `steps` steps of
random actions from a pool prepared beforehand, one synchronize at each end, `runs` runs of each mode (fused kernels,
torch path) interleaved on the same env.

Controller alone, by device events around `launches` back-to-back launches on one set of random well-conditioned inputs
at --num-envs envs: gt_arm_control (one env per lane, 6 dofs), gt_osc_control at nd = 6 on the same inputs, and
gt_osc_control at nd = 7, the three interleaved over `--ctl-runs` rounds; reported as the median microseconds per
launch with the smallest and largest round (the spread).  The arm's model is not shipped with the package:
--asset-root / --asset-file name the reference's URDF or a packed *.model.json of it
(tests/golden/franka_panda_manipulator.model.json by default).  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.flat_tasks_profile import steps_per_s  # noqa: E402


def make(n, asset_root, asset_file):
    import isaacgymenvs
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    vec_task.EXISTING_SIM = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the fixed-base self-collision deviation)
        return isaacgymenvs.make(seed=42, task="Manipulator", num_envs=n, sim_device="cuda:0", rl_device="cuda:0",
                                 headless=True, force_render=False,
                                 overrides=[f"task.env.asset.assetRoot={asset_root}",
                                            f"task.env.asset.assetFileNameFranka={asset_file}"])


def controller_times(n, launches, rounds):
    """{name: [microseconds per launch, one per round]} of the three controller launches, interleaved."""
    import torch
    from isaacgymenv_amd import gymtask
    from isaacgymenv_amd._stream import raw_stream
    L = gymtask.lib()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    stream = ctypes.c_void_p(raw_stream(dev))
    cases = {}
    for nd in (6, 7):
        nl = nd + 1
        a = rnd(n, nd, nd) * 0.3
        mm = (a @ a.transpose(1, 2) + torch.eye(nd, device=dev)).contiguous()  # SPD, condition number of a few
        jac_full = torch.zeros((n, nl, 6, nd), device=dev)
        jac = jac_full[:, 1:]
        jac[:, nd - 1] = torch.eye(6, nd, device=dev) + 0.15 * rnd(n, 6, nd)
        bufs = dict(actions=torch.rand((n, 6), device=dev, generator=gen) * 2 - 1, dof=rnd(n * nd, 2).contiguous(),
                    mm=mm, jac=jac, rb=rnd(n * nl, 13).contiguous(), torques=torch.zeros((n, nd), device=dev),
                    effort=torch.zeros((n, nd), device=dev), keep=jac_full)
        gains = dict(kp=[150.0] * 6, kd=[24.494898] * 6, cmd_limit=[0.1] * 3 + [0.5] * 3, kp_null=[10.0] * nd,
                     kd_null=[6.3245554] * nd, dof_default=[0.0] * nd, effort_limit=[87.0] * nd)
        p = gymtask.manip_params(nd, n, nl, nd - 1, nd, nd, 1.0, gains["kp"], gains["kd"], gains["cmd_limit"],
                                 gains["kp_null"], gains["kd_null"], gains["dof_default"], gains["effort_limit"],
                                 [-3.0] * nd, [3.0] * nd)
        cases[f"gt_osc_control_nd{nd}"] = (L.gt_osc_control, p, bufs)
        if nd == 6:
            pa = gymtask.GtArmParams()
            pa.num_envs, pa.num_links, pa.jac_row, pa.eef_link, pa.effort_stride = n, nl, nd - 1, nd, nd
            pa.action_scale = 1.0
            for name, vals in gains.items():
                getattr(pa, name)[:] = vals
            cases["gt_arm_control"] = (L.gt_arm_control, pa, bufs)

    def launch(fn, p, b):
        rc = fn(ctypes.byref(p), b["actions"].data_ptr(), b["dof"].data_ptr(), b["mm"].data_ptr(), b["jac"].data_ptr(),
                b["rb"].data_ptr(), b["torques"].data_ptr(), b["effort"].data_ptr(), stream)
        assert rc == 0, L.gt_last_error()

    out = {name: [] for name in cases}
    results = {}
    for name, case in cases.items():  # warm-up, and the nd = 6 outputs for the bit comparison
        for _ in range(10):
            launch(*case)
        torch.cuda.synchronize()
        results[name] = case[2]["torques"].clone()
    same_bits = bool(torch.equal(results["gt_arm_control"], results["gt_osc_control_nd6"]))
    for _ in range(rounds):
        for name, case in cases.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                launch(*case)
            end.record()
            end.synchronize()
            out[name].append(start.elapsed_time(end) * 1000.0 / launches)
    return out, same_bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asset-root", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--asset-file", default="franka_panda_manipulator.model.json")
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--ctl-runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    env = make(a.num_envs, a.asset_root, a.asset_file)
    pool = torch.empty((64, env.num_envs, env.num_actions), device="cuda:0").uniform_(-1, 1)
    kernels = env._kernels
    out = {"task": "Manipulator", "num_envs": a.num_envs, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "kernel_variant": int(env.sim.kernel_variant),
           "fused": [], "torch_path": []}
    for _ in range(a.runs):  # interleaved on the same env
        for mode in ("fused", "torch_path"):
            env._kernels = kernels if mode == "fused" else None
            out[mode].append(round(steps_per_s(env, pool, a.warmup, a.steps)))
    env._kernels = kernels
    times, same_bits = controller_times(a.num_envs, a.launches, a.ctl_runs)
    out["controller_us_per_launch"] = {
        name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        for name, v in times.items()}
    out["controller_launches"], out["controller_rounds"] = a.launches, a.ctl_runs
    out["nd6_bits_equal_gt_arm_control"] = same_bits
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
