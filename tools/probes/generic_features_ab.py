"""Per-simulate time of the runtime-sized kernel (gs_generic.hip, kernel_variant 4) at 4096 envs by HIP events, one
robot and one libgymsim build per process (GPU box probe), for an A/B of two builds of the library:

    GS_LIBGYMSIM=<build>.so python tools/probes/generic_features_ab.py <tag> hound_new [--out DIR]
    python tools/probes/generic_features_ab.py <tag> hound [generic] [--out DIR]

hound_new (no compiled topology; point candidates, no pairs, no sensors: the kernel's plain form) also writes
DIR/<tag>_state.npy, the sim state after one simulate from the inputs of
tests/test_generic_gpu.py::test_hound_new_runs_without_a_compiled_topology, for a bitwise comparison of two builds.
hound is UsefulHound with self-collision, on the runtime-sized kernel's full form (`generic`) or on its compiled
kernel.  Each process times 20 simulates after 5, twice, and appends one JSON line to DIR/timing.jsonl."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    args = [a for a in sys.argv[1:]]
    out_dir = "."
    if "--out" in args:
        k = args.index("--out")
        out_dir = args[k + 1]
        del args[k:k + 2]
    tag, robot = args[0], args[1]
    if len(args) > 2:
        os.environ["GS_PHYSICS_KERNEL"] = args[2]
    import numpy as np
    import torch
    from tests import helpers as H
    os.makedirs(out_dir, exist_ok=True)
    out = {"tag": tag, "robot": robot, "lib": os.environ.get("GS_LIBGYMSIM", "libgymsim.so"),
           "kernel": os.environ.get("GS_PHYSICS_KERNEL", "default")}
    n = 4096
    if robot == "hound_new":
        from isaacgymenv_amd.isaacgym import gymtorch
        m = 512
        rng = np.random.RandomState(31)
        root, dof, tau, mu = H.hound_new_states(m, seed=5)
        ptgt = dof[:, :, 0] + rng.uniform(-0.2, 0.2, (m, 12))
        params = dict(H.HOUND_PARAMS, solver_type=1)
        gym, sim = H.make_gpu_sim("hound_new", m, params, drives=H.HOUND_NEW_DRIVES, self_collide=False)
        H.load_state_into(sim, root, dof, mu)
        sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)).cuda())
        gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(torch.from_numpy(ptgt.astype(np.float32)).cuda()))
        gym.simulate(sim)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"{tag}_state.npy"), sim.state.cpu().numpy())
        root, dof, tau, mu = H.hound_new_states(n, seed=2, spread=0.2)
        root[:, 2] = 0.5
        gym, sim = H.make_gpu_sim("hound_new", n, params, drives=H.HOUND_NEW_DRIVES, self_collide=False)
    else:
        root, dof, tau, mu = H.hound_states(n, seed=2, spread=0.2)
        gym, sim = H.make_gpu_sim("hound", n, H.HOUND_PARAMS)
    H.load_state_into(sim, root, dof, mu)
    for _ in range(5):
        gym.simulate(sim)
    s = torch.cuda.current_stream()
    runs = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        H.load_state_into(sim, root, dof, mu)
        e0.record(s)
        for _ in range(20):
            gym.simulate(sim)
        e1.record(s)
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / 20)
    out.update(kernel_variant=sim.kernel_variant, envs=n, ms_per_simulate=runs,
               self_collide=bool(getattr(sim, "self_collide", False)))
    print(json.dumps(out))
    with open(os.path.join(out_dir, "timing.jsonl"), "a") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
