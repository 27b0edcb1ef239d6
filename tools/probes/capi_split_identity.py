"""Bit identity of libgymsim across a change that must not touch a result: sha256 of the state, the contact forces and
the force sensors after 20 steps of five scenes built through gymapi.

    python tools/probes/capi_split_identity.py [--device cpu|gpu] [--kernel auto|lane|team|generic] [--n 67]
                                               [--scenes anymal_plane,anymal_trimesh,hound,ant,cartpole_drives]

Run it on two builds (GS_LIBGYMSIM names another library file in isaacgymenv_amd/_lib) and compare the lines: same
kernels, same inputs, so every hash must be equal.  ANYmal and UsefulHound run the fused PD step
(amd_pd_decimation_step, 4 x PD + 1) with a fixed action pattern, Ant and Cartpole `simulate` with fixed dof forces
(Cartpole: a position and a velocity drive with fixed targets), all from the assets' default state.  A scene the
requested kernel form refuses prints the refusal instead, which must be equal too.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS = 20


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def run(scene, n, host):
    import torch
    from isaacgymenv_amd.isaacgym import gymtorch
    from tests import helpers as H
    drives = None
    if scene == "anymal_plane":
        kind, params, ter = "anymal", H.ANYMAL_PARAMS, None
    elif scene == "anymal_trimesh":
        kind, params, ter = "anymal", dict(H.ANYMAL_PARAMS, has_ground=0), H.rough_terrain(seed=5)
    elif scene == "hound":
        kind, params, ter = "hound", H.HOUND_PARAMS, None
    elif scene == "ant":
        kind, params, ter = "ant", H.ANT_PARAMS, None
    else:
        kind, params, ter = "cartpole", H.CARTPOLE_PARAMS, None
        drives = (np.array([1, 2], dtype=np.int32), np.array([400.0, 0.0]), np.array([30.0, 2.0]))
    gym, sim = H.make_gpu_sim(kind, n, params, terrain=ter, host=host, drives=drives,
                              self_collide=True if kind == "hound" else None)
    dev, nd = sim.state.device, sim.num_dofs
    i = torch.arange(n * nd, dtype=torch.float32, device=dev).reshape(n, nd)
    if kind in ("anymal", "hound"):
        gym.refresh_dof_state_tensor(sim)
        default = torch.zeros(nd, device=dev)
        torques = torch.zeros((n, nd), device=dev)
        for k in range(STEPS):
            act = torch.sin(0.37 * i + 0.9 * k)
            gym.amd_pd_decimation_step(sim, act, default, 80.0, 2.0, 0.5, 80.0, 4, 1, torques)
    else:
        if drives is not None:
            gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(0.3 * torch.sin(0.5 * i)))
            gym.set_dof_velocity_target_tensor(sim, gymtorch.unwrap_tensor(0.2 * torch.cos(0.5 * i)))
        for k in range(STEPS):
            sim.dof_force.copy_((10.0 * torch.sin(0.37 * i + 0.9 * k)).reshape(-1))
            gym.simulate(sim)
    if not host:
        torch.cuda.synchronize()
    assert torch.isfinite(sim.state).all()
    return f"variant {sim.kernel_variant} state {sha(sim.state)} contacts {sha(sim.cf_soa)} sensors {sha(sim.sens_soa)}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="gpu", choices=["cpu", "gpu"])
    ap.add_argument("--kernel", default="auto", choices=["auto", "lane", "team", "generic"])
    ap.add_argument("--n", type=int, default=67)
    ap.add_argument("--scenes", default="anymal_plane,anymal_trimesh,hound,ant,cartpole_drives")
    a = ap.parse_args()
    os.environ["GS_PHYSICS_KERNEL"] = a.kernel
    for scene in a.scenes.split(","):
        try:
            line = run(scene, a.n, a.device == "cpu")
        except RuntimeError as e:
            line = f"refused: {e}"
        print(f"{a.device} kernel={a.kernel} n={a.n} {scene}: {line}", flush=True)
