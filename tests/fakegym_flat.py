"""FlatFakeGym -- TEST INFRASTRUCTURE: tests/fakegym.FakeGym with what the flat-ground tasks (tasks/anymal.py: Anymal,
Hound) ask of the simulator on top of it: the DOF force tensor, position targets, and the dof force sensor switch.

The DOF forces are a seeded pseudo-random draw, redrawn at every simulate (not from the torch RNG, so the task
layer's stream is untouched); every fourth env gets forces large enough for the torque penalty to outweigh the
tracking rewards, so the reward's clip at 0 engages there.  The same fake drives the reference's own Python
(tests/golden/make_golden_flat.py) and this repository's tasks (tests/test_flat_tasks_cpu.py).
"""
from __future__ import annotations

import numpy as np
import torch

from isaacgymenv_amd.isaacgym import gymapi as _g
from tests.fakegym import FakeGym

LARGE_FORCE_EVERY = 4
KNEE_KEEP = 0.1


class FlatFakeGym(FakeGym):
    def prepare_sim(self, sim):
        ok = super().prepare_sim(sim)
        sim.dof_frc = torch.zeros(sim.N * sim.nd, dtype=torch.float32)
        sim.ptgt = torch.zeros(sim.N * sim.nd, dtype=torch.float32)
        return ok

    def simulate(self, sim):
        super().simulate(sim)
        rng = np.random.RandomState(self.seed + 5000 + sim.t)
        f = rng.normal(0.0, 8.0, (sim.N, sim.nd))
        f[::LARGE_FORCE_EVERY] *= 12.0
        sim.dof_frc.copy_(torch.from_numpy(f.astype(np.float32).reshape(-1)))
        # the base fake touches a knee in ~19 % of the envs per step: thinned to a tenth of that, so a 32-env
        # recording also holds steps that reset nobody and steps that reset exactly one env
        drop = torch.from_numpy(rng.rand(sim.N) >= KNEE_KEEP)
        cf = sim.cf.view(sim.N, sim.nb, 3)
        for k in self.knees:
            cf[drop, k] = 0.0

    def acquire_dof_force_tensor(self, sim):
        self._sizes(sim)
        if not hasattr(sim, "dof_frc_t"):
            sim.dof_frc_t = torch.zeros(sim.N * sim.nd, dtype=torch.float32)
        return _g.GymTensor(sim.dof_frc_t, "dof_force")

    def refresh_dof_force_tensor(self, sim):
        sim.dof_frc_t.copy_(sim.dof_frc)

    def set_dof_position_target_tensor(self, sim, t):
        sim.ptgt.copy_(t.tensor.reshape(-1))
        return True

    def enable_actor_dof_force_sensors(self, env, actor):
        return True


FAKE_KW = {"anymal": dict(seed=2024, base_contact_p=0.02), "hound": dict(seed=2025, base_contact_p=0.02)}
TASKS = {"anymal": ("Anymal", "anymal_flat.npz"), "hound": ("Hound", "hound_flat.npz")}


def assert_fixture_conditions(d):
    """The cases a flat-task recording must hold (the generator asserts them, the tests re-check them)."""
    n = d["rew"].shape[1]
    base = np.linalg.norm(d["in_contact"][:, np.arange(n), int(d["base_index"])], axis=-1) > 1.0
    knee = (np.linalg.norm(d["in_contact"][:, :, d["knee_indices"]], axis=-1) > 1.0).any(-1)
    timeout = d["time_outs"] != 0
    reset = d["reset"] != 0
    k = d["reset_count_in"]  # envs reset at the start of each post_physics_step
    cases = {"base contact resets": int((reset & base).sum()), "knee contact resets": int((reset & knee & ~base).sum()),
             "time-outs": int(timeout.sum()), "steps without a reset": int((k == 0).sum()),
             "steps resetting exactly one env": int((k == 1).sum()), "clipped rewards": int((d["rew"] == 0).sum()),
             "positive rewards": int((d["rew"] > 0).sum())}
    for what, count in cases.items():
        assert count > 0, f"fixture lacks: {what}"
    return cases
