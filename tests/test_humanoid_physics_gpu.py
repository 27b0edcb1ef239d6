"""Humanoid physics on the GPU (the runtime-sized kernel, kernel_variant 4: 22 moving bodies of which 9 are massless
hidden links, 21 dofs, 147 self-collision pairs, sensors on both feet) vs the fp64 oracle on the states of
tests/test_humanoid_physics_cpu.py: one simulate under TGS with 2 % efforts and 20 simulates under PGS, through the
explained-env rule at the project's 2 % cap with helpers.STATE_TOL, the foot sensors and the DOF force tensor
included.  The sim is the task's: every dof in DOF_MODE_POS toward 0 with the MJCF's stiffness and damping, so the DOF
force tensor holds effort plus spring-damper force; its expectation and tolerance are built as in
tests/dof_force_cases.py from the oracle's states around the last substep."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import humanoid_cases as HC

pytestmark = pytest.mark.gpu


def _gpu(params, root, dof, tau, mu, steps):
    n = root.shape[0]
    gym, sim = HC.make_sim(n, params)
    assert sim.kernel_variant == 4 and sim.num_sensors == 2 and sim.self_collide
    H.load_state_into(sim, root, dof, mu)
    sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)).to(sim.state.device))
    for _ in range(steps):
        gym.simulate(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, HC.ND)
    gym.refresh_force_sensor_tensor(sim)
    gym.refresh_dof_force_tensor(sim)
    torch.cuda.synchronize()
    sens = sim.sensor_tensor.cpu().numpy().astype(np.float64).reshape(n, 2, 6)
    force = sim.dof_force_tensor.cpu().numpy().reshape(n, HC.ND)
    return g_root, g_dof, sens, force


@pytest.mark.parametrize("solver,steps,effort", HC.PHYSICS_CASES)
def test_humanoid_matches_the_oracle(solver, steps, effort):
    from tests import dof_force_cases as D
    art, flat = HC.load_humanoid()
    flat["self_collide"] = 1
    root, dof, tau, mu = HC.physics_states()
    tau = (tau * effort).astype(np.float32).astype(np.float64)
    params = dict(HC.HUMANOID_PARAMS, solver_type=1 if solver == "tgs" else 0)
    oparams = dict(HC.HUMANOID_PARAMS, solver_type=3 if solver == "tgs" else 0)
    g_root, g_dof, g_sens, g_force = _gpu(params, root, dof, tau, mu, steps)
    ref, force, tol = HC.oracle_reference(art, flat, oparams, root, dof, tau, mu, steps, 64)
    assert np.abs(force - tau).max() > 0.5 and (tol > 0).all()  # the drives act on every dof

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        fl, fo, _ = HC.oracle_reference(art, flat, oparams, r, d, tau[idx], mu[idx], steps, bits)
        return dict(fl, force=D.in_tolerance_units(fo, tol[idx]))
    got = dict(H.state_fields(g_root, g_dof, sens=g_sens), force=D.in_tolerance_units(g_force.astype(np.float64), tol))
    H.assert_close_or_explained(got, dict(ref, force=D.in_tolerance_units(force, tol)), rerun, tol=D.FORCE_TOL,
                                max_env_frac=0.02, what=f"Humanoid with drives vs the oracle ({solver}, {steps} simulates)")
