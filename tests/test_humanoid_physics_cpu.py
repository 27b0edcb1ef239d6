"""The cap of tests/test_humanoid_physics_gpu.py is attainable: the physics oracle's own float32 build, run in the
kernel's place on the GPU test's states (tests/humanoid_cases.physics_states: standing with the feet in contact,
lying with the lower arms across the torso, dofs on their limits), against the fp64 oracle under helpers.STATE_TOL
and assert_close_or_explained at the project's 2 % cap -- foot sensors included.  Each case prints how many envs the
float32 build leaves beyond tolerance (the report line of assert_close_or_explained).

The sim compared is the task's: every dof in DOF_MODE_POS toward 0 with the MJCF's stiffness and damping.  Measured
when the states were chosen (64 envs, drives on, seed 12 of 3..12): 0 envs beyond tolerance in both cases; other
seeds leave one or two envs after the 20 simulates (tests/humanoid_cases.PHYSICS_SEED).  The evidence is for quiet
states only: from states that drop 2 mm onto the ground the float32 build leaves 16 of 64 envs beyond tolerance after
20 simulates, with 30 % efforts 59 of 64 (measured without drives), and the task runs at up to full efforts."""
import numpy as np
import pytest

from tests import helpers as H
from tests import humanoid_cases as HC


def test_states_hold_the_three_kinds():
    from oracle.oracle import OracleSim
    art, flat = HC.load_humanoid()
    root, dof, tau, mu = HC.physics_states()
    n = root.shape[0]
    assert n == HC.PHYSICS_N == 64
    kind = np.arange(n) % 3
    o = OracleSim(flat, HC.HUMANOID_PARAMS, self_collide=1)
    _, cnt = o.self_contacts(root, dof, mu)
    assert (cnt[kind == 1] > 0).mean() > 0.5 and (cnt[kind == 0] == 0).all()  # the arms touch the torso where lying
    # standing: one simulate leaves weight on both feet (the sensors read the ankles' reaction, ~ the body's 400 N)
    flat["self_collide"] = 1
    sb = HC.sensor_bodies(art)
    assert sb == [9, 15]
    _, _, _, sens = H.oracle_run(flat, dict(HC.HUMANOID_PARAMS, solver_type=3), root, dof, 0.0 * tau, mu, 64, 1, nsens=2,
                                 sensor_bodies=sb)
    fz = np.linalg.norm(sens[kind == 0][:, :, 0:3], axis=-1)
    assert (fz > 20.0).all(), fz.min()
    # dofs on or beyond a limit in the third kind, none elsewhere at the start
    lo, hi = flat["lower"], flat["upper"]
    out = (dof[:, :, 0] <= lo) | (dof[:, :, 0] >= hi)
    assert (out[kind == 2].sum(axis=1) == HC.LIMIT_DOFS).all() and not out[kind == 0].any()


@pytest.mark.parametrize("solver,steps,effort", HC.PHYSICS_CASES)
def test_oracle_float32_run_stays_inside_the_gpu_comparison_cap(solver, steps, effort):
    """With the task's joint drives on (DOF_MODE_POS toward 0 with the MJCF's stiffness and damping), the expected DOF
    force of the last substep included as the field "force" in units of its propagated tolerance
    (tests/dof_force_cases.py)."""
    from tests import dof_force_cases as D
    art, flat = HC.load_humanoid()
    flat["self_collide"] = 1
    root, dof, tau, mu = HC.physics_states()
    tau = (tau * effort).astype(np.float32).astype(np.float64)
    params = dict(HC.HUMANOID_PARAMS, solver_type=3 if solver == "tgs" else 0)
    f64, force64, tol = HC.oracle_reference(art, flat, params, root, dof, tau, mu, steps, 64)
    f32, force32, _ = HC.oracle_reference(art, flat, params, root, dof, tau, mu, steps, 32)
    assert np.abs(force64 - tau).max() > 0.5  # the drives act: the force is not the effort alone

    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        fl, fo, _ = HC.oracle_reference(art, flat, params, r, d, tau[idx], mu[idx], steps, bits)
        return dict(fl, force=D.in_tolerance_units(fo, tol[idx]))
    report = H.assert_close_or_explained(
        dict(f32, force=D.in_tolerance_units(force32, tol)), dict(f64, force=D.in_tolerance_units(force64, tol)), rerun,
        tol=D.FORCE_TOL, max_env_frac=0.02, what=f"oracle float32 vs float64, Humanoid with drives ({solver}, {steps} simulates)")
    print(report)
    assert np.abs(f64["q"] - dof[:, :, 0]).max() > 1e-3  # the states move: the comparison is not of a rest pose
