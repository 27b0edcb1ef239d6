"""The DOF force tensor on every GPU kernel form, against the oracle-derived expectation of
tests/dof_force_cases.py under its tolerance rule: the one-env-per-lane kernel (ANYmal, Cartpole, and ANYmal without
gains), the runtime-sized kernel (Hound_new, which has no host solver, and ANYmal under kernel_variant 4), and the
lane team, whose launch is followed by the small clamp kernel.
"""
import numpy as np
import pytest
import torch

from tests import dof_force_cases as D
from tests import helpers as H
from tests.test_dof_force_cpu import ANYMAL_TASK_DRIVES, CARTPOLE_ONE_SUBSTEP
from tests.test_drives import CARTPOLE_DRIVES

pytestmark = pytest.mark.gpu


def test_anymal_task_gains_lane_kernel():
    case = D.Case("anymal", 256, H.ANYMAL_PARAMS, ANYMAL_TASK_DRIVES, seed=11)
    sim, fields, force = case.run(1, host=False)
    assert sim.kernel_variant == 1
    case.check(fields, force, 1, "anymal dof force gpu (one env per lane) vs oracle")


def test_cartpole_pos_and_vel_drives_lane_kernel():
    case = D.Case("cartpole", 64, CARTPOLE_ONE_SUBSTEP, CARTPOLE_DRIVES, seed=7)
    sim, fields, force = case.run(3, host=False)
    assert sim.kernel_variant == 1
    case.check(fields, force, 3, "cartpole dof force gpu (one env per lane) vs oracle")


def _clamped(case, tau):
    ef = np.asarray(case.flat["effort"], dtype=np.float64)[:case.nd]
    return np.where(ef > 0, np.clip(tau, -ef, ef), tau)


def test_no_drive_gains_lane_kernel(monkeypatch):
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "lane")
    case = D.Case("anymal", 256, H.ANYMAL_PARAMS, None, seed=5)
    case.tau[:] = D.f32(case.tau * 2.0)
    sim, fields, force = case.run(1, host=False)
    assert sim.kernel_variant == 1
    assert np.array_equal(force, _clamped(case, case.tau))


def test_hound_new_runtime_sized_kernel():
    """Hound_new with the Hound task's gains (85 / 2): no compiled topology, so the expectation is the oracle's."""
    case = D.Case("hound_new", 64, H.HOUND_PARAMS, H.HOUND_NEW_DRIVES, seed=13)
    sim, fields, force = case.run(1, host=False)
    assert sim.kernel_variant == 4
    case.check(fields, force, 1, "hound_new dof force gpu (runtime-sized) vs oracle")


def test_anymal_task_gains_runtime_sized_kernel(monkeypatch):
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    case = D.Case("anymal", 256, H.ANYMAL_PARAMS, ANYMAL_TASK_DRIVES, seed=11)
    sim, fields, force = case.run(1, host=False)
    assert sim.kernel_variant == 4
    case.check(fields, force, 1, "anymal dof force gpu (runtime-sized) vs oracle")


def _team_case():
    case = D.Case("anymal", 256, H.ANYMAL_PARAMS, None, seed=5)
    case.tau[:] = D.f32(case.tau * 2.0)  # past the 80 N m effort in about half the entries
    return case


def test_lane_team_reads_the_clamped_actuation():
    case = _team_case()
    sim, fields, force = case.run(1, host=False)
    assert sim.kernel_variant == 2
    want = _clamped(case, case.tau)
    assert (want != case.tau).mean() > 0.2 and np.array_equal(force, want)
    # one fused PD step: the clamped torques_out (torque limit 160 above the 80 N m effort)
    rng = np.random.RandomState(1)
    default = np.array([H.ANYMAL_DEFAULT[d] for d in case.art.dof_names()])
    pd = (rng.uniform(-3, 3, (case.n, 12)), default, 80.0, 2.0, 0.5, 160.0, 4)
    sim, fields, force = case.run(1, host=False, pd=pd)
    assert sim.kernel_variant == 2
    torques = case.last["torques"].cpu().numpy().astype(np.float64)
    want = _clamped(case, torques)
    assert (want != torques).mean() > 0.02 and np.array_equal(force, want)


def test_lane_team_outputs_do_not_change_with_the_tensor():
    """Root, dof and contact outputs of a lane-team sim with the tensor acquired are bit-identical to a sim without."""
    case = _team_case()
    out = []
    for acquire in (True, False):
        sim, fields, force = case.run(3, host=False, acquire=acquire)
        assert sim.kernel_variant == 2 and (force is not None) == acquire
        out.append((sim.state.clone(), case.last["contact"]))
    for what, x, y in zip(("state", "contact forces"), *out):
        assert torch.isfinite(x).all() and torch.equal(x, y), what
