"""The cap of the HoundTerrain GPU physics tests holds for the reference alone (no GPU).

tests/test_hound_terrain_gpu.py compares the runtime-sized kernel, a float solver, with the fp64 oracle on the states
of tests/hound_terrain_cases.py under helpers.assert_close_or_explained and at most 2 % of the envs beyond tolerance.
Here the oracle's own float build (liboracle32: the same restatement in float arithmetic) takes the kernel's place on
exactly those states and seeds.  It must stay within HALF of the cap, so that the cap asks the kernel for nothing a
float solver of this model cannot do, and the states must really hold what the GPU tests claim to cover: active
self-contacts, dofs at their limits, ground contacts.

Figures of this run (also in the GPU tests' docstrings):
  one simulate, 256 envs, seed 21: 1 env beyond tolerance (cap 5), 90 envs with an active self-contact;
  4 x PD + 1 sequence, 128 envs, seed 22: 0 envs beyond tolerance (cap 2), 4 envs with an active self-contact.
The states were chosen on these figures alone.  Crossed-leg states are what limits them: over the five substeps of the
PD sequence about one crossed-leg env in five ends on another branch (which leg touches first) in float than in double,
and a 1e-6 perturbation of the fp64 run does the same, so the PD case keeps four of them among 128 envs.
"""
import numpy as np

from tests import helpers as H
from tests import hound_terrain_cases as K


def _off_count(report):
    return int(report.split(";")[1].split()[0])


def test_simulate_states_cover_what_the_gpu_test_claims():
    root, dof, tau, mu = K.states(K.N_SIMULATE, K.SEED_SIMULATE)
    cnt = K.self_contact_counts(root, dof, mu)
    kind = np.arange(K.N_SIMULATE) % 4
    assert int((cnt > 0).sum()) >= K.MIN_SELF_CONTACT_ENVS_ORACLE and (cnt[kind == 1] > 0).all()
    assert (K.at_limit_counts(dof)[kind == 3] >= 1).all()
    art, flat = K.model()
    knees = dof[kind == 2][:, 2::3, 0]  # tucked: every knee within 0.15 rad of its lower limit, half of them on it
    assert (knees <= np.asarray(flat["lower"])[2::3] + 0.15).all()
    assert (K.at_limit_counts(dof)[kind == 2] >= 1).mean() > 0.8
    assert mu.min() >= 0.5 and mu.max() <= 1.25 and len(np.unique(mu[:, 0])) > 200  # per-env friction
    assert np.abs(tau).max() <= K.TORQUE_CLIP
    ref = K.oracle_simulate(root, dof, tau, mu, 64)
    assert int((np.abs(ref["cf"]).sum(axis=(1, 2)) > 0).sum()) > 64
    # the pairs are in effect: without them the oracle ends elsewhere
    x = H.oracle_run(dict(flat, self_collide=0), K.ORACLE_PARAMS, root, dof, tau, mu, 64, nc=K.NUM_LINKS)
    assert np.abs(x[1][:, :, 1] - ref["qd"]).max() > 0.1


def test_float_oracle_meets_half_the_cap_on_one_simulate():
    root, dof, tau, mu = K.states(K.N_SIMULATE, K.SEED_SIMULATE)
    ref = K.oracle_simulate(root, dof, tau, mu, 64)
    f32 = K.oracle_simulate(root, dof, tau, mu, 32)
    report = H.assert_close_or_explained(f32, ref, K.simulate_rerun(root, dof, tau, mu), max_env_frac=K.MAX_ENV_FRAC,
                                         what="hound_terrain one simulate, float oracle vs fp64 oracle (256 envs, TGS)")
    assert 2 * _off_count(report) <= K.MAX_ENV_FRAC * K.N_SIMULATE, report


def test_float_oracle_meets_half_the_cap_on_the_pd_sequence():
    root, dof, mu, act = K.pd_states(K.N_PD, K.SEED_PD)
    assert int((K.self_contact_counts(root, dof, mu) > 0).sum()) >= 4
    dof_tensor = dof.astype(np.float32).astype(np.float64)  # the dof tensor the task reads is float32
    ref = K.pd_sequence(root, dof, dof_tensor, mu, act, 64)
    assert np.abs(ref["cf"]).sum() > 0 and np.abs(ref["tau"]).max() <= K.TORQUE_CLIP
    f32 = K.pd_sequence(root, dof, dof_tensor, mu, act, 32)
    report = H.assert_close_or_explained(f32, ref, K.pd_rerun(root, dof, dof_tensor, mu, act), tol=K.SEQ_TOL,
                                         max_env_frac=K.MAX_ENV_FRAC,
                                         what="hound_terrain 4 x PD + 1, float oracle vs fp64 oracle (128 envs, TGS)")
    assert 2 * _off_count(report) <= K.MAX_ENV_FRAC * K.N_PD, report
