"""The link-kinematics reference and cases, pinned without a GPU (tests/kinematics_cases.py):

* the float64 oracle on every shipped asset -- Cartpole, ANYmal, Ant, Hound, Hound_new, the arm and Franka fixtures,
  the Humanoid with its nine massless hidden links -- on tumbled bases and dofs over their whole ranges: Jacobian
  against central differences of FK, 1/2 nu^T M nu against the kinetic energy of finite-difference body velocities,
  M symmetric and positive definite (the arm's smallest eigenvalue is of size 1e-4);
* the states hold their conditions (every Shepperd branch, no link rotation on a branch border, both halves of every
  dof's range, dofs on their bounds, envs at rest) and the oracle's own float32 run uses at most half of every bar, on
  every asset and kind;
* the host backend (the kernel's source on the CPU: Cartpole, ANYmal, Ant, Hound) at the C ABI against the oracle on
  those states, inside guarded buffers;
* known answers: Cartpole's pole over 33 angles in [-2 pi, 2 pi] -- quaternion, Jacobian column and mass-matrix entries
  with the analytic sine and cosine -- for the oracle and for the host backend;
* the mass-matrix bar leaves no room for a wrist entry of the arm scaled by 2 (1e4 bars; the former 1e-4 + 1e-4 rel
  let a factor of 1.8 pass).
"""
import time

import numpy as np
import pytest

from oracle import kinematics_oracle as KO
from tests import helpers as H
from tests import kinematics_cases as KC
from tests import test_kinematics_oracle as TO

ALL = tuple(KC.ASSETS)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    H.parity_report(f"[kinematics] tests/test_kinematics_cpu.py wall time {time.perf_counter() - t0:.1f} s")


def _envs_of(asset, kinds, each=2):
    kind = KC.kinds_of(asset, KC.NMAX)
    idx = np.concatenate([np.nonzero(kind == k)[0][:each] for k in kinds if k in KC.ASSETS[asset].kinds])
    root, dof = KC.states(asset, KC.NMAX)
    return root[idx], dof[idx]


@pytest.mark.parametrize("asset", ALL)
def test_oracle_jacobian_matches_fk_finite_differences(asset):
    root, dof = _envs_of(asset, ("tumbled", "limits"))
    TO.check_jacobian_against_fk(KC.ASSETS[asset].model()[1], root, dof)


@pytest.mark.parametrize("asset", ALL)
def test_oracle_mass_matrix_is_the_kinetic_energy_metric(asset):
    flat = KC.ASSETS[asset].model()[1]
    root, dof = _envs_of(asset, ("tumbled", "limits"))
    low = TO.check_mass_matrix_is_kinetic_energy_metric(flat, root, dof)
    if asset == "arm":
        assert low < 3e-4, low  # the wrist: M is positive definite with an eigenvalue of size 1e-4
    if asset == "humanoid":
        assert int((flat["mass"] == 0).sum()) == 9  # the hidden links are exactly massless, M is definite all the same


@pytest.mark.parametrize("asset", ALL)
def test_states_hold_their_conditions(asset):
    root, dof = KC.states(asset, KC.NMAX)
    figures = KC.assert_case_conditions(asset, root, dof)
    assert np.array_equal(KC.branch_counts(asset), figures["branch"])
    for n in KC.SIZES:  # the states of a smaller N are the first N
        r, d = KC.states(asset, n)
        assert np.array_equal(r, root[:n]) and np.array_equal(d, dof[:n])
    assert sorted(set(KC.kinds_of(asset, KC.NMAX))) == sorted(KC.ASSETS[asset].kinds)


@pytest.mark.parametrize("asset", ALL)
def test_float32_oracle_uses_at_most_half_of_every_bar(asset):
    ref, ref32 = KC.reference(asset), KC.reference(asset, dtype="float32")
    kind = KC.kinds_of(asset, KC.NMAX)
    every = np.arange(KC.ASSETS[asset].model()[1]["nr"])  # hidden-link rows included: the oracle computes them
    for k in KC.ASSETS[asset].kinds:
        sel = kind == k
        ratios = KC.field_ratios(asset, *(x[sel] for x in ref32), tuple(x[sel] for x in ref), links=every)
        ratios["quat_norm"] = float(np.abs(np.linalg.norm(ref32[0][sel][:, :, 3:7], axis=-1) - 1).max() / KC.BAR_NORM)
        H.parity_report(f"[kinematics f32 oracle] {asset} {k}: " + " ".join(f"{f} {v:.3f}" for f, v in ratios.items()))
        assert max(ratios.values()) <= 0.5, (asset, k, ratios)


def test_float32_oracle_runs_in_float32():
    flat = KC.ASSETS["hound"].model()[1]
    root, dof = KC.states("hound", 1)
    for out in KO.env_kinematics(flat, root[0], dof[0], np.float32):
        assert out.dtype == np.float32
    f32 = KO.cast_model(flat, np.float32)
    R, p, a, o = KO.fk(f32, root[0].astype(np.float32), dof[0, :, 0].astype(np.float32))
    assert {x.dtype for x in (R, p, a, o)} == {np.dtype(np.float32)}
    assert KO.cast_model(flat, np.float64) is flat
    # and differs from the float64 run: it is not the float64 result rounded
    r64 = KO.env_kinematics(flat, root[0], dof[0])[1]
    assert not np.array_equal(r64.astype(np.float32), KO.env_kinematics(flat, root[0], dof[0], np.float32)[1])


@pytest.mark.parametrize("asset", KC.HOST_ASSETS)
def test_host_backend_matches_oracle(asset):
    n = 5
    a = KC.ASSETS[asset]
    gym, sim = a.host_sim(n)
    ratios, ratios32 = KC.check_parity(asset, sim, n, "cpu")
    H.parity_report(f"[kinematics host] {asset}: " + " ".join(f"{f} {v:.3f}" for f, v in ratios.items()))
    # twice on the same state: identical bits; and the tensor the API hands out is the full one without the welded row
    g1, g2 = KC.run_all(asset, sim, n, "cpu"), KC.run_all(asset, sim, n, "cpu")
    for name in a.offered:
        assert np.array_equal(g1.bytes(name), g2.bytes(name))
    from isaacgymenv_amd.isaacgym import gymtorch
    jac = gymtorch.wrap_tensor(gym.acquire_jacobian_tensor(sim, asset))
    gym.refresh_jacobian_tensors(sim)
    full = g1.t["jac"]
    assert np.array_equal(jac.numpy(), (full[:, 1:] if not a.floating else full).numpy())


def test_cartpole_sweep_known_answer():
    """The pole link over 33 angles in [-2 pi, 2 pi]: oracle and host backend against the analytic row."""
    flat = KC.ASSETS["cartpole"].model()[1]
    root, dof, theta = KC.cartpole_sweep()
    n = len(theta)
    assert n == 33 and theta[0] == -theta[-1] and abs(theta[-1] - 2 * np.pi) < 1e-6
    quat, col, m11, m01, rail = KC.cartpole_known_answer(flat, dof)
    rb, jac, mm = KO.batch(flat, root, dof)
    rb = rb.reshape(n, 3, 13)
    assert np.abs(np.sum(rb[:, 2, 3:7] * quat, axis=1)).min() >= 1 - 1e-12
    np.testing.assert_allclose(jac[:, 2, :, 1], col, atol=1e-12)
    np.testing.assert_allclose(jac[:, 2, 0:3, 0], np.repeat(rail[None], n, axis=0), atol=1e-12)
    np.testing.assert_allclose(mm[:, 1, 1], m11, atol=1e-12)
    np.testing.assert_allclose(mm[:, 0, 1], m01, atol=1e-12)
    gym, sim = KC.ASSETS["cartpole"].host_sim(n)
    worst = KC.check_sweep_known_answer(sim, "cpu")
    H.parity_report(f"[kinematics host] cartpole sweep: worst error / bar {worst[0]:.3f} at |theta| = {worst[1]:.3f}")


def test_mass_matrix_bar_sees_a_wrist_entry_scaled_by_two():
    """The arm's M[5, 5] is 1.25e-4: doubled, it is 1.25 of the former 1e-4 + 1e-4 rel (scaled by 1.8 it passed) and
    1e4 of the new bar."""
    ref = KC.reference("arm")[2]
    wrong = ref.copy()
    wrong[:, 5, 5] *= 2
    assert ref[:, 5, 5].max() < 5e-4
    assert KC.ratio(wrong, ref, (1e-4, 1e-4)) < 1.3
    assert KC.ratio(ref + 0.8 * (wrong - ref), ref, (1e-4, 1e-4)) <= 1.0
    assert KC.mm_ratio("arm", wrong, ref) > 1e3
    assert KC.mm_ratio("arm", ref, ref) == 0
