"""Shared cases of the DOF force tensor tests (test_dof_force_cpu.py, test_dof_force_gpu.py).

The expectation is built here, in float64, from two oracle states straddling the last substep of the last simulate:

    f = clamp(tau, +-effort) + drive
    f_est = kp (q* - q - h qd) + kd (qd* - qd)                       (state before the substep)
    drive = f_est - (h kd + h^2 kp)(qd_after - qd_before)            (implicit: |f_est| <= effort, or no effort limit)
          = clamp(f_est, +-effort)                                   (saturated)

Tolerance, no free number: helpers.STATE_TOL's q and qd entries carried through that formula per dof,

    tol = |df/dq| tol_q + |df/dqd| tol_qd,  |df/dq| = kp,  |df/dqd| = |c - (kd + h kp)| + c,  c = h kd + h^2 kp

(|df/dqd| sums the two velocities the force reads: qd_before with c - (kd + h kp), qd_after with -c; tol_qd =
atol + rtol max(|qd_before|, |qd_after|)).  A saturated drive and a dof without gains have zero derivatives: there
the tensor must equal the expectation exactly (clamp(tau) and +-effort are float32 values).  The force goes
through helpers.assert_close_or_explained as the extra field "force", in units of that tolerance.
"""
import numpy as np
import torch

from tests import helpers as H

DOF_MODE_POS, DOF_MODE_VEL, DOF_MODE_EFFORT = 1, 2, 3
FORCE_TOL = dict(H.STATE_TOL, force=(1.0, 0.0))  # "force" is compared in units of its propagated tolerance
MAX_ENV_FRAC = 0.03  # test_drives.py's


def f32(a):
    """The float32 value the sim receives, as float64 (so the oracle starts from the same numbers)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def effective_gains(drives, nd):
    """(kp, kd) the solver reads: stiffness where POS, damping where POS or VEL; None = no drive."""
    if drives is None:
        return np.zeros(nd), np.zeros(nd)
    mode, kp, kd = drives
    return (np.where(mode == DOF_MODE_POS, kp, 0.0).astype(np.float64),
            np.where((mode == DOF_MODE_POS) | (mode == DOF_MODE_VEL), kd, 0.0).astype(np.float64))


def expected_force(flat, h, gains, before, after, tau, ptgt, vtgt):
    """(force [n, nd], tolerance [n, nd], saturated [n, nd] bool) in float64 from the dof states [n, nd, 2] before
    and after the last substep of length h."""
    nd = int(flat["nd"])
    kp, kd = gains
    ef = np.asarray(flat["effort"], dtype=np.float64)[:nd]
    q, qd, qd_end = before[:, :, 0], before[:, :, 1], after[:, :, 1]
    t = np.where(ef > 0, np.clip(tau, -ef, ef), tau)
    f_est = kp * (ptgt - q - h * qd) + kd * (vtgt - qd)
    impl = ~(ef > 0) | (np.abs(f_est) <= ef)
    c = h * kd + h * h * kp
    drive = np.where(impl, f_est - c * (qd_end - qd), np.clip(f_est, -ef, ef))
    (aq, rq), (av, rv) = H.STATE_TOL["q"], H.STATE_TOL["qd"]
    tol_q = aq + rq * np.abs(q)
    tol_qd = av + rv * np.maximum(np.abs(qd), np.abs(qd_end))
    tol = np.where(impl, kp * tol_q + (np.abs(c - (kd + h * kp)) + c) * tol_qd, 0.0)
    return t + drive, tol, ~impl


def in_tolerance_units(force, tol):
    """force / tol; where tol == 0 the float32 value of force (what an exact tensor entry holds) against a denominator
    that makes any difference a failure."""
    return np.where(tol > 0, force, f32(force)) / np.where(tol > 0, tol, np.finfo(np.float64).tiny ** 0.5)


class Case:
    """One robot, start states, actuation forces, drive gains and targets; inputs rounded to float32 once."""

    def __init__(self, kind, n, params, drives, seed, target_spread=None):
        self.kind, self.n, self.params, self.drives = kind, n, params, drives
        rng = np.random.RandomState(seed + 100)
        if kind == "cartpole":
            self.art, self.flat = H.cartpole()
            r = np.random.RandomState(seed)
            root = np.zeros((n, 13)); root[:, 2] = 2.0; root[:, 6] = 1.0
            dof = np.zeros((n, 2, 2))
            dof[:, :, 0] = 0.4 * (r.rand(n, 2) - 0.5)
            dof[:, :, 1] = 1.0 * (r.rand(n, 2) - 0.5)
            tau = np.zeros((n, 2)); tau[:, 0] = r.uniform(-50, 50, n)
            mu = np.ones((n, 1))
            ptgt = r.uniform(-0.5, 0.5, (n, 2))
            vtgt = r.uniform(-0.3, 0.3, (n, 2))
        else:
            self.art, self.flat = H.anymal() if kind == "anymal" else H.hound_new()
            root, dof, tau, mu = (H.anymal_states if kind == "anymal" else H.hound_new_states)(n, seed=seed)
            nd = dof.shape[1]
            if kind == "anymal":
                default = np.array([H.ANYMAL_DEFAULT[d] for d in self.art.dof_names()])
            else:
                default = np.tile([0.0, 0.6, -1.2], 4)
            ptgt = default + rng.uniform(-(target_spread or 0.5), target_spread or 0.5, (n, nd))
            vtgt = np.zeros((n, nd))
        self.nd = dof.shape[1]
        self.root, self.dof, self.tau, self.mu, self.ptgt, self.vtgt = (f32(a) for a in (root, dof, tau, mu, ptgt, vtgt))
        self.gains = effective_gains(drives, self.nd)

    # ---- the oracle
    def oracle(self, steps, root, dof, sel, bits=64, params=None):
        """`steps` simulates of envs `sel` from their states root / dof ([len(sel), ...]): (root, dof) float64."""
        if steps == 0:
            return root.copy(), dof.copy()
        r, d, _, _ = H.oracle_run(self.flat, params or self.params, root, dof, self.tau[sel], self.mu[sel], bits, steps,
                                  drives=self.gains, pos_targets=self.ptgt[sel], vel_targets=self.vtgt[sel])
        return r, d

    def reference(self, steps, root=None, dof=None, idx=None, bits=64):
        """The oracle's outputs after `steps` simulates with the expected force of the last substep: (fields,
        force, tol, saturated), for every env from the case's start or for envs idx from root / dof.  substeps == 2:
        the state before the last substep is steps - 1 whole simulates and one single-substep simulate of dt / 2
        (two_half_steps shows that this is the oracle's own first substep)."""
        sub = int(self.params["substeps"])
        h = float(self.params["dt"]) / sub
        sel = np.arange(self.n) if idx is None else np.asarray(idx)
        root = self.root[sel] if root is None else root
        dof = self.dof[sel] if dof is None else dof
        r0, d0 = self.oracle(steps - 1, root, dof, sel, bits)
        rb, db = r0, d0
        if sub != 1:
            assert sub == 2
            rb, db = self.oracle(1, r0, d0, sel, bits, params=dict(self.params, dt=h, substeps=1))
        ra, da = self.oracle(1, r0, d0, sel, bits)
        force, tol, sat = expected_force(self.flat, h, self.gains, db, da, self.tau[sel], self.ptgt[sel], self.vtgt[sel])
        return H.state_fields(ra, da), force, tol, sat

    def two_half_steps(self):
        """(whole, halves): the oracle's dof state after one two-substep simulate, and after two single-substep
        simulates of dt / 2 from the same start."""
        assert int(self.params["substeps"]) == 2
        half = dict(self.params, dt=float(self.params["dt"]) / 2, substeps=1)
        sel = np.arange(self.n)
        return self.oracle(1, self.root, self.dof, sel), self.oracle(2, self.root, self.dof, sel, params=half)

    # ---- the sim
    def run(self, steps, host, acquire=True, pd=None):
        """(sim, fields, force [n, nd] float64 or None): `steps` gym.simulate calls (pd = (actions, default, kp, kd,
        scale, limit, decimation): one fused PD step instead) and the refreshed DOF force tensor."""
        from isaacgymenv_amd.isaacgym import gymtorch
        gym, sim = H.make_gpu_sim(self.kind, self.n, self.params, host=host, drives=self.drives)
        H.load_state_into(sim, self.root, self.dof, self.mu)
        dev = sim.state.device
        frc = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim)) if acquire else None
        to = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)  # noqa: E731
        sim.dof_force.copy_(to(self.tau.reshape(-1)))
        gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(to(self.ptgt)))
        gym.set_dof_velocity_target_tensor(sim, gymtorch.unwrap_tensor(to(self.vtgt)))
        torques = None
        if pd is None:
            for _ in range(steps):
                gym.simulate(sim)
        else:
            gym.refresh_dof_state_tensor(sim)
            actions, default, kp, kd, scale, limit, decimation = pd
            torques = torch.zeros((self.n, self.nd), device=dev)
            gym.amd_pd_decimation_step(sim, to(actions), to(default), kp, kd, scale, limit, decimation, 0, torques)
        gym.refresh_dof_force_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        if not host:
            torch.cuda.synchronize()
        root, dof = H.read_state(sim, self.nd)
        force = None if frc is None else frc.cpu().numpy().astype(np.float64).reshape(self.n, self.nd)
        self.last = dict(gym=gym, torques=torques, contact=sim.contact_tensor.clone())
        return sim, H.state_fields(root, dof), force

    # ---- the comparison
    def check(self, fields, force, steps, what, ref=None):
        """State and force against the oracle-derived reference under assert_close_or_explained."""
        ref_fields, ref_force, tol, sat = ref or self.reference(steps)
        exact = tol == 0
        assert np.array_equal(force[exact], f32(ref_force[exact])), f"{what}: zero-tolerance dofs differ"

        def rerun(idx, rng, bits):
            r, d = H.perturbed(self.root, self.dof, idx, rng)
            fl, fo, _, _ = self.reference(steps, r, d, idx, bits)
            return dict(fl, force=in_tolerance_units(fo, tol[idx]))
        got = dict(fields, force=in_tolerance_units(force, tol))
        want = dict(ref_fields, force=in_tolerance_units(ref_force, tol))
        H.assert_close_or_explained(got, want, rerun, tol=FORCE_TOL, max_env_frac=MAX_ENV_FRAC, what=what)
        return ref_force, tol, sat
