"""Physics cases of the HoundTerrain tests (TEST INFRASTRUCTURE): the Hound_new model with HoundTerrain's asset
options and collision filter 0 on the runtime-sized kernel, the states of its one-simulate and fused-PD-step tests, and
the oracle's side of both.  tests/test_hound_terrain_physics_cpu.py runs the float oracle against the fp64 oracle on
exactly these states (the cap must be attainable by a float solver at all); tests/test_hound_terrain_gpu.py runs the
kernel on them.
"""
import numpy as np

from oracle.oracle import OracleSim
from tests import helpers as H

# HoundTerrain.yaml's sim block is AnymalTerrain's (dt 0.005, 1 substep, 4 / 1 iterations, contacts of the last
# substep); TGS as the task runs it (config.yaml solver_type 1; the oracle's TGS is solver_type 3)
PARAMS = dict(H.HOUND_PARAMS, solver_type=1)
ORACLE_PARAMS = dict(H.HOUND_PARAMS, solver_type=3)
DEFAULT_POS = np.array([0.0, 0.7854, -1.5708] * 4)  # HoundTerrain.yaml defaultJointAngles in dof order
KP, KD, ACTION_SCALE, TORQUE_CLIP, DECIMATION, EXTRA = 80.0, 2.0, 0.5, 80.0, 4, 1
MAX_ENV_FRAC = 0.02  # the project's cap for this robot (tests/test_generic_gpu.py)
N_SIMULATE, SEED_SIMULATE = 256, 21
N_PD, SEED_PD = 128, 22
# tolerances of the 4 x PD + 1 sequence (5 substeps; tests/test_hound_gpu.py SEQ_TOL, test_headline_oracle_gpu.py)
SEQ_TOL = {"q": (1e-4, 0.0), "qd": (2.5e-2, 2.5e-2), "pose": (1e-4, 0.0), "vel": (2.5e-2, 2.5e-2), "tau": (0.5, 1e-2),
           "cf": (2.0, 5e-2)}
NUM_LINKS = 17
# envs of the one-simulate states with an active self-contact: the fp64 oracle's pools hold one in 90 of the 256
# (tests/test_hound_terrain_physics_cpu.py asserts that); the kernel's pools (gs_debug_self_contacts) must show at
# least 80 -- ten fewer, for float contacts that sit within rounding of the contact offset
MIN_SELF_CONTACT_ENVS_ORACLE = 90
MIN_SELF_CONTACT_ENVS = 80


def model():
    """(articulation, flat model) of urdf/Hound_new/Hound.urdf under HoundTerrain's options: fixed joints kept,
    cylinders kept, collision filter 0."""
    art, flat = H.hound_new()  # HOUND_NEW_OPTS are Hound_terrain.py:218-229's values
    flat["self_collide"] = 1
    assert (flat["nb"], flat["nd"], flat["nr"], flat["ns"], flat["nc"]) == (13, 12, NUM_LINKS, 17, 84)
    assert flat["npair"] == 120 and flat["npool"] == 8 and all(flat["has_limits"])
    return art, flat


def _crossed(m, seed, spread, max_depth):
    """m crossed-leg states with at least one self-contact and none deeper than max_depth, the first such of a
    seeded pool (the oracle's self-contact pools decide, as tests/test_self_collision.py::crossed_leg_states)."""
    art, flat = model()
    lo, hi = np.asarray(flat["lower"]), np.asarray(flat["upper"])
    rng = np.random.RandomState(3000 + seed)
    pool = 60 * m
    root, dof, _, mu = H.hound_new_states(pool, seed=seed + 500, spread=spread)
    inward = np.array([-1.0, 1.0, -1.0, 1.0])  # FL, FR, RL, RR roll joints: towards the body's mid-plane
    dof[:, :, 0] += rng.uniform(-1.2, 1.2, (pool, 12))
    dof[:, 0::3, 0] += inward * rng.uniform(0.0, 0.9, (pool, 4))
    dof[:, :, 0] = np.clip(dof[:, :, 0], lo, hi)
    root[:, 2] += 0.1
    c, cnt = OracleSim(flat, ORACLE_PARAMS).self_contacts(root, dof, mu)
    depth = np.where(np.arange(c.shape[1])[None, :] < cnt[:, None], -c[:, :, 6], 0.0).max(axis=1)
    idx = np.nonzero((cnt >= 1) & (depth <= max_depth))[0][:m]
    assert len(idx) == m, (len(idx), m)
    return root[idx], dof[idx], mu[idx]


def states(n, seed, spread=1.0, max_depth=0.02, crossed_every=4, limit_frac=1.0):
    """n states in four kinds by env index % 4, per-env friction in [0.5, 1.25] and torques within the task's clip:
    0 standing near the task's pose (H.hound_new_states: on, above or into the ground, tilted, moving);
    1 crossed legs: every joint moved by up to +-1.2 rad and the roll joints turned inwards, clipped to the limits,
      chosen so that a self-contact is active and none is deeper than max_depth;
    2 tucked legs: knees at or next to their lower limit (-2.79 rad), hips swung by up to +-1.5 rad;
    3 dofs at their limits: each roll and knee dof, with probability limit_frac, at its lower or upper limit (hips,
      +-2 pi, stay free; at least one dof per env), moving into the limit on half of them.
    spread scales the base tilt, the velocities and the hip swing; max_depth bounds how far crossed legs overlap;
    crossed_every (a multiple of 4) thins kind 1 to the envs with index % crossed_every == 1, the rest of them
    standing."""
    art, flat = model()
    lo, hi = np.asarray(flat["lower"]), np.asarray(flat["upper"])
    rng = np.random.RandomState(1000 + seed)
    root, dof, tau, mu = H.hound_new_states(n, seed=seed, spread=spread)
    kind = np.arange(n) % 4
    hip, knee = np.array([1, 4, 7, 10]), np.array([2, 5, 8, 11])
    assert crossed_every % 4 == 0
    kind[(kind == 1) & (np.arange(n) % crossed_every != 1)] = 0
    k1 = kind == 1
    root[k1], dof[k1], mu[k1] = _crossed(int(k1.sum()), seed, spread, max_depth)
    q, qd = dof[:, :, 0], dof[:, :, 1]
    k2 = kind == 2
    q[np.ix_(k2, knee)] = lo[knee] + rng.uniform(0.0, 0.15, (int(k2.sum()), 4)) * (rng.rand(int(k2.sum()), 4) < 0.5)
    q[np.ix_(k2, hip)] += rng.uniform(-1.5, 1.5, (int(k2.sum()), 4)) * spread
    k3 = kind == 3
    m3 = int(k3.sum())
    side = rng.rand(m3, 12) < 0.5
    at = np.where(side, lo, hi)
    free = np.zeros(12, dtype=bool)
    free[hip] = True
    chosen = ~free & (rng.rand(m3, 12) < limit_frac)
    chosen[np.arange(m3), 3 * rng.randint(0, 4, m3) + 2 * rng.randint(0, 2, m3)] = True  # a roll or a knee dof
    q[k3] = np.where(chosen, at, q[k3])
    push = np.where(side, -1.0, 1.0) * np.abs(qd[k3])
    qd[k3] = np.where(chosen & (rng.rand(m3, 12) < 0.5), push, qd[k3])
    dof[:, :, 0] = np.clip(q, lo, hi)
    root[k3 | k2, 2] += 0.15  # folded / splayed legs: keep the trunk off the plane
    tau = rng.uniform(-TORQUE_CLIP, TORQUE_CLIP, (n, 12))
    return root, dof, tau, mu


def pd_states(n, seed, spread=0.5, max_depth=0.005, crossed_every=32):
    """States and actions of the fused PD step: the task's own regime -- joints within +-0.4 spread rad of the default
    angles, the base tilted and moving by hound_new_states' spread, actions in +-spread -- so that the PD torques
    mostly stay inside the +-80 clip instead of whirling the light legs to their velocity limits, where one simulate
    sequence is decided by which leg hits which first; every crossed_every-th env has crossed legs with an active
    self-contact at most max_depth deep.  Returns (root, dof, mu, actions)."""
    rng = np.random.RandomState(4000 + seed)
    root, dof, _, mu = H.hound_new_states(n, seed=seed, spread=spread)
    dof[:, :, 0] = DEFAULT_POS + rng.uniform(-0.4, 0.4, (n, 12)) * spread
    k1 = np.arange(n) % crossed_every == 1
    root[k1], dof[k1], mu[k1] = _crossed(int(k1.sum()), seed, spread, max_depth)
    act = rng.uniform(-1.0, 1.0, (n, 12)) * spread
    return root, dof, mu, act


def self_contact_counts(root, dof, mu):
    art, flat = model()
    return OracleSim(flat, ORACLE_PARAMS).self_contacts(root, dof, mu)[1]


def at_limit_counts(dof):
    art, flat = model()
    lo, hi = np.asarray(flat["lower"]), np.asarray(flat["upper"])
    q = dof[:, :, 0]
    return ((q <= lo + 1e-9) | (q >= hi - 1e-9)).sum(axis=1)


def oracle_simulate(root, dof, tau, mu, bits=64):
    """One simulate on the oracle: STATE_TOL fields incl. the per-link contact forces."""
    art, flat = model()
    r, d, c, _ = H.oracle_run(flat, ORACLE_PARAMS, root, dof, tau, mu, bits, nc=NUM_LINKS)
    return H.state_fields(r, d, c)


def simulate_rerun(root, dof, tau, mu):
    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        return oracle_simulate(r, d, tau[idx], mu[idx], bits)
    return rerun


def pd_sequence(root, dof, dof_tensor, mu, act, bits=64):
    """Hound_terrain.py:458-468's decimation loop and VecTask's extra simulate on the oracle (the sequence
    gs_sim_pd_step fuses; tests/test_hound_gpu.py::_pd_sequence's pattern): the first PD torque from the dof tensor
    as the task last saw it, the next from the oracle's own state."""
    art, flat = model()
    dt = np.float64 if bits == 64 else np.float32
    c = lambda a: np.array(a, dtype=dt, order="C")  # noqa: E731  (a copy: the oracle steps it in place)
    sim = OracleSim(flat, ORACLE_PARAMS, real_bits=bits)
    r, d, m = c(root), c(dof), c(mu)
    cf = np.zeros((root.shape[0], NUM_LINKS, 3), dt)
    q, qd = dof_tensor[:, :, 0], dof_tensor[:, :, 1]
    tau = None
    for i in range(DECIMATION + EXTRA):
        if i < DECIMATION:
            tau = np.clip(KP * (ACTION_SCALE * act + DEFAULT_POS - q) - KD * qd, -TORQUE_CLIP, TORQUE_CLIP)
        sim.simulate(r, d, c(tau), m, cf)
        q, qd = d[:, :, 0].copy(), d[:, :, 1].copy()
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    return dict(q=f(d[:, :, 0]), qd=f(d[:, :, 1]), pose=f(r[:, :7]), vel=f(r[:, 7:]), tau=f(tau), cf=f(cf))


def pd_rerun(root, dof, dof_tensor, mu, act):
    def rerun(idx, rng, bits):
        r, d = H.perturbed(root, dof, idx, rng)
        return pd_sequence(r, d, dof_tensor[idx], mu[idx], act[idx], bits)
    return rerun
