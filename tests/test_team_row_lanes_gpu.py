"""Row lanes of the 4-envs-per-wave plane form of the lane-team kernels (gs_team.hip ROWL).

With row lanes on, lanes 16 .. 63 of a wave stay as three more copies of the teams in lanes 0 .. 15; copy r builds row r
(normal, tangent 1, tangent 2) of the chain candidates' records and of the self-contact pool entries and the copies
exchange the finished rows; root records are built whole by every copy.  Per-env arithmetic is the same statements in the same order as in every
other form, so every output word must equal the 16-envs-per-wave form's: a differing bit is a bug, never a tolerance
question.

Covered: gs_sim_pd_step (4 PD + 1) and plain simulate, PGS and TGS, plane, three consecutive steps, at N = 1, 5, 16,
21 and 67 envs (a lone team, a wave with one env, a full workgroup, ragged workgroups), and against
GS_TEAM_ROW_LANES=0 at N = 21.  States that reach every split loop -- crossed legs (self-contact pool full / partly
filled), ANYmal on its back (root candidates), crouched (all three candidates of a chain) -- sit first, last and alone
in a wave; which kind sits where rotates with the case, so that over the cases each kind is alone in a wave (N = 1,
the last env of N = 5 and 21).  That the states do what they are for is asserted from the REFERENCE run.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import kinematics_oracle as K
from oracle.oracle import OracleSim
from tests import helpers as H

pytestmark = pytest.mark.gpu

COUNTS = [1, 5, 16, 21, 67]
STEPS = 3
KINDS = ["full", "some", "upside", "crouch"]
THIGHS = [2, 5, 8, 11]  # bodies of ANYmal's four thighs (chain c: hip 1 + 3c, thigh 2 + 3c, shank 3 + 3c)


def _candidate_gaps(flat, root, q):
    """Each ground candidate's distance to the plane in one env (active in the kernels: below contact_offset)."""
    R, p, _, _ = K.fk(flat, root, q)
    return np.array([(p[b] + R[b] @ flat["cpoint"][c])[2] - flat["cradius"][c] for c, b in enumerate(flat["cbody"])])


@functools.lru_cache(maxsize=None)
def _special():
    """Three states of each kind, chosen on the CPU: crossed legs with the self-contact pool full (4 contacts, the
    oracle's count) and partly filled (1 .. 3); on the back, both root candidates a few mm into the plane; crouched,
    all three candidates of at least one chain in the plane (both knee ends of a thigh and its foot) and no root
    candidate active.  (In the plane, not merely within contact_offset: the rows then carry an impulse whatever
    the velocities, which is what the reference run's forces show.)"""
    art, flat = H.anymal()
    m = 600
    rng = np.random.RandomState(5)
    root, dof, tau, mu = H.anymal_states(m, seed=5)
    dof[:, :, 0] += rng.uniform(-1.8, 1.8, (m, 12))
    _, cnt = OracleSim(flat, H.ANYMAL_PARAMS).self_contacts(root, dof, mu)
    full, some = np.nonzero(cnt >= 4)[0][:3], np.nonzero((cnt >= 1) & (cnt < 4))[0][:3]
    assert len(full) == 3 and len(some) == 3
    out = {"full": [(root[i], dof[i], tau[i], mu[i]) for i in full],
           "some": [(root[i], dof[i], tau[i], mu[i]) for i in some]}
    # on the back (helpers.upside_down_anymal), slightly different heights and spins
    uroot, udof = H.upside_down_anymal(3)
    r2, d2, t2, m2 = H.anymal_states(3, seed=23)
    uroot[:, 2] = [0.096, 0.094, 0.092]
    uroot[:, 10:13] = r2[:, 10:13] * 0.3
    out["upside"] = []
    for i in range(3):
        z = _candidate_gaps(flat, uroot[i], udof[i, :, 0])
        assert z[0] < 0 and z[1] < 0
        out["upside"].append((uroot[i], udof[i], t2[i], m2[i]))
    # crouched: base height drawn low, the legs folded by random amounts
    cr, cd, ct, cm = H.anymal_states(400, seed=29, spread=0.3)
    rng = np.random.RandomState(29)
    cr[:, 2] = rng.uniform(0.12, 0.30, 400)
    cd[:, :, 0] += rng.uniform(-0.9, 0.9, (400, 12))
    out["crouch"] = []
    for i in range(400):
        z = _candidate_gaps(flat, cr[i], cd[i, :, 0])
        if z[:2].min() > H.ANYMAL_PARAMS["contact_offset"] and any(z[2 + 3 * c:5 + 3 * c].max() < 0 for c in range(4)):
            out["crouch"].append((cr[i], cd[i], ct[i], cm[i]))
        if len(out["crouch"]) == 3:
            break
    assert len(out["crouch"]) == 3
    return out


def _places(n):
    return sorted({0, n - 1} | ({3, 4, 8, 12, n - 2} if n >= 16 else set()))


def _kind_at(n, tgs):
    """place -> kind; the rotation makes each kind the lone env of a wave in some case (see the module docstring)."""
    r = COUNTS.index(n) + (2 if tgs else 0)
    return {i: KINDS[(k + r) % 4] for k, i in enumerate(_places(n))}


@functools.lru_cache(maxsize=None)
def _states(n, tgs):
    root, dof, tau, mu = H.anymal_states(n, seed=17 + n)
    sp = _special()
    used = {k: 0 for k in KINDS}
    for i, kind in _kind_at(n, tgs).items():
        xy = root[i, 0:2].copy()
        root[i], dof[i], tau[i], mu[i] = sp[kind][used[kind] % 3]
        used[kind] += 1
        root[i, 0:2] = xy
    act = np.random.RandomState(3 * n).uniform(-1, 1, (STEPS, n, 12)).astype(np.float32)
    return root, dof, tau, mu, act


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _team_form(sim):
    from isaacgymenv_amd.isaacgym import _lib
    epw, rowl = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().gs_debug_team_form(sim.handle, ctypes.byref(epw), ctypes.byref(rowl)), "gs_debug_team_form")
    return epw.value, rowl.value


def _run(monkeypatch, form, n, tgs, mode):
    """Every output of STEPS steps of `form` = (envs per wave, row lanes), as int32 bit patterns; plus the sim's
    self-contact counts at the start."""
    epw, rowl = form
    monkeypatch.setenv("GS_TEAM_ENVS_PER_WAVE", str(epw))  # both read once, at sim creation
    monkeypatch.setenv("GS_TEAM_ROW_LANES", str(rowl))
    params = dict(H.ANYMAL_PARAMS, solver_type=1 if tgs else 0)
    gym, sim = H.make_gpu_sim("anymal", n, params)
    assert sim.kernel_variant == 2
    assert _team_form(sim) == (epw, rowl), "the form under test is the one that runs"
    root, dof, tau, mu, act = _states(n, tgs)
    H.load_state_into(sim, root, dof, mu)
    _, cnt = H.sim_self_contacts(sim)
    sim.refresh("dof")  # the first PD evaluation reads the dof tensor
    out = []
    if mode == "pd":
        art, _ = H.anymal()
        default = torch.tensor([H.ANYMAL_DEFAULT[d] for d in art.dof_names()], dtype=torch.float32, device="cuda:0")
        torques = torch.zeros((n, 12), device="cuda:0")
        copy = torch.zeros((n, 12), device="cuda:0")
        for k in range(STEPS):
            a = torch.from_numpy(act[k]).to("cuda:0")
            gym.amd_pd_decimation_step(sim, a, default, 80.0, 2.0, 0.5, 80.0, 4, 1, torques, actions_copy_out=copy)
            torch.cuda.synchronize()
            out.append(dict(state=_bits(sim.state), dof=_bits(sim.dof_tensor), root=_bits(sim.root_tensor),
                            cf_soa=_bits(sim.cf_soa), cf_aos=_bits(sim.contact_tensor), torques=_bits(torques),
                            actions=_bits(copy)))
    else:
        sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
        for k in range(STEPS):
            gym.simulate(sim)
            torch.cuda.synchronize()
            out.append(dict(state=_bits(sim.state), cf_soa=_bits(sim.cf_soa)))
    assert all(np.isfinite(o["state"].view(np.float32)).all() for o in out)
    return out, cnt


def _assert_coverage(ref, cnt, n, tgs, mode):
    """The reference run's own evidence that each placed state reaches the loop it is for: self-contact counts, a
    contact force on the base body (root candidates) and on a thigh (a chain's thigh candidates).  The forces are
    those of the first substep from the placed state, which plain simulate reports (the fused step reports its
    fifth substep, by when a body pushed out of the plane may be in the air); both modes start from the same
    states and run the same substep."""
    cf = ref[0]["cf_soa"].view(np.float32).reshape(-1, 3, n)  # [body][xyz][env] after the first step
    for i, kind in _kind_at(n, tgs).items():
        if kind == "full":
            assert cnt[i] == 4, (i, cnt[i])
        elif kind == "some":
            assert 1 <= cnt[i] < 4, (i, cnt[i])
        elif mode != "simulate":
            continue
        elif kind == "upside":
            assert np.abs(cf[0, :, i]).sum() > 0, i
        else:
            assert max(np.abs(cf[b, :, i]).sum() for b in THIGHS) > 0, i


def _assert_same(ref, got, what):
    for k, (a, b) in enumerate(zip(ref, got)):
        for name in a:
            bad = np.nonzero(a[name] != b[name])
            assert a[name].shape == b[name].shape and bad[0].size == 0, (
                f"{what} step {k}: {name} differs from the reference in {bad[0].size} words, first at "
                f"{[int(x[0]) for x in bad]}")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_row_lane_form_is_bit_identical_to_the_16_form(tgs, n, monkeypatch):
    for mode in ("pd", "simulate"):
        ref, cnt = _run(monkeypatch, (16, 0), n, tgs, mode)
        _assert_coverage(ref, cnt, n, tgs, mode)
        got, _ = _run(monkeypatch, (4, 1), n, tgs, mode)
        _assert_same(ref, got, f"{mode}, row lanes")


@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_row_lane_form_is_bit_identical_to_the_4_form_without_row_lanes(tgs, monkeypatch):
    n = 21
    for mode in ("pd", "simulate"):
        ref, cnt = _run(monkeypatch, (4, 0), n, tgs, mode)
        _assert_coverage(ref, cnt, n, tgs, mode)
        got, _ = _run(monkeypatch, (4, 1), n, tgs, mode)
        _assert_same(ref, got, f"{mode}, row lanes against GS_TEAM_ROW_LANES=0")


def test_row_lanes_are_off_outside_the_4_form(monkeypatch):
    """GS_TEAM_ROW_LANES=1 leaves the 16 and 8 forms as they are (the debug entry reports what will run)."""
    monkeypatch.setenv("GS_TEAM_ROW_LANES", "1")
    for epw in (16, 8):
        monkeypatch.setenv("GS_TEAM_ENVS_PER_WAVE", str(epw))
        gym, sim = H.make_gpu_sim("anymal", 5, H.ANYMAL_PARAMS)
        assert _team_form(sim) == (epw, 0)
