"""Resident sweeps of the row-lane form of the lane-team kernels (gs_team.hip RES), and the fused PD
step's contact forces formed once per launch.

With resident sweeps on, copy c = lane >> 4 of a team keeps chain c's contact records, velocity and impulses in its
registers over the Gauss-Seidel sweeps of a substep; chain block c of a sweep runs in copy c alone and the copies then
take the base velocity from it (the hand-off).  Each contact's arithmetic is the same statements on the same values in
the same order as in the replicated form, so every output word must be equal: a differing bit is a bug, never a
tolerance question.  tests/test_team_row_lanes_gpu.py and test_team_envs_per_wave_gpu.py pin the default (resident)
launch to the 16 form; this file pins what they cannot single out.

Everything is compared as int32 words (state, dof, root, cf_soa, cf_aos, torques, the actions copy), over three
consecutive steps, fused PD step (4 PD + 1) and plain simulate, PGS and TGS.

* resident on against off (GS_TEAM_RESIDENT_SWEEPS=1 / 0, both with row lanes) at N = 1, 5, 21, the row-lane test's
  states; the form that ran is read back with gs_debug_team_sweeps;
* the hand-off chain: states with ground contacts in chain 3 only, in chains 0 and 2 only (a hand-off passes an idle
  copy), crouched (all three candidates of a chain), on the back (root candidates before chain 0), crossed legs with
  the pool full, and with the pool partly filled -- one state with an entry between two chains, one with an entry
  between a chain and the base.  Each kind sits first and last in a wave of four envs and, in the case named after it,
  alone in the launch's last wave.  That the states do what they are for is asserted from the REFERENCE run (resident
  off): pool counts and bodies from the sim's self-contact pools, contact forces after the first simulate.
  (An entry whose two bodies share a chain is stored with chain B = -1, the value a base body gets; ANYmal's pair
  table has no pair within one leg, so that case is reached here through the base entry only.)
* iteration-count edges at N = 5: 1 position / 0 velocity iterations and 4 / 1 (the position snapshot after sweep
  pos_iters - 1 and TGS's mean-velocity path);
* forces once per launch: with 1 and 2 substeps the fused step (4 PD + 1) leaves the cf_soa and cf_aos of the same
  sim stepped by separate launches, which each collect: launches of the fused kernel, and four of them with a final
  plain simulate (to the bit; TGS with 2 substeps against the plain simulate to 1e-3 N: the test's docstring);
* GS_TEAM_RESIDENT_SWEEPS=1 is ignored outside the row-lane form.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle.oracle import OracleSim
from tests import helpers as H
from tests import test_team_row_lanes_gpu as RL

pytestmark = pytest.mark.gpu

STEPS = 3
HAND_OFF_KINDS = ["chain3", "chains02", "crouch", "upside", "full", "some_cross", "some_base"]
CHAIN_BODIES = [[1 + 3 * c, 2 + 3 * c, 3 + 3 * c] for c in range(4)]


def _chain_of(body):
    return -1 if body < 1 else (int(body) - 1) // 3


def _resident(sim):
    from isaacgymenv_amd.isaacgym import _lib
    res = ctypes.c_int(-1)
    _lib.check(_lib.lib().gs_debug_team_sweeps(sim.handle, ctypes.byref(res)), "gs_debug_team_sweeps")
    return res.value


def _make(monkeypatch, form, resident, n, params):
    """A sim of `form` = (envs per wave, row lanes) with the resident-sweeps selector set (all read at creation)."""
    epw, rowl = form
    monkeypatch.setenv("GS_TEAM_ENVS_PER_WAVE", str(epw))
    monkeypatch.setenv("GS_TEAM_ROW_LANES", str(rowl))
    monkeypatch.setenv("GS_TEAM_RESIDENT_SWEEPS", str(resident))
    gym, sim = H.make_gpu_sim("anymal", n, params)
    assert sim.kernel_variant == 2
    assert RL._team_form(sim) == (epw, rowl)
    return gym, sim


def _default_pos():
    art, _ = H.anymal()
    return torch.tensor([H.ANYMAL_DEFAULT[d] for d in art.dof_names()], dtype=torch.float32, device="cuda:0")


def _pd(gym, sim, a, default, decimation, extra, torques, copy=None):
    gym.amd_pd_decimation_step(sim, a, default, 80.0, 2.0, 0.5, 80.0, decimation, extra, torques,
                               actions_copy_out=copy)


def _run(monkeypatch, resident, states, params, mode):
    """Every output of STEPS steps of the row-lane form with resident sweeps on / off, as int32 words; plus the sim's
    self-contact pools at the start."""
    root, dof, tau, mu, act = states
    n = root.shape[0]
    gym, sim = _make(monkeypatch, (4, 1), resident, n, params)
    assert _resident(sim) == resident, "the form under test is the one that runs"
    H.load_state_into(sim, root, dof, mu)
    pools = H.sim_self_contacts(sim)
    sim.refresh("dof")  # the first PD evaluation reads the dof tensor
    out = []
    if mode == "pd":
        default = _default_pos()
        torques = torch.zeros((n, 12), device="cuda:0")
        copy = torch.zeros((n, 12), device="cuda:0")
        for k in range(STEPS):
            _pd(gym, sim, torch.from_numpy(act[k]).to("cuda:0"), default, 4, 1, torques, copy)
            torch.cuda.synchronize()
            out.append(dict(state=RL._bits(sim.state), dof=RL._bits(sim.dof_tensor), root=RL._bits(sim.root_tensor),
                            cf_soa=RL._bits(sim.cf_soa), cf_aos=RL._bits(sim.contact_tensor),
                            torques=RL._bits(torques), actions=RL._bits(copy)))
    else:
        sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
        for k in range(STEPS):
            gym.simulate(sim)
            torch.cuda.synchronize()
            out.append(dict(state=RL._bits(sim.state), cf_soa=RL._bits(sim.cf_soa)))
    assert all(np.isfinite(o["state"].view(np.float32)).all() for o in out)
    return out, pools


def _params(tgs, **over):
    return dict(H.ANYMAL_PARAMS, solver_type=1 if tgs else 0, **over)


def _row_lane_states(n, tgs):
    return RL._states(n, tgs)


# ------------------------------------------------------------------ resident on against off
@pytest.mark.parametrize("n", [1, 5, 21])
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_resident_sweeps_are_bit_identical_to_the_replicated_sweeps(tgs, n, monkeypatch):
    for mode in ("pd", "simulate"):
        ref, (_, cnt) = _run(monkeypatch, 0, _row_lane_states(n, tgs), _params(tgs), mode)
        RL._assert_coverage(ref, cnt, n, tgs, mode)
        got, _ = _run(monkeypatch, 1, _row_lane_states(n, tgs), _params(tgs), mode)
        RL._assert_same(ref, got, f"{mode}, resident sweeps against GS_TEAM_RESIDENT_SWEEPS=0")


# ------------------------------------------------------------------ the hand-off chain
def _lifted(flat, dof_names, keep):
    """Upright ANYmal at rest whose legs outside `keep` are folded up (thigh and shank angles tripled), the feet of
    the chains in `keep` 4 mm into the plane: ground contacts in those chains only."""
    root = np.zeros(13)
    root[6] = 1.0
    root[2] = 1.0
    q = np.array([H.ANYMAL_DEFAULT[d] for d in dof_names])
    for c in range(4):
        if c not in keep:
            q[3 * c + 1] *= 3.0
            q[3 * c + 2] *= 3.0
    z = RL._candidate_gaps(flat, root, q)
    root[2] -= min(z[2 + 3 * c:5 + 3 * c].min() for c in keep) + 0.004
    z = RL._candidate_gaps(flat, root, q)
    off = H.ANYMAL_PARAMS["contact_offset"]
    assert z[:2].min() > off
    for c in range(4):
        zc = z[2 + 3 * c:5 + 3 * c]
        assert (zc.min() < 0) if c in keep else (zc.min() > off), (c, zc)
    dof = np.zeros((12, 2))
    dof[:, 0] = q
    return root, dof


@functools.lru_cache(maxsize=None)
def _hand_off_special():
    """One state of each kind (root, dof, tau, mu), chosen on the CPU."""
    art, flat = H.anymal()
    sp = RL._special()
    _, _, tau, mu = H.anymal_states(2, seed=41)
    out = {k: sp[k][0] for k in ("crouch", "upside", "full")}
    for i, (kind, keep) in enumerate((("chain3", (3,)), ("chains02", (0, 2)))):
        root, dof = _lifted(flat, art.dof_names(), keep)
        out[kind] = (root, dof, 0.0 * tau[i], mu[i])  # (no joint torque: nothing lifts the feet off the plane)
    # partly filled pools: the row-lane test's draw, split by what the entries join
    m = 600
    rng = np.random.RandomState(5)
    root, dof, tau, mu = H.anymal_states(m, seed=5)
    dof[:, :, 0] += rng.uniform(-1.8, 1.8, (m, 12))
    con, cnt = OracleSim(flat, H.ANYMAL_PARAMS).self_contacts(root, dof, mu)
    for i in np.nonzero((cnt >= 1) & (cnt < 4))[0]:
        chains = [(_chain_of(con[i, p, 8]), _chain_of(con[i, p, 9])) for p in range(cnt[i])]
        if "some_cross" not in out and any(a >= 0 and b >= 0 and a != b for a, b in chains):
            out["some_cross"] = (root[i], dof[i], tau[i], mu[i])
        elif "some_base" not in out and any(a < 0 or b < 0 for a, b in chains):
            out["some_base"] = (root[i], dof[i], tau[i], mu[i])
    assert set(out) == set(HAND_OFF_KINDS)
    return out


def _hand_off_places(alone):
    """env -> kind: kind k first in wave 2k and last in wave 2k + 1 (waves of four envs), `alone` the only env of the
    launch's last wave."""
    places = {}
    for k, kind in enumerate(HAND_OFF_KINDS):
        places[8 * k] = kind
        places[8 * k + 7] = kind
    places[8 * len(HAND_OFF_KINDS)] = alone
    return places


@functools.lru_cache(maxsize=None)
def _hand_off_states(alone):
    places = _hand_off_places(alone)
    n = max(places) + 1
    assert n % 4 == 1
    root, dof, tau, mu = H.anymal_states(n, seed=57)
    sp = _hand_off_special()
    for i, kind in places.items():
        xy = root[i, 0:2].copy()
        root[i], dof[i], tau[i], mu[i] = sp[kind]
        root[i, 0:2] = xy
    act = np.random.RandomState(57).uniform(-1, 1, (STEPS, n, 12)).astype(np.float32)
    return root, dof, tau, mu, act


def _assert_hand_off_coverage(ref, pools, alone, mode):
    """The reference run's own evidence that each placed state reaches the path it is for."""
    con, cnt = pools
    n = cnt.shape[0]
    cf = ref[0]["cf_soa"].view(np.float32).reshape(-1, 3, n)  # [body][xyz][env] after the first step
    force = lambda bodies, i: sum(np.abs(cf[b, :, i]).sum() for b in bodies)
    for i, kind in _hand_off_places(alone).items():
        chains = [(_chain_of(con[i, p, 8]), _chain_of(con[i, p, 9])) for p in range(cnt[i])]
        if kind == "full":
            assert cnt[i] == 4, (i, cnt[i])
        elif kind == "some_cross":
            assert 1 <= cnt[i] < 4 and any(a >= 0 and b >= 0 and a != b for a, b in chains), (i, chains)
        elif kind == "some_base":
            assert 1 <= cnt[i] < 4 and any(a < 0 or b < 0 for a, b in chains), (i, chains)
        elif mode != "simulate":
            continue  # (the fused step reports its fifth substep, by when a body pushed out may be in the air)
        elif kind == "upside":
            assert force([0], i) > 0, i
        elif kind == "crouch":
            assert max(force([b], i) for b in RL.THIGHS) > 0, i
        else:
            keep = (3,) if kind == "chain3" else (0, 2)
            assert cnt[i] == 0 and force([0], i) == 0, (i, kind)
            for c in range(4):
                assert (force(CHAIN_BODIES[c], i) > 0) == (c in keep), (i, kind, c)


@pytest.mark.parametrize("alone", HAND_OFF_KINDS)
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_hand_off_chain(tgs, alone, monkeypatch):
    for mode in ("pd", "simulate"):
        ref, pools = _run(monkeypatch, 0, _hand_off_states(alone), _params(tgs), mode)
        _assert_hand_off_coverage(ref, pools, alone, mode)
        got, _ = _run(monkeypatch, 1, _hand_off_states(alone), _params(tgs), mode)
        RL._assert_same(ref, got, f"{mode}, hand-off chain with {alone} alone in the last wave")


# ------------------------------------------------------------------ iteration-count edges
@pytest.mark.parametrize("iters", [(1, 0), (4, 1)], ids=["1+0", "4+1"])
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_iteration_count_edges(tgs, iters, monkeypatch):
    n = 5
    params = _params(tgs, pos_iters=iters[0], vel_iters=iters[1])
    for mode in ("pd", "simulate"):
        ref, _ = _run(monkeypatch, 0, _row_lane_states(n, tgs), params, mode)
        got, _ = _run(monkeypatch, 1, _row_lane_states(n, tgs), params, mode)
        RL._assert_same(ref, got, f"{mode}, {iters[0]} position + {iters[1]} velocity iterations")


# ------------------------------------------------------------------ forces once per launch
@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
def test_fused_step_forces_equal_those_of_separate_launches(tgs, substeps, monkeypatch):
    """The fused step (4 PD evaluations, 5 simulates, one launch) collects contact forces in its last substep only.
    The same sim stepped by separate launches, every one of which collects, must end with the same forces:

    * by launches of the fused kernel itself -- three of one PD evaluation + one simulate, then one of one evaluation
      + two simulates: every word (state, cf_soa, cf_aos, torques) equal;
    * by four launches of one evaluation + one simulate and a fifth PLAIN simulate on the last torques
      (gs_sim_simulate, the refreshed contact tensor): the reference that does not share the fused kernel's choice of
      the collecting substep.  cf_soa and cf_aos must be equal word for word with PGS (1 and 2 substeps) and with TGS
      and 1 substep.  With TGS and 2 substeps they cannot be: the plain simulate is another kernel than the fused
      step and rounds a few last bits of the state differently -- for the parent commit exactly as for this one, at
      these very states: 20 state words off by at most 9.6e-7 and 3 force words off by 4.6e-5 N (in the other three
      cases 3 .. 7 state words and no force word).  That case is held to atol 1e-3 N, rtol 1e-5: twenty times the
      reference kernels' own disagreement and ~80 ulp.  Forces collected in another substep would miss it: the
      reference's own forces move by more than 0.1 N from the fourth simulate to the fifth (asserted below)."""
    n = 21
    root, dof, tau, mu, act = _row_lane_states(n, tgs)
    params = _params(tgs, substeps=substeps)
    default = _default_pos()
    a = torch.from_numpy(act[0]).to("cuda:0")

    def start():
        gym, sim = _make(monkeypatch, (4, 1), 1, n, params)
        H.load_state_into(sim, root, dof, mu)
        sim.refresh("dof")
        return gym, sim, torch.zeros((n, 12), device="cuda:0")

    def outputs(sim, torques):
        torch.cuda.synchronize()
        return [dict(state=RL._bits(sim.state), cf_soa=RL._bits(sim.cf_soa), cf_aos=RL._bits(sim.contact_tensor),
                     torques=RL._bits(torques))]

    gym, sim, torques = start()
    _pd(gym, sim, a, default, 4, 1, torques)
    fused = outputs(sim, torques)
    assert np.abs(fused[0]["cf_soa"].view(np.float32)).sum() > 0, "the states stand on the plane"

    gym, sim, torques = start()
    for _ in range(3):
        _pd(gym, sim, a, default, 1, 0, torques)  # (writes the dof tensor the next evaluation reads)
    _pd(gym, sim, a, default, 1, 1, torques)
    RL._assert_same(outputs(sim, torques), fused, f"fused step, {substeps} substeps, against separate fused launches")

    gym, sim, torques = start()
    for _ in range(4):
        _pd(gym, sim, a, default, 1, 0, torques)
    earlier = outputs(sim, torques)[0]["cf_soa"].view(np.float32)  # the forces of the fourth simulate
    sim.dof_force.copy_(torques.reshape(-1))
    gym.simulate(sim)
    sim.refresh("contact")
    plain = outputs(sim, torques)
    moved = np.abs(plain[0]["cf_soa"].view(np.float32) - earlier).max()
    assert moved > 0.1, f"the reference's forces move between simulates ({moved:.3g} N): stale forces would show"
    exact = not (tgs and substeps == 2)
    for name in ("cf_soa", "cf_aos"):
        x, y = fused[0][name].view(np.float32), plain[0][name].view(np.float32)
        words = int((fused[0][name] != plain[0][name]).sum())
        print(f"{name}: {words} words differ, max |d| {np.abs(x - y).max():.3g}")
        if exact:
            assert words == 0, f"{name} against a final plain simulate: {words} words differ"
        else:
            np.testing.assert_allclose(x, y, atol=1e-3, rtol=1e-5, err_msg=f"{name} against a final plain simulate")
    assert np.array_equal(fused[0]["torques"], plain[0]["torques"])


# ------------------------------------------------------------------ the selector
def test_resident_sweeps_are_off_outside_the_row_lane_form(monkeypatch):
    for form in ((16, 0), (8, 0), (4, 0)):
        _, sim = _make(monkeypatch, form, 1, 5, H.ANYMAL_PARAMS)
        assert _resident(sim) == 0, form
    _, sim = _make(monkeypatch, (4, 1), 1, 5, H.ANYMAL_PARAMS)
    assert _resident(sim) == 1
