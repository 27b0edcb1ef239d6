"""Envs per wave of the lane-team kernels (gs_team.hip WaveForm): the 8 and 4 forms against the 16 form.

A workgroup holds 16 envs in every form; with 8 or 4 envs per wave it runs 2 or 4 waves, each on lanes 0 .. 4 EPW - 1
and on its own slice of the workgroup's LDS tables.  Per-env arithmetic is the same statements in the same order, so
every output must be bit-identical, whatever envs share a wave -- a difference in any bit is a bug (a coupling between
the envs of a wave, or between the waves of a workgroup), never a tolerance question.

Covered: gs_sim_pd_step (4 PD + 5 simulates) and plain simulate, PGS and TGS, plane and trimesh, three consecutive
steps from randomised states, at N = 1, 5, 16, 21 and 67 envs (a single team, a ragged wave, a full workgroup, a ragged
workgroup, counts that are no multiple of 4, 8 or 16).  Envs with crossed legs -- self-collision narrowphase entered,
pool full -- sit first, last and (N = 1; the last env of N = 5 and 21 in the 4 form) alone in their wave.

The fused tail (GS_FUSED_TAIL=1) at N = 21 and 67 under the default form: reset masks and count equal the separate
k_post_a launch's.
"""
import functools

import numpy as np
import pytest
import torch

from oracle.oracle import OracleSim
from tests import helpers as H

pytestmark = pytest.mark.gpu

COUNTS = [1, 5, 16, 21, 67]
STEPS = 3


@functools.lru_cache(maxsize=None)
def _crossed():
    """ANYmal states with crossed legs (after tests/test_self_collision.py crossed_leg_states): 3 whose self-contact
    pool is full (4 contacts, the oracle's count) and 3 with at least one contact."""
    art, flat = H.anymal()
    m = 600
    rng = np.random.RandomState(5)
    root, dof, tau, mu = H.anymal_states(m, seed=5)
    dof[:, :, 0] += rng.uniform(-1.8, 1.8, (m, 12))
    _, cnt = OracleSim(flat, H.ANYMAL_PARAMS).self_contacts(root, dof, mu)
    full, some = np.nonzero(cnt >= 4)[0][:3], np.nonzero((cnt >= 1) & (cnt < 4))[0][:3]
    assert len(full) == 3 and len(some) == 3
    idx = np.array([full[0], some[0], full[1], some[1], full[2], some[2]])
    return root[idx], dof[idx], tau[idx], mu[idx]


@functools.lru_cache(maxsize=None)
def _terrain():
    return H.rough_terrain(seed=5)


@functools.lru_cache(maxsize=None)
def _states(n, trimesh):
    """Randomised states, the crossed-leg ones first, last and at the first env of the second 8-env wave."""
    root, dof, tau, mu = H.anymal_states(n, seed=17 + n)
    c_root, c_dof, c_tau, c_mu = _crossed()
    places = sorted({0, n - 1} | ({8, 12, n - 2} if n >= 16 else set()))
    for k, i in enumerate(places):
        xy = root[i, 0:2].copy()
        root[i], dof[i], tau[i], mu[i] = c_root[k], c_dof[k], c_tau[k], c_mu[k]
        root[i, 0:2] = xy
    if trimesh:  # just above the mesh under each base (tests/test_terrain_gpu.py)
        v = _terrain()["oracle"]["vertices"].reshape(-1, 3)
        rng = np.random.RandomState(n)
        root[:, 0:2] = rng.uniform(-5.0, 5.0, (n, 2))
        for i in range(n):
            near = (np.abs(v[:, 0] - root[i, 0]) < 0.15) & (np.abs(v[:, 1] - root[i, 1]) < 0.15)
            root[i, 2] += v[near, 2].mean() + 0.05
    act = np.random.RandomState(3 * n).uniform(-1, 1, (STEPS, n, 12)).astype(np.float32)
    return root, dof, tau, mu, act


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _run(monkeypatch, epw, n, trimesh, tgs, mode):
    """Every output of STEPS steps of the form with `epw` envs per wave, as int32 bit patterns."""
    monkeypatch.setenv("GS_TEAM_ENVS_PER_WAVE", str(epw))  # read once, at sim creation
    params = dict(H.ANYMAL_PARAMS, solver_type=1 if tgs else 0, has_ground=0 if trimesh else 1)
    gym, sim = H.make_gpu_sim("anymal", n, params, terrain=_terrain() if trimesh else None)
    assert sim.kernel_variant == 2
    root, dof, tau, mu, act = _states(n, trimesh)
    H.load_state_into(sim, root, dof, mu)
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
    return out


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
@pytest.mark.parametrize("trimesh", [False, True], ids=["plane", "trimesh"])
def test_narrow_forms_are_bit_identical_to_the_16_form(trimesh, tgs, n, monkeypatch):
    for mode in ("pd", "simulate"):
        ref = _run(monkeypatch, 16, n, trimesh, tgs, mode)
        if n >= 16:  # the states do what they are for: contact forces, and self-contacts that change the result
            assert np.abs(ref[-1]["cf_soa"].view(np.float32)).sum() > 0
        for epw in (8, 4):
            got = _run(monkeypatch, epw, n, trimesh, tgs, mode)
            for k, (a, b) in enumerate(zip(ref, got)):
                for name in a:
                    bad = np.nonzero(a[name] != b[name])
                    assert a[name].shape == b[name].shape and bad[0].size == 0, (
                        f"{mode} step {k}, {epw} envs per wave: {name} differs from the 16 form in {bad[0].size} "
                        f"words, first at {[int(x[0]) for x in bad]}")


def test_crossed_leg_states_enter_the_narrowphase(monkeypatch):
    """The states above do fill self-contact pools in the kernel under test (gs_debug_self_contacts)."""
    monkeypatch.setenv("GS_TEAM_ENVS_PER_WAVE", "4")
    n = 21
    gym, sim = H.make_gpu_sim("anymal", n, H.ANYMAL_PARAMS)
    root, dof, tau, mu, _ = _states(n, False)
    H.load_state_into(sim, root, dof, mu)
    _, cnt = H.sim_self_contacts(sim)
    assert cnt.max() == 4 and cnt[0] >= 1 and cnt[8] >= 1 and cnt[n - 1] >= 1 and (cnt > 0).sum() >= 5


@pytest.mark.parametrize("n", [21, 67])
def test_fused_tail_masks_and_count_equal_post_a_at_ragged_counts(n, monkeypatch):
    """post_a in the physics launch (which runs the 16 form for it) against the separate k_post_a launch under the
    default envs per wave, at env counts that end inside a wave's 16-env slice of the reset masks."""
    from tests.test_task_gpu import _make, _restore, _snapshot
    monkeypatch.delenv("GS_TEAM_ENVS_PER_WAVE", raising=False)
    monkeypatch.setenv("GS_FUSED_TAIL", "1")
    env = _make("AnymalTerrain", n, monkeypatch, **{"task.env.learn.episodeLength_s": 0.1})
    assert env.gym.amd_pd_tail_supported(env.sim)
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    acts = [2 * torch.rand((n, 12), device="cuda:0", generator=gen) - 1 for _ in range(8)]
    env.step(acts[0])
    snap = _snapshot(env)
    kernels = env._kernels
    out, fused_steps = {}, {}
    for mode in ("fused", "separate"):
        _restore(env, snap)
        kernels._tail_ok = None if mode == "fused" else False
        res, n0 = [], env.fused_tail_steps
        for a in acts:
            obs, rew, reset, extras = env.step(a)
            res.append([reset.clone(), kernels.reset_masks.clone(), torch.tensor(getattr(kernels, "last_reset_count", -1)),
                        obs["obs"].clone(), rew.clone(), env.progress_buf.clone()])
            env.extras.pop("episode", None)
        out[mode] = res
        fused_steps[mode] = env.fused_tail_steps - n0
    kernels._tail_ok = None
    assert fused_steps["separate"] == 0 and fused_steps["fused"] >= len(acts) - 1, fused_steps
    resets = 0
    for t, (a, b) in enumerate(zip(out["fused"], out["separate"])):
        resets += int(a[2])
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {t} output {k}"
    assert resets >= n, "every env was reset at least once in the window"
