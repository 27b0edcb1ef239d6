"""Launch constants of the lane-team kernels (gs_team.hip; DESIGN.md 5, "Launch constants").

What a launch reads that does not change while it runs -- the root body's model words, default_pos, the lane's
action words, the first evaluation's dof tensor -- is read once, before the staging barrier, and held (LDS tables,
registers in the plane forms, the lane's stash column in the trimesh forms).  Past the barrier the kernel loads
nothing of it again.  These tests pin what that must not change:

* the actions copy is the raw action words, whatever their bit patterns;
* the PD law, against float64 from the dof tensor that was passed in;
* a fused launch equals the same sim stepped by one-evaluation launches (the held words are the ones every
  evaluation would have loaded);
* nothing is held from one launch to the next: tensors overwritten in place are read afresh;
* every combination of the optional outputs leaves the remaining ones as they are;
* envs past N: partly empty waves and workgroups load and store nothing of theirs.

Both default forms run: plane <4 envs per wave, row lanes, resident sweeps> (actions in registers) and, over a rough
trimesh, the 16-envs-per-wave form (actions in the stash column).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_team_envs_per_wave_gpu as EW
from tests import test_team_row_lanes_gpu as RL

pytestmark = pytest.mark.gpu

KP, KD, SCALE, TLIM = 80.0, 2.0, 0.5, 80.0
# action words planted among uniform(-1, 1) ones: -0.0, float32 denormals (the smallest too), +-1, and +-10, which
# saturates the torque clamp whatever the dof (kp * scale * 10 = 400 against a limit of 80)
SPECIAL_BITS = np.array([0x80000000, 0x00011111, 0x80011111, 0x00000001, 0x3F800000, 0xBF800000, 0x41200000,
                         0xC1200000], dtype=np.uint32).view(np.int32)


def _actions(n, seed):
    a = np.random.RandomState(1000 + 7 * n + seed).uniform(-1, 1, (n, 12)).astype(np.float32)
    w = a.view(np.int32).reshape(-1)
    stride = max(1, w.size // len(SPECIAL_BITS))  # n = 1: words 0 .. 7 of the env's 12; every chain gets some
    w[(seed + np.arange(len(SPECIAL_BITS)) * stride) % w.size] = SPECIAL_BITS
    return a


@functools.lru_cache(maxsize=None)
def _default_np():
    art, _ = H.anymal()
    return np.array([H.ANYMAL_DEFAULT[d] for d in art.dof_names()], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _scene_states(n, tgs, trimesh):
    """test_team_row_lanes_gpu's seeded states (copies); over the trimesh, placed just above the mesh under each base
    as test_team_envs_per_wave_gpu places its own.  (A count that module does not seed: the first n of its 67.)"""
    root, dof, tau, mu, _ = RL._states(n if n in RL.COUNTS else 67, tgs)
    root, dof, mu = root[:n].copy(), dof[:n].copy(), mu[:n].copy()
    if trimesh:
        v = EW._terrain()["oracle"]["vertices"].reshape(-1, 3)
        root[:, 0:2] = np.random.RandomState(n).uniform(-5.0, 5.0, (n, 2))
        for i in range(n):
            near = (np.abs(v[:, 0] - root[i, 0]) < 0.15) & (np.abs(v[:, 1] - root[i, 1]) < 0.15)
            root[i, 2] += v[near, 2].mean() + 0.05
    return root, dof, mu


def _make(monkeypatch, n, tgs, trimesh, substeps=1):
    """A sim in the scene's default form."""
    for name in ("GS_TEAM_ENVS_PER_WAVE", "GS_TEAM_ROW_LANES", "GS_TEAM_RESIDENT_SWEEPS"):
        monkeypatch.delenv(name, raising=False)
    params = dict(H.ANYMAL_PARAMS, solver_type=1 if tgs else 0, substeps=substeps, has_ground=0 if trimesh else 1)
    gym, sim = H.make_gpu_sim("anymal", n, params, terrain=EW._terrain() if trimesh else None)
    assert sim.kernel_variant == 2
    assert RL._team_form(sim) == ((16, 0) if trimesh else (4, 1)), "the default form"
    return gym, sim


def _start(monkeypatch, n, tgs, trimesh, substeps=1, states=None):
    gym, sim = _make(monkeypatch, n, tgs, trimesh, substeps)
    root, dof, mu = states if states is not None else _scene_states(n, tgs, trimesh)
    H.load_state_into(sim, root, dof, mu)
    sim.refresh("dof")  # the first PD evaluation reads the dof tensor
    return gym, sim


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _launch(gym, sim, a, default, decimation, extra, torques, copy=None, write_root=True, write_contacts=True):
    gym.amd_pd_decimation_step(sim, a, default, KP, KD, SCALE, TLIM, decimation, extra, torques,
                               write_root=write_root, write_contacts=write_contacts, actions_copy_out=copy)
    torch.cuda.synchronize()


def _outputs(sim, torques, copy=None, root=True, contacts=True):
    out = dict(state=RL._bits(sim.state), dof=RL._bits(sim.dof_tensor), cf_soa=RL._bits(sim.cf_soa),
               torques=RL._bits(torques))
    if root:
        out["root"] = RL._bits(sim.root_tensor)
    if contacts:
        out["cf_aos"] = RL._bits(sim.contact_tensor)
    if copy is not None:
        out["actions"] = RL._bits(copy)
    assert np.isfinite(out["state"].view(np.float32)).all()
    return [out]


SCENES = pytest.mark.parametrize("trimesh", [False, True], ids=["plane", "trimesh"])


# ------------------------------------------------------------------ the copy is the raw words
@pytest.mark.parametrize("n", [1, 5, 21, 67])
@SCENES
def test_actions_copy_is_the_raw_action_words(trimesh, n, monkeypatch):
    gym, sim = _start(monkeypatch, n, True, trimesh)
    act = _actions(n, 0)
    torques = torch.zeros((n, 12), device="cuda:0")
    copy = torch.full((n, 12), float("nan"), device="cuda:0")
    _launch(gym, sim, _dev(act), _dev(_default_np()), 4, 1, torques, copy=copy)
    got = RL._bits(copy).reshape(n, 12)
    want = act.view(np.int32)
    assert set(SPECIAL_BITS.tolist()) <= set(want.reshape(-1).tolist())
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, f"{bad[0].size} words of the actions copy differ, first at {[int(x[0]) for x in bad]}"


# ------------------------------------------------------------------ the PD law
@SCENES
def test_pd_law_against_float64(trimesh, monkeypatch):
    """One evaluation, one simulate: torques_out against the law in float64 from the dof tensor passed in.  Allowance
    per element 4 * 2^-23 * (kp (|scale a| + |default| + |q|) + kd |qd|): the expression's float32 roundings, with
    contraction on or off; an entry whose float64 value is past the limit by more than that equals the limit."""
    n = 21
    gym, sim = _start(monkeypatch, n, True, trimesh)
    act, default = _actions(n, 1), _default_np()
    dof_in = sim.dof_tensor.detach().cpu().numpy().astype(np.float64).reshape(n, 12, 2)
    torques = torch.full((n, 12), float("nan"), device="cuda:0")
    _launch(gym, sim, _dev(act), _dev(default), 1, 0, torques)
    got = torques.cpu().numpy().astype(np.float64)
    a, d = act.astype(np.float64), default.astype(np.float64)[None, :]
    q, qd = dof_in[:, :, 0], dof_in[:, :, 1]
    raw = KP * (SCALE * a + d - q) - KD * qd
    allow = 4 * 2.0 ** -23 * (KP * (np.abs(SCALE * a) + np.abs(d) + np.abs(q)) + KD * np.abs(qd))
    want = np.clip(raw, -TLIM, TLIM)
    err = np.abs(got - want)
    sure = np.abs(raw) > TLIM + allow
    print(f"max err / allowance {np.max(err / allow):.3g}; {int(sure.sum())} entries clamped, "
          f"{int((~sure).sum())} not")
    assert sure.sum() >= 2 and (raw[sure] > 0).any() and (raw[sure] < 0).any(), "the inputs saturate both limits"
    assert np.array_equal(got[sure], np.sign(raw[sure]) * TLIM), "clamped entries equal the limit exactly"
    assert (np.abs(got) <= TLIM).all()
    bad = np.nonzero(err > allow)
    assert bad[0].size == 0, f"{bad[0].size} torques off the float64 law, first at {[int(x[0]) for x in bad]}"


# ------------------------------------------------------------------ held over the launch
HELD = [(False, it, sub, tgs) for it in [(1, 0), (1, 1), (2, 0), (4, 1)] for sub in (1, 2) for tgs in (False, True)]
HELD += [(True, (4, 1), sub, tgs) for sub in (1, 2) for tgs in (False, True)]


@pytest.mark.parametrize("trimesh,iters,substeps,tgs", HELD,
                         ids=[f"{'trimesh' if t else 'plane'}-{i[0]}+{i[1]}-sub{s}-{'tgs' if g else 'pgs'}"
                              for t, i, s, g in HELD])
def test_fused_launch_equals_one_evaluation_launches(trimesh, iters, substeps, tgs, monkeypatch):
    """(after test_fused_step_forces_equal_those_of_separate_launches) decimation - 1 launches of one evaluation + one
    simulate, then one of one evaluation + 1 + extra simulates, each of which loads the action words afresh."""
    n = 5
    decimation, extra = iters
    a, default = _dev(_actions(n, 2)), _dev(_default_np())

    gym, sim = _start(monkeypatch, n, tgs, trimesh, substeps)
    torques = torch.zeros((n, 12), device="cuda:0")
    _launch(gym, sim, a, default, decimation, extra, torques)
    fused = _outputs(sim, torques)

    gym, sim = _start(monkeypatch, n, tgs, trimesh, substeps)
    torques = torch.zeros((n, 12), device="cuda:0")
    for _ in range(decimation - 1):
        _launch(gym, sim, a, default, 1, 0, torques)  # (writes the dof tensor the next evaluation reads)
    _launch(gym, sim, a, default, 1, extra, torques)
    RL._assert_same(_outputs(sim, torques), fused, f"fused {decimation}+{extra}, {substeps} substeps")


# ------------------------------------------------------------------ nothing survives a launch
@SCENES
def test_tensors_overwritten_in_place_are_read_afresh(trimesh, monkeypatch):
    n = 21
    gym, sim = _start(monkeypatch, n, True, trimesh)
    a = torch.zeros((n, 12), device="cuda:0")
    default = torch.zeros(12, device="cuda:0")
    torques = torch.zeros((n, 12), device="cuda:0")
    copy = torch.zeros((n, 12), device="cuda:0")
    ptrs = (a.data_ptr(), default.data_ptr())
    for k, shift in enumerate((0.0, 0.1, -0.1)):
        act_k, default_k = _actions(n, 10 + k), (_default_np() + np.float32(shift)).astype(np.float32)
        a.copy_(_dev(act_k))
        default.copy_(_dev(default_k))
        assert (a.data_ptr(), default.data_ptr()) == ptrs
        state0, dof0, mu0 = sim.state.clone(), sim.dof_tensor.clone(), sim.shape_mu.clone()
        _launch(gym, sim, a, default, 4, 1, torques, copy=copy)
        got = _outputs(sim, torques, copy=copy)

        gym2, sim2 = _make(monkeypatch, n, True, trimesh)
        sim2.state.copy_(state0)
        sim2.shape_mu.copy_(mu0)
        sim2.dof_tensor.copy_(dof0)
        torques2 = torch.zeros((n, 12), device="cuda:0")
        copy2 = torch.zeros((n, 12), device="cuda:0")
        _launch(gym2, sim2, _dev(act_k), _dev(default_k), 4, 1, torques2, copy=copy2)
        RL._assert_same(_outputs(sim2, torques2, copy=copy2), got, f"launch {k} against a fresh sim")


# ------------------------------------------------------------------ optional outputs
@SCENES
def test_optional_outputs_leave_the_others_as_they_are(trimesh, monkeypatch):
    n = 5
    a, default = _dev(_actions(n, 3)), _dev(_default_np())

    def run(root, contacts, with_copy):
        gym, sim = _start(monkeypatch, n, True, trimesh)
        torques = torch.zeros((n, 12), device="cuda:0")
        copy = torch.zeros((n, 12), device="cuda:0") if with_copy else None
        _launch(gym, sim, a, default, 4, 1, torques, copy=copy, write_root=root, write_contacts=contacts)
        return _outputs(sim, torques, copy=copy, root=root, contacts=contacts)

    full = run(True, True, True)
    for root, contacts, with_copy in itertools.product((True, False), repeat=3):
        got = run(root, contacts, with_copy)
        want = [{name: full[0][name] for name in got[0]}]
        assert len(want[0]) == 4 + root + contacts + with_copy
        RL._assert_same(want, got, f"write_root={root}, write_contacts={contacts}, actions copy={with_copy}")


# ------------------------------------------------------------------ envs past N
@pytest.mark.parametrize("n", [1, 17])
@SCENES
def test_partly_empty_waves_and_workgroups(trimesh, n, monkeypatch):
    """n = 1 and 17 (16 envs to a workgroup: the last wave and the last workgroup are partly empty) against the first n
    envs of a run at 32 with the same states."""
    m = 32
    root, dof, mu = _scene_states(m, True, trimesh)
    act, default = _actions(m, 4), _dev(_default_np())

    def run(k):
        gym, sim = _start(monkeypatch, k, True, trimesh, states=(root[:k], dof[:k], mu[:k]))
        torques = torch.zeros((k, 12), device="cuda:0")
        copy = torch.zeros((k, 12), device="cuda:0")
        _launch(gym, sim, _dev(act[:k]), default, 4, 1, torques, copy=copy)
        out = _outputs(sim, torques, copy=copy)[0]
        for name, w in out.items():
            assert np.isfinite(w.view(np.float32)).all(), name
            # state and cf_soa are [row][env]; the others [env][...]
            out[name] = w.reshape(-1, k)[:, :n] if name in ("state", "cf_soa") else w.reshape(k, -1)[:n]
        return [out]

    RL._assert_same(run(m), run(n), f"{n} envs against the first {n} of {m}")
