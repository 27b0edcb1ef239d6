"""oracle/task_oracle.py (the float64 / float32 restatement of include/gymtask.h's AnymalTerrain tail) tied to the
reference's recorded results, and every claim of the input generators of tests/helpers.py that
tests/test_task_kernels_gpu.py relies on.  CPU only.

The golden fixtures hold the reference's own float32 results of whole post_physics_steps: the float32 oracle replays
them from the in_* arrays (post_a; the push, reset_idx and the noise with the draws of the recorded CPU generator
state; post_b) to the bar those fixtures already carry, integers exactly and floats within rtol 1e-5.
"""
import os

import numpy as np
import pytest
import yaml

from oracle import task_oracle as O
from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS = (1, 15, 17, 63, 64, 65, 130, 4161)
K = len(H.TAIL_KINDS)
F32, F64 = np.float32, np.float64


def _close(a, b, what, rtol=1e-5, atol=2e-6):
    np.testing.assert_allclose(np.asarray(a, dtype=F64), np.asarray(b, dtype=F64), rtol=rtol, atol=atol, err_msg=what)


def _params_from_cfg(cfg, N, nb, names, feet, knees, hound=False):
    env, learn = cfg["env"], cfg["env"]["learn"]
    dt = env["control"]["decimation"] * cfg["sim"]["dt"]
    keys = dict(s_termination="terminalReward", s_lin_vel_xy="linearVelocityXYRewardScale",
                s_lin_vel_z="linearVelocityZRewardScale", s_ang_vel_z="angularVelocityZRewardScale",
                s_ang_vel_xy="angularVelocityXYRewardScale", s_orient="orientationRewardScale",
                s_torque="torqueRewardScale", s_joint_acc="jointAccRewardScale", s_base_height="baseHeightRewardScale",
                s_air_time="feetAirTimeRewardScale", s_collision="kneeCollisionRewardScale",
                s_stumble="feetStumbleRewardScale", s_action_rate="actionRateRewardScale", s_hip="hipRewardScale")
    init = env["baseInitState"]
    default = [float(env["defaultJointAngles"][n]) for n in names[:12]]
    p = dict(num_envs=N, num_dofs=12, num_bodies=nb, num_obs=204 if hound else 188, base_index=0, num_feet=len(feet),
             feet_idx=[int(x) for x in feet], num_knees=len(knees), knee_idx=[int(x) for x in knees],
             allow_knee_contacts=int(bool(learn["allowKneeContacts"])),
             max_episode_length=int(learn["episodeLength_s"] / dt + 0.5),
             dt=cfg["sim"]["dt"],  # VecTask.__init__ rebinds self.dt to the sim's dt after the scales were made
             lin_vel_scale=learn["linearVelocityScale"], ang_vel_scale=learn["angularVelocityScale"],
             dof_pos_scale=learn["dofPositionScale"], dof_vel_scale=learn["dofVelocityScale"],
             height_meas_scale=learn["heightMeasurementScale"], default_dof_pos=default + [0.0] * 4,
             base_init_state=init["pos"] + init["rot"] + init["vLinear"] + init["vAngular"])
    p.update({k: learn[v] * dt for k, v in keys.items()})
    return p


def _step_bufs(d, t, N, na):
    to = d["in_timeout"][t]
    return dict(root_states=d["in_root"][t].copy(), contact_forces=d["in_contact"][t],
                dof_state=d["in_dof"][t].reshape(N, na, 2), torques=d["in_torques"][t], actions=d["in_actions"][t],
                last_actions=d["in_last_actions"][t], last_dof_vel=d["in_last_dof_vel"][t],
                commands=d["in_commands"][t], feet_air_time=d["in_feet_air_time"][t], progress_buf=d["in_progress"][t],
                randomize_buf=np.zeros(N, np.int64), timeout_buf=to if d["in_timeout_is_long"][t] else to.astype(bool),
                episode_sums=d["in_episode_sums"][t], reset_buf=np.zeros(N, np.uint8))


@pytest.mark.parametrize("fixture", ["anymal_terrain.npz", "anymal_terrain_long.npz"])
def test_float32_oracle_replays_the_anymal_fixtures(fixture):
    """Whole steps: the push, post_a, reset_idx on the recorded generator's draws, the noise, post_b."""
    import torch
    d = np.load(os.path.join(GOLDEN, fixture))
    cfg = yaml.safe_load(str(d["cfg_yaml"]))
    learn = cfg["env"]["learn"]
    art, _ = H.anymal()
    T, N = d["actions"].shape[:2]
    p = _params_from_cfg(cfg, N, d["in_contact"].shape[2], art.dof_names(), d["feet_indices"], d["knee_indices"])
    rg = cfg["env"]["randomCommandVelocityRanges"]
    maps = dict(pos_range=1.5 - 0.5, pos_lower=0.5, vel_range=0.1 - -0.1, vel_lower=-0.1)
    for n, key in (("cmd_x", "linear_x"), ("cmd_y", "linear_y"), ("cmd_h", "yaw")):
        maps[n + "_range"], maps[n + "_lower"] = float(rg[key][1] - rg[key][0]), float(rg[key][0])
    resets = 0
    for t in range(T):
        b = _step_bufs(d, t, N, 12)
        torch.set_rng_state(torch.from_numpy(d["in_rng_state"][t]))
        if d["in_push"][t]:
            b["root_states"][:, 7:9] = (2.0 * torch.rand(N, 2) + -1.0).numpy()
        a = O.post_a(p, b, dtype=F32)
        np.testing.assert_array_equal(a["reset_buf"], d["reset"][t], err_msg=f"reset step {t}")
        _close(a["rew_buf"], d["rew"][t], f"reward step {t}")
        _close(a["base_lin_vel"], d["out_base_lin_vel"][t], f"base_lin_vel step {t}")
        _close(a["base_ang_vel"], d["out_base_ang_vel"][t], f"base_ang_vel step {t}")
        _close(a["projected_gravity"], d["out_projected_gravity"][t], f"gravity step {t}")
        nb = dict(b, commands=a["commands"], feet_air_time=a["feet_air_time"], progress_buf=a["progress_buf"],
                  reset_buf=a["reset_buf"], episode_sums=a["episode_sums"])
        k = a["count"]
        if k:
            resets += k
            u = lambda *s: torch.rand(*s).numpy()  # noqa: E731
            draws = dict(maps, u_pos=u(k, 12), u_vel=u(k, 12), u_cmd_x=u(k, 1), u_cmd_y=u(k, 1), u_cmd_h=u(k, 1))
            r = O.reset_flagged(p, nb, a["reset_masks"], draws, episode_length_s=learn["episodeLength_s"], dtype=F32)
            np.testing.assert_array_equal(r["env_ids"], np.nonzero(d["reset"][t])[0])
            nb.update({f: r[f] for f in ("root_states", "dof_state", "commands", "last_actions", "last_dof_vel",
                                         "feet_air_time", "progress_buf", "reset_buf", "episode_sums")})
            assert d["ep_mask"][t]
            _close(r["episode_out"], d["ep_extras"][t][:13], f"extras step {t}", rtol=1e-4, atol=1e-7)
        np.testing.assert_array_equal(nb["progress_buf"], d["progress"][t], err_msg=f"progress step {t}")
        _close(nb["commands"], d["commands"][t], f"commands step {t}")
        _close(nb["feet_air_time"], d["feet_air_time"][t], f"air time step {t}")
        _close(nb["episode_sums"], d["episode_sums"][t], f"episode sums step {t}")
        _close(nb["root_states"], d["out_root"][t], f"root step {t}")
        _close(np.asarray(nb["dof_state"]).reshape(-1, 2), d["out_dof"][t], f"dof step {t}")
        nb.update(base_lin_vel=a["base_lin_vel"], base_ang_vel=a["base_ang_vel"],
                  projected_gravity=a["projected_gravity"], noise_scale=d["noise_scale_vec"], measured_heights=None)
        noise = torch.rand(N, 188).numpy() if learn["addNoise"] else None
        o = O.post_b(p, nb, noise, dtype=F32)
        _close(o["obs_buf"], d["obs"][t], f"obs step {t}")
        np.testing.assert_array_equal(o["time_outs"], d["time_outs"][t], err_msg=f"time_outs step {t}")
        _close(o["last_actions"], d["out_last_actions"][t], f"last_actions step {t}")
        _close(o["last_dof_vel"], d["out_last_dof_vel"][t], f"last_dof_vel step {t}")
    assert resets > 0


def test_float32_oracle_replays_the_hound_fixture_part_a():
    """UsefulHound: post_a's results on every recorded step (reset and reward of every env; the carried fields of the
    envs that were not reset afterwards -- the fixture's outputs are taken after reset_idx, whose arm and arm-command
    draws it does not record one by one)."""
    d = np.load(os.path.join(GOLDEN, "useful_hound.npz"))
    cfg = yaml.safe_load(str(d["cfg_yaml"]))
    art, _ = H.hound()
    T, N = d["actions"].shape[:2]
    p = _params_from_cfg(cfg, N, d["in_contact"].shape[2], art.dof_names(), d["feet_indices"], d["knee_indices"], True)
    hound = dict(num_actions=18, num_shoulders=len(d["base_indices"]), shoulder_idx=[int(x) for x in d["base_indices"]])
    seen_reset = 0
    for t in range(T):
        if d["in_push"][t]:
            continue  # the push draws precede post_a and are not stored
        a = O.post_a(p, _step_bufs(d, t, N, 18), hound=hound, dtype=F32)
        np.testing.assert_array_equal(a["reset_buf"], d["reset"][t], err_msg=f"reset step {t}")
        _close(a["rew_buf"], d["rew"][t], f"reward step {t}")
        keep = d["reset"][t] == 0
        seen_reset += int((~keep).sum())
        np.testing.assert_array_equal(a["progress_buf"][keep], d["progress"][t][keep])
        _close(a["commands"][keep], d["commands"][t][keep], f"commands step {t}")
        _close(a["feet_air_time"][keep], d["feet_air_time"][t][keep], f"air time step {t}")
        _close(a["episode_sums"][:, keep], d["episode_sums"][t][:, keep], f"episode sums step {t}")
    assert seen_reset > 0


def test_float32_oracle_reproduces_the_trimesh_fixture_heights():
    """anymal_trimesh.npz records the root states and the measured heights of every step (not the pre-reset inputs
    the terrain curriculum reads, so the level update is not replayed from it)."""
    d = np.load(os.path.join(GOLDEN, "anymal_trimesh.npz"))
    y = 0.1 * np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5])
    x = 0.1 * np.array([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8])
    gx, gy = np.meshgrid(x.astype(F32), y.astype(F32), indexing="ij")
    T, N = d["heights"].shape[:2]
    pts = np.zeros((N, 140, 3), F32)
    pts[:, :, 0], pts[:, :, 1] = gx.flatten(), gy.flatten()
    for t in range(T):
        _, _, h, _ = O.measure_heights(d["height_samples"], 20.0, 0.1, 0.005, d["root_states"][t], pts, F32)
        np.testing.assert_array_equal(h, d["heights"][t], err_msg=f"heights step {t}")


# ------------------------------------------------------------------------------------------- the generators' claims
def _margin(x, thr, tie=None):
    """Every element of x at least TAIL_MARGIN (relative to thr) from thr, or exactly on it where tie is set."""
    x = np.asarray(x, F64)
    far = np.abs(x - thr) >= H.TAIL_MARGIN * max(abs(thr), 1e-30)
    if tie is None:
        return bool(far.all())
    tie = np.broadcast_to(tie, x.shape)
    return bool((far | tie).all()) and bool((x[tie] == thr).all())


@pytest.mark.parametrize("hound", [False, True])
@pytest.mark.parametrize("N", NS)
def test_tail_inputs_hold_what_they_claim(N, hound):
    p, b, kind = H.tail_inputs(N, 12, seed=N, hound=hound)
    hd = H.tail_hound(N) if hound else None
    o = O.post_a(p, b, hound=hd)
    is_ = lambda name: kind == H.TAIL_KINDS.index(name)  # noqa: E731
    np.testing.assert_array_equal(kind, np.arange(N) % K)
    cf = b["contact_forces"].astype(F64)
    nrm = np.sqrt((cf * cf).sum(-1))
    bd = H.TAIL_BODIES["hound" if hound else "anymal"]
    tie_n = np.zeros(nrm.shape, bool)
    tie_n[is_("tie_norm"), bd["base"]] = True
    tie_n[is_("tie_norm"), bd["knees"][0]] = True
    watched = [bd["base"]] + list(bd["knees"]) + list(bd.get("shoulders", ()))
    assert _margin(nrm[:, watched], 1.0, tie_n[:, watched])
    feet = list(bd["feet"])
    fz = cf[:, feet, 2]
    tie_z = np.repeat(is_("tie_z")[:, None], 4, 1)
    assert _margin(fz, 1.0, tie_z) and _margin(np.abs(fz), 1.0, tie_z)
    assert _margin(np.sqrt(cf[:, feet, 0] ** 2 + cf[:, feet, 1] ** 2), 5.0)
    air = b["feet_air_time"].astype(F64)
    assert ((air == 0) | (air >= 0.02)).all()
    cmd = b["commands"].astype(F64)
    assert _margin(np.sqrt(cmd[:, 0] ** 2 + cmd[:, 1] ** 2), 0.1)
    diff = cmd[:, 3] - o["heading"]
    for thr in (np.pi, -np.pi, 2 * np.pi, -2 * np.pi, 2.0, -2.0):
        assert _margin(diff, thr), thr
    # wrapped: the clamp's thresholds on the wrapped angle
    ang = np.fmod(diff, 2 * np.pi)
    ang = ang - 2 * np.pi * (ang > np.pi)
    assert _margin(0.5 * ang, 1.0) and _margin(0.5 * ang, -1.0)
    T = p["max_episode_length"]
    prog = b["progress_buf"] + 1
    assert (prog[is_("prog_at")] == T - 1).all() and (prog[is_("prog_below")] == T - 2).all()
    assert (prog[~is_("prog_at")] < T - 1).all()
    # the reward before its clip: at least TAIL_MARGIN of the sum of the terms' magnitudes from 0
    mag = sum(np.abs(v) for v in o["terms"].values())
    assert (np.abs(o["rew_preclip"]) >= H.TAIL_MARGIN * mag).all()
    if N < K:
        return
    # every kind present, and does what it says
    assert np.bincount(kind, minlength=K).min() >= N // K >= 1
    rst = o["reset_buf"].astype(bool)
    for name in ("base_contact", "knee_one", "knee_many", "prog_at", "timeout_reset"):
        assert rst[is_(name)].all(), name
    assert rst[is_("shoulder")].all() == hound and (o["sh_count"][is_("shoulder")] == (1 if hound else 0)).all()
    for name in ("ordinary", "tie_norm", "tie_z", "stumble_one", "prog_below", "reward_clip", "timeout_only",
                 "heading_below_minus_pi", "small_cmd"):
        assert not rst[is_(name)].any(), name
    assert (o["knee_count"][is_("knee_one")] == 1).all() and (o["knee_count"][is_("knee_many")] == 4).all()
    assert (o["knee_count"][is_("tie_norm")] == 0).all()
    assert not o["contact"][is_("tie_z")].any() and (o["stumble"][is_("tie_z")] == 0).all()
    assert (o["stumble"][is_("stumble_one")] == 1).all() and (o["stumble"][is_("stumble_many")] == 4).all()
    assert o["first"][is_("first_contact")].all() and o["contact"][is_("contact_zero_air")].all()
    assert not o["first"][is_("contact_zero_air")].any()
    assert o["first"][is_("small_cmd")].all() and not o["cmd_gate"][is_("small_cmd")].any()
    assert o["cmd_gate"][is_("first_contact")].all() and (o["terms"]["air_time"][is_("first_contact")] != 0).all()
    assert (o["terms"]["air_time"][is_("small_cmd")] == 0).all()
    assert (o["wrap_side"][is_("heading_above_pi")] == 1).all()
    assert (o["wrap_side"][is_("heading_below_minus_pi")] == -1).all()
    assert (o["c2_clamp"][is_("heading_below_minus_pi")] == -1).all()
    assert (o["c2_clamp"][is_("c2_high")] == 1).all() and (o["c2_clamp"][is_("c2_low")] == -1).all()
    assert (o["c2_clamp"][is_("ordinary")] == 0).all() and (o["c2_clamp"][is_("heading_above_pi")] == 0).all()
    assert o["rew_clipped"][is_("reward_clip")].all() and (o["rew_buf"][is_("reward_clip")] == 0).all()
    assert not o["rew_clipped"][is_("ordinary")].any()
    # termination with the time-out flag set leaves the reward alone; without it the penalty is paid
    assert (o["rew_buf"][is_("timeout_reset")] == np.maximum(o["rew_preclip"][is_("timeout_reset")], 0)).all()
    assert (o["rew_buf"][is_("base_contact")] < np.maximum(o["rew_preclip"][is_("base_contact")], 0)).all()
    # both ways, over the whole batch
    for name in ("reset_buf", "rew_clipped", "cmd_gate"):
        v = np.asarray(o[name]).astype(bool)
        assert v.any() and not v.all(), name
    for name in ("first", "contact"):
        assert o[name].any() and not o[name].all(), name
    assert set(np.unique(o["wrap_side"])) == {-1, 0, 1} and set(np.unique(o["c2_clamp"])) == {-1, 0, 1}
    assert (o["stumble"] > 0).any() and (o["knee_count"] > 0).any()


@pytest.mark.parametrize("hound", [False, True])
@pytest.mark.parametrize("N", NS)
def test_precisions_agree_on_every_discrete_output(N, hound):
    """reset, counts, masks, ids, decisions, levels: float32 and float64 agree on every generated env (none left out)."""
    p, b, _ = H.tail_inputs(N, 12, seed=N, hound=hound)
    hd = H.tail_hound(N) if hound else None
    for over in (dict(), dict(timeout_buf=b["timeout_buf"].astype(np.int64))):
        bb = dict(b, **over)
        o64, o32 = O.post_a(p, bb, hound=hd), O.post_a(p, bb, hound=hd, dtype=F32)
        for f in ("reset_buf", "progress_buf", "randomize_buf", "reset_masks", "knee_count", "sh_count", "stumble",
                  "first", "contact", "rew_clipped", "wrap_side", "c2_clamp", "cmd_gate"):
            np.testing.assert_array_equal(o64[f], o32[f], err_msg=f)
        assert o64["count"] == o32["count"] == H.popcount(o64["reset_masks"])
    nb = dict(b, base_lin_vel=o64["base_lin_vel"], base_ang_vel=o64["base_ang_vel"],
              projected_gravity=o64["projected_gravity"], commands=o64["commands"], progress_buf=o64["progress_buf"],
              reset_buf=o64["reset_buf"])
    hb = dict(hd, eef=hd["eef_rows"][:, :7]) if hound else None
    np.testing.assert_array_equal(O.post_b(p, nb, hound=hb)["time_outs"], O.post_b(p, nb, hound=hb, dtype=F32)["time_outs"])


@pytest.mark.parametrize("N", [1, 63, 65, 130, 4161])
def test_reset_inputs_hold_what_they_claim(N):
    cases = H.reset_masks_cases(N)
    W = (N + 63) // 64
    assert {"none", "all", "first", "last", "alternating"} <= set(cases)
    assert (N > 4096) == ("last_wave" in cases) == ("first_and_last_wave" in cases)
    for name, m in cases.items():
        assert m.dtype == np.uint64 and m.shape == (W,)
        ids = O.ids_of(m, 64 * W)
        assert (ids < N).all(), name
        assert len(ids) == H.popcount(m)
    assert H.popcount(cases["none"]) == 0 and H.popcount(cases["all"]) == N
    assert O.ids_of(cases["first"], N).tolist() == [0] and O.ids_of(cases["last"], N).tolist() == [N - 1]
    assert O.ids_of(cases["alternating"], N).tolist() == list(range(0, N, 2))
    if N > 4096:
        assert O.ids_of(cases["last_wave"], N).min() >= 64 * (W - 1) and W > 64
        fl = O.ids_of(cases["first_and_last_wave"], N)
        assert fl.min() < 64 and fl.max() >= 64 * (W - 1) and ((fl < 64) | (fl >= 64 * (W - 1))).all()
    # the terrain states: every branch of the curriculum, the same in both precisions
    p, b, _ = H.tail_inputs(N, 12, seed=N)
    for name in ("all", "alternating") + (("first_and_last_wave",) if N > 4096 else ()):
        m = cases[name]
        ids = O.ids_of(m, N)
        k = len(ids)
        flagged = np.zeros(N, bool)
        flagged[ids] = True
        d, extra = H.reset_draws(k, 12, terrain=True)
        for batch_norm in (0.4, 2.0):
            tr, root_xy, cmd_xy, state = H.terrain_reset_inputs(N, ids, batch_norm=batch_norm)
            b["root_states"][:, :2], b["commands"][:, :2] = root_xy, cmd_xy
            # the claims: the batch's norm, the walks' margins from both thresholds, the other envs' commands
            c = b["commands"][ids, :2].astype(F64)
            assert abs(np.sqrt((c * c).sum()) - batch_norm) < 1e-5 * batch_norm
            walked = np.linalg.norm(b["root_states"][:, :2].astype(F64) - tr["env_origins"][:, :2].astype(F64), axis=1)
            assert _margin(walked, 5.0 * batch_norm) and _margin(walked, tr["env_length"] / 2)
            assert (np.linalg.norm(b["commands"][~flagged, :2], axis=1) == 10).all()
            outs = [O.reset_flagged(p, b, m, d, terrain=dict(tr, **extra), dtype=dt) for dt in (F64, F32)]
            for f in ("env_ids", "terrain_levels", "progress_buf", "reset_buf"):
                np.testing.assert_array_equal(outs[0][f], outs[1][f], err_msg=f)
            lv0, lv1 = tr["terrain_levels"], outs[0]["terrain_levels"]
            st = lambda i: flagged & (state == i)  # noqa: E731
            np.testing.assert_array_equal(lv1[~flagged], lv0[~flagged])
            assert (lv1[st(0) | st(6)] == lv0[st(0) | st(6)] - 1).all() and (lv1[st(1)] == 0).all() and (lv0[st(1)] == 0).all()
            assert (lv0[st(3)] == tr["env_rows"] - 1).all()
            assert (lv1[st(5)] == lv0[st(5)] - 1).all()
            if batch_norm == 0.4:  # threshold 2 m: up, wrap, neither
                assert (lv1[st(2)] == lv0[st(2)] + 1).all() and (lv1[st(3)] == 0).all()
                assert (lv1[st(4)] == lv0[st(4)]).all()
            else:  # threshold 10 m: down and up cancel, 3 m is down
                assert (lv1[st(2)] == lv0[st(2)]).all() and (lv1[st(3)] == lv0[st(3)]).all()
                assert (lv1[st(4)] == lv0[st(4)] - 1).all()
            off = O.reset_flagged(p, b, m, d, terrain=dict(tr, update_levels=0, **extra))
            np.testing.assert_array_equal(off["terrain_levels"], lv0)
            # the per-env reading of the command norm is a different function wherever more than 4 envs reset
            per = O.reset_flagged(p, b, m, d, terrain=dict(tr, **extra), per_env_norm=True)
            if k >= 7:
                assert (per["terrain_levels"] != lv1).any()
    m = cases["all"]
    outs = [O.reset_flagged(p, b, m, *H.reset_draws(N, 12)[:1])]
    # the small-command gate is taken both ways and the Hound arm clamp binds at both limits
    c = outs[0]["commands"]
    if N >= 4:
        assert (c[:, :2] == 0).all(1).any() and (c[:, :2] != 0).all(1).any()
    hp, hb_, _ = H.tail_inputs(N, 12, seed=N, hound=True)
    hd = H.tail_hound(N)
    dh, eh = H.reset_draws(N, 12, hound=True)
    hh = dict(hd, pos_control=np.zeros((N, 6), F32), effort_control=np.ones((N, 6), F32), **eh)
    q = O.reset_flagged(hp, hb_, m, dh, hound=hh)["dof_state"][:, 12:, 0]
    if N >= 3:
        assert (q == np.asarray(hd["arm_lower"], F32)).all(1).any() and (q == np.asarray(hd["arm_upper"], F32)).all(1).any()
        assert ((q > np.asarray(hd["arm_lower"], F32)) & (q < np.asarray(hd["arm_upper"], F32))).any()


@pytest.mark.parametrize("N,npts", H.HEIGHTS_SHAPES)
def test_heights_inputs_hold_what_they_claim(N, npts):
    samples, border, hs, vs, root, pts, kindp = H.heights_inputs(N, npts)
    rows, cols = samples.shape
    assert samples.dtype == np.int16 and len(np.unique(samples)) == samples.size
    ix, iy, h, cells = O.measure_heights(samples, border, hs, vs, root, pts)
    ix32, iy32, _, _ = O.measure_heights(samples, border, hs, vs, root, pts, dtype=F32)
    near = np.abs(cells - np.round(cells)).min(-1) < H.HEIGHTS_NEAR
    print(f"[task heights] N {N} points {npts}: share of probes within {H.HEIGHTS_NEAR} cells of an integer "
          f"{near.mean():.4%}")
    assert near.mean() <= 0.01
    assert (ix32[~near] == ix[~near]).all() and (iy32[~near] == iy[~near]).all()
    cx, cy = cells[..., 0], cells[..., 1]
    tol = 1e-3  # the generator aims in float64 and stores float32
    assert ((cx[kindp == 2] > -3 - tol) & (cx[kindp == 2] < tol)).all()
    assert ((cx[kindp == 3] > rows - tol) & (cx[kindp == 3] < rows + 3 + tol)).all()
    assert ((cy[kindp == 4] > -3 - tol) & (cy[kindp == 4] < tol)).all()
    assert ((cy[kindp == 5] > cols - tol) & (cy[kindp == 5] < cols + 3 + tol)).all()
    strip = kindp == 6
    assert ((cx[strip] > -1) & (cx[strip] < 0) & (cy[strip] > -1) & (cy[strip] < 0)).all()
    assert (ix[strip] == 0).all() and (iy[strip] == 0).all()
    if N * npts >= 7:
        assert (ix[kindp == 3] == rows - 2).all() and (iy[kindp == 5] == cols - 2).all()
        assert (ix[kindp == 2] == 0).all() and (iy[kindp == 4] == 0).all()
        inside = kindp < 2
        assert ((cx[inside] > 0) & (cx[inside] < rows) & (cy[inside] > 0) & (cy[inside] < cols)).all()
        # world coordinates below 0 (before the border shift) occur and are plain interior cells
        assert ((cx * hs - border < 0) & (cx > 1)).any()
    assert (np.abs(root[1::2, 3]) > 0).all() and (root[0::2, 3] == 0).all()


# ------------------------------------------------------------------------------------------- the comparison rule
FLOAT_FIELDS = ("base_lin_vel", "base_ang_vel", "projected_gravity", "commands2", "feet_air_time", "rew_buf",
                "episode_sums")


def _rule(got, o64, o32, what):
    seen, fails = {}, []
    for f in FLOAT_FIELDS:
        H.field_check("task oracle", seen, fails, what, f, got[f], o64[f], o32[f])
    return fails


def test_rule_passes_the_float32_oracle_and_refuses_wrong_oracles():
    """field_check, the rule of tests/test_task_kernels_gpu.py, with a wrong float32 oracle in the kernel's place."""
    N = 130
    p, b, _ = H.tail_inputs(N, 12, seed=N)
    o64, o32 = O.post_a(p, b), O.post_a(p, b, dtype=F32)
    assert _rule(o32, o64, o32, "float32 oracle") == []
    o32n = O.post_a(p, b, dtype=F32)
    nb = {f: o32[f] for f in ("base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "progress_buf", "reset_buf")}
    pb64, pb32 = O.post_b(p, dict(b, **nb)), O.post_b(p, dict(b, **nb), dtype=F32)
    seen, fails = {}, []
    H.field_check("task oracle", seen, fails, "float32 oracle", "obs_buf", pb32["obs_buf"], pb64["obs_buf"], pb32["obs_buf"])
    assert fails == [] and o32n["rew_buf"].tobytes() == o32["rew_buf"].tobytes()
    for variant, fields in (("floored_wrap", {"commands2", "rew_buf", "episode_sums"}),
                            ("knee_ge", {"rew_buf", "episode_sums"}),
                            ("first_after_update", {"rew_buf", "episode_sums"}),
                            ("clip_after_termination", {"rew_buf"})):
        wrong = O.post_a(p, b, dtype=F32, variant=variant)
        fails = _rule(wrong, o64, o32, variant)
        hit = {f.split()[1].rstrip(":") for f in fails}
        assert hit == fields, (variant, fails)
    # the discrete outputs tell too: >= at the knee threshold resets the norm-1.0 envs
    assert (O.post_a(p, b, dtype=F32, variant="knee_ge")["reset_buf"] != o32["reset_buf"]).any()
    # an FMA-contracted quat_rotate_inverse in float32 moves results by an f32 rounding: it stays inside the bar,
    # which only says the bar is not that fine (bit-exactness against the other kernel forms is what pins it)
    fma = O.post_a(p, b, dtype=F32, variant="fma_rotate")
    assert (fma["base_lin_vel"] != o32["base_lin_vel"]).any()
    print("[task oracle] FMA-contracted quat_rotate_inverse:", _rule(fma, o64, o32, "fma_rotate") or "inside the bar")
