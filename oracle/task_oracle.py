"""AnymalTerrain / UsefulHound tail oracle -- TEST INFRASTRUCTURE ONLY (imported by tests/ alone).

Plain numpy restatements of the statements include/gymtask.h makes for gt_anymal_post_physics_a / _b,
gt_anymal_reset_flagged, gt_anymal_reset and gt_measure_heights, and of the lines of
isaacgymenv_amd/isaacgymenvs/tasks/anymal_terrain.py / useful_hound.py they cite.  Every function takes ``dtype``:
np.float64 (the default) is the truth, np.float32 the same statements in the same order in float32 (the yardstick),
and the pair measures what f32 rounding alone does to each output.  Inputs are the f32 values the kernel receives
(parameters included: they are rounded to f32 first, as the C struct holds them), widened to ``dtype``; integers,
masks and ids are exact in both.  Sums over dofs, feet and envs are added one term at a time in ascending order.

params: a dict with the fields of gt_anymal_params (lists for the arrays).  hound: None, or a dict with the fields of
gt_anymal_hound the statements read (num_actions, num_shoulders, shoulder_idx, arm_default, arm_lower, arm_upper,
arm_noise2) plus eef [N][7] (end-effector position | quaternion) and arm_commands [N][3].  bufs: a dict of numpy
arrays named as gt_anymal_buffers, shaped [N][...] (contact_forces [N][nb][3], dof_state [N][na][2], episode_sums
[13][N]); nothing passed in is modified.
"""
from __future__ import annotations

import numpy as np

NUM_TERMS = 13
TERMS = ("lin_vel_xy", "lin_vel_z", "ang_vel_z", "ang_vel_xy", "orient", "torques", "joint_acc", "base_height",
         "air_time", "collision", "stumble", "action_rate", "hip")
HIP_DOFS = (0, 3, 6, 9)  # anymal_terrain.py: dof_pos[:, [0, 3, 6, 9]]
# deliberately wrong variants of post_a (tests/test_task_oracle.py: the comparison rule must refuse them)
VARIANTS = (None, "floored_wrap", "knee_ge", "fma_rotate", "first_after_update", "clip_after_termination")


def _f(x, dt):
    """Kernel-side f32 values (arrays or parameters) widened to dt."""
    return np.asarray(np.asarray(x, dtype=np.float32), dtype=dt)


def _fma(a, b, c, dt):
    """a * b + c rounded once (exact in float64 for f32 operands up to the final rounding)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(dt)


def quat_rotate_inverse(q, v, dt, fma=False):
    """torch_jit_utils.quat_rotate_inverse: a - b + c with a = v (2 w^2 - 1), b = 2 w (u x v), c = 2 u (u . v)."""
    w = q[:, 3]
    two, one = dt(2.0), dt(1.0)
    if fma:  # what a contracting compiler would make of the same statements
        s = _fma(two, w * w, -one, dt)
        cx = _fma(q[:, 1], v[:, 2], -(q[:, 2] * v[:, 1]), dt)
        cy = _fma(q[:, 2], v[:, 0], -(q[:, 0] * v[:, 2]), dt)
        cz = _fma(q[:, 0], v[:, 1], -(q[:, 1] * v[:, 0]), dt)
        d = _fma(q[:, 2], v[:, 2], _fma(q[:, 1], v[:, 1], q[:, 0] * v[:, 0], dt), dt)
        c = (cx, cy, cz)
        return np.stack([_fma(q[:, i] * d, two, _fma(v[:, i], s, -((c[i] * w) * two), dt), dt) for i in range(3)], 1)
    s = two * (w * w) - one
    cx = q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1]
    cy = q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2]
    cz = q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0]
    d = q[:, 0] * v[:, 0] + q[:, 1] * v[:, 1] + q[:, 2] * v[:, 2]
    c = (cx, cy, cz)
    return np.stack([(v[:, i] * s - (c[i] * w) * two) + (q[:, i] * d) * two for i in range(3)], 1)


def _norm3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _seq_sum(x, dt):
    """Sum over the last axis, one term at a time in ascending order."""
    s = np.zeros(x.shape[:-1], dtype=dt)
    for j in range(x.shape[-1]):
        s = s + x[..., j]
    return s


def masks_of(flags):
    """Per-wave 64-bit ballots of a bool [N]: bit l of word w = env 64 w + l."""
    flags = np.asarray(flags, dtype=bool)
    n = flags.shape[0]
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    for e in np.nonzero(flags)[0]:
        words[e >> 6] |= np.uint64(1) << np.uint64(e & 63)
    return words


def ids_of(masks, n):
    """The flagged env ids ascending (torch.nonzero's order)."""
    masks = np.asarray(masks).view(np.uint64)
    return np.asarray([e for e in range(n) if (int(masks[e >> 6]) >> (e & 63)) & 1], dtype=np.int32)


def post_a(params, bufs, hound=None, dtype=np.float64, variant=None):
    """gt_anymal_post_physics_a (anymal_terrain.py post_physics_step up to compute_reward, minus the push;
    useful_hound.py's differences with `hound`).  Returns every stored field, the masks and count, and the decisions."""
    assert variant in VARIANTS
    dt = dtype
    p = params
    N, nd = int(p["num_envs"]), int(p["num_dofs"])
    na = int(hound["num_actions"]) if hound else nd
    nf, nk = int(p["num_feet"]), int(p["num_knees"])
    root = _f(bufs["root_states"], dt)
    cf = _f(bufs["contact_forces"], dt).reshape(N, -1, 3)
    dof = _f(bufs["dof_state"], dt).reshape(N, na, 2)
    tq, act, lact = (_f(bufs[k], dt).reshape(N, na) for k in ("torques", "actions", "last_actions"))
    lqd = _f(bufs["last_dof_vel"], dt).reshape(N, nd)
    cmd = _f(bufs["commands"], dt).copy()
    air = _f(bufs["feet_air_time"], dt).copy()
    sums = _f(bufs["episode_sums"], dt).reshape(NUM_TERMS, N)
    S = {k: dt(np.float32(v)) for k, v in p.items() if k.startswith("s_")}
    pdt = dt(np.float32(p["dt"]))
    default = _f(p["default_dof_pos"], dt)
    out = {}
    prog = np.asarray(bufs["progress_buf"], dtype=np.int64) + 1
    out["progress_buf"] = prog
    out["randomize_buf"] = np.asarray(bufs["randomize_buf"], dtype=np.int64) + 1
    tb = np.asarray(bufs["timeout_buf"])
    if tb.dtype == np.int64:  # VecTask's initial zeros: ~int64 is -1 - x, not a logical not
        not_timeout = (~tb).astype(dt)
    else:
        not_timeout = np.where(tb != 0, dt(0.0), dt(1.0))

    # base-frame quantities and the heading command
    q = root[:, 3:7]
    fma = variant == "fma_rotate"
    blv = quat_rotate_inverse(q, root[:, 7:10], dt, fma)
    bav = quat_rotate_inverse(q, root[:, 10:13], dt, fma)
    gv = np.tile(np.asarray([0.0, 0.0, -1.0], dtype=dt), (N, 1))
    pg = quat_rotate_inverse(q, gv, dt, fma)
    z, one, two = dt(0.0), dt(1.0), dt(2.0)
    tx = (q[:, 1] * z - q[:, 2] * z) * two  # quat_apply(q, (1, 0, 0)): t = 2 u x f; f + w t + u x t
    ty = (q[:, 2] * one - q[:, 0] * z) * two
    tz = (q[:, 0] * z - q[:, 1] * one) * two
    fx = (one + q[:, 3] * tx) + (q[:, 1] * tz - q[:, 2] * ty)
    fy = (z + q[:, 3] * ty) + (q[:, 2] * tx - q[:, 0] * tz)
    heading = np.arctan2(fy, fx)
    two_pi, pi = dt(2 * np.pi), dt(np.pi)
    diff = cmd[:, 3] - heading
    ang = np.mod(diff, two_pi) if variant == "floored_wrap" else np.fmod(diff, two_pi)  # TorchScript %: C fmod
    wrap_high = ang > pi
    ang = ang - two_pi * np.where(wrap_high, one, z)
    half = dt(0.5) * ang
    c2 = np.minimum(np.maximum(half, -one), one)
    out["wrap_side"] = np.where(wrap_high, 1, np.where(diff < -pi, -1, 0))  # which side of +-pi cmd - heading lay on
    out["c2_clamp"] = np.where(half > one, 1, np.where(half < -one, -1, 0))

    # check_termination
    thr = (lambda x: x >= one) if variant == "knee_ge" else (lambda x: x > one)
    reset = _norm3(cf[:, int(p["base_index"])]) > one
    knee = np.stack([thr(_norm3(cf[:, int(p["knee_idx"][k])])) for k in range(nk)], 1) if nk else np.zeros((N, 0), bool)
    knee_count = knee.sum(1).astype(np.int64)
    sh_count = np.zeros(N, dtype=np.int64)
    if hound:
        for k in range(int(hound["num_shoulders"])):
            sh_count += (_norm3(cf[:, int(hound["shoulder_idx"][k])]) > one).astype(np.int64)
        reset = reset | (knee_count > 0) | (sh_count > 0)
    elif not p["allow_knee_contacts"]:
        reset = reset | (knee_count > 0)
    reset = reset | (prog >= int(p["max_episode_length"]) - 1)

    # compute_reward, the reference's order
    sq = lambda x: x * x  # noqa: E731
    lin_err = sq(cmd[:, 0] - blv[:, 0]) + sq(cmd[:, 1] - blv[:, 1])
    ang_err = sq(c2 - bav[:, 2])
    r = {}
    r["lin_vel_xy"] = np.exp(-lin_err / dt(0.25)) * S["s_lin_vel_xy"]
    r["ang_vel_z"] = np.exp(-ang_err / dt(0.25)) * S["s_ang_vel_z"]
    r["lin_vel_z"] = sq(blv[:, 2]) * S["s_lin_vel_z"]
    r["ang_vel_xy"] = (sq(bav[:, 0]) + sq(bav[:, 1])) * S["s_ang_vel_xy"]
    r["orient"] = (sq(pg[:, 0]) + sq(pg[:, 1])) * S["s_orient"]
    r["base_height"] = sq(root[:, 2] - dt(0.52)) * S["s_base_height"]
    r["torques"] = _seq_sum(sq(tq), dt) * S["s_torque"]
    r["joint_acc"] = _seq_sum(sq(lqd - dof[:, :nd, 1]), dt) * S["s_joint_acc"]
    kc = knee_count.astype(dt) * S["s_collision"]
    r["collision"] = kc + sh_count.astype(dt) * S["s_collision"] if hound else kc
    stumble = np.zeros(N, dtype=np.int64)
    air_sum = np.zeros(N, dtype=dt)
    contacts, firsts = np.zeros((N, 4), bool), np.zeros((N, 4), bool)
    for k in range(nf):
        f = cf[:, int(p["feet_idx"][k])]
        stumble += ((np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) > dt(5.0)) & (np.abs(f[:, 2]) < one)).astype(np.int64)
        contact = f[:, 2] > one
        a = air[:, k] + pdt
        first = ((a if variant == "first_after_update" else air[:, k]) > z) & contact
        air_sum = air_sum + (a - dt(0.5)) * np.where(first, one, z)
        air[:, k] = a * np.where(contact, z, one)
        contacts[:, k], firsts[:, k] = contact, first
    r["stumble"] = stumble.astype(dt) * S["s_stumble"]
    r["action_rate"] = _seq_sum(sq(lact - act), dt) * S["s_action_rate"]
    cmd_gate = np.sqrt(cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) > dt(0.1)
    r["air_time"] = (air_sum * S["s_air_time"]) * np.where(cmd_gate, one, z)
    hip = np.zeros(N, dtype=dt)
    for j in HIP_DOFS:
        hip = hip + np.abs(dof[:, j, 0] - default[j])
    r["hip"] = hip * S["s_hip"]
    rew = r["lin_vel_xy"] + r["ang_vel_z"] + r["lin_vel_z"] + r["ang_vel_xy"] + r["orient"] + r["base_height"] + \
        r["torques"] + r["joint_acc"] + r["collision"] + r["action_rate"] + r["air_time"] + r["hip"] + r["stumble"]
    term = S["s_termination"] * (np.where(reset, one, z) * not_timeout)
    out["rew_preclip"] = rew
    out["rew_clipped"] = rew < z
    if variant == "clip_after_termination":
        rew = np.maximum(rew + term, z)
    else:
        rew = np.maximum(rew, z) + term
    cmd[:, 2] = c2
    out.update(base_lin_vel=blv, base_ang_vel=bav, projected_gravity=pg, commands=cmd, commands2=c2,
               feet_air_time=air, reset_buf=reset.astype(np.uint8), rew_buf=rew,
               episode_sums=np.stack([sums[t] + r[name] for t, name in enumerate(TERMS)]), terms=r,
               reset_masks=masks_of(reset), count=int(reset.sum()), knee_count=knee_count, sh_count=sh_count,
               stumble=stumble, first=firsts, contact=contacts, cmd_gate=cmd_gate, heading=heading)
    return out


def post_b(params, bufs, noise=None, hound=None, dtype=np.float64):
    """gt_anymal_post_physics_b (compute_observations, the noise, last_actions / last_dof_vel, VecTask's time_outs and
    clamped copy).  bufs additionally holds post_a's base_lin_vel / base_ang_vel / projected_gravity, noise_scale,
    clip_obs, and measured_heights [N][140] or None (plane).  noise: uniform draws [N][num_obs] or None."""
    dt = dtype
    p = params
    N, nd, no = int(p["num_envs"]), int(p["num_dofs"]), int(p["num_obs"])
    na = int(hound["num_actions"]) if hound else nd
    nh = no - 12 - 2 * nd - na - (10 if hound else 0)
    root = _f(bufs["root_states"], dt)
    dof = _f(bufs["dof_state"], dt).reshape(N, na, 2)
    act = _f(bufs["actions"], dt).reshape(N, na)
    cmd = _f(bufs["commands"], dt)
    lin, angs = dt(np.float32(p["lin_vel_scale"])), dt(np.float32(p["ang_vel_scale"]))
    mh = bufs.get("measured_heights")
    mh = np.zeros((N, nh), dtype=dt) if mh is None else _f(mh, dt).reshape(N, nh)
    one = dt(1.0)
    heights = np.minimum(np.maximum(root[:, 2:3] - dt(0.5) - mh, -one), one) * dt(np.float32(p["height_meas_scale"]))
    cscale = np.asarray([lin, lin, angs], dtype=dt)
    parts = [_f(bufs["base_lin_vel"], dt) * lin, _f(bufs["base_ang_vel"], dt) * angs, _f(bufs["projected_gravity"], dt),
             cmd[:, :3] * cscale, dof[:, :nd, 0] * dt(np.float32(p["dof_pos_scale"])),
             dof[:, :nd, 1] * dt(np.float32(p["dof_vel_scale"])), heights, act]
    if hound:
        parts += [_f(hound["eef"], dt).reshape(N, 7), _f(hound["arm_commands"], dt).reshape(N, 3)]
    obs = np.concatenate(parts, axis=1)
    assert obs.shape == (N, no)
    if noise is not None:
        obs = obs + (dt(2.0) * _f(noise, dt).reshape(N, no) - one) * _f(bufs["noise_scale"], dt)
    clip = dt(np.float32(bufs.get("clip_obs", np.inf)))
    prog = np.asarray(bufs["progress_buf"], dtype=np.int64)
    rst = np.asarray(bufs["reset_buf"])
    return dict(obs_buf=obs, obs_out=np.minimum(np.maximum(obs, -clip), clip),
                time_outs=((prog >= int(p["max_episode_length"]) - 1) & (rst != 0)).astype(np.uint8),
                last_actions=act.copy(), last_dof_vel=dof[:, :nd, 1].copy())


def _reset_common(p, b, e, off, vel, cx, cy, ch, nd, na, dt):
    """The statements reset_idx applies to env e (rows already mapped through torch_rand_float)."""
    default = _f(p["default_dof_pos"], dt)
    b["dof_state"][e, :nd, 0] = default[:nd] * off
    b["dof_state"][e, :nd, 1] = vel
    c = np.asarray([cx, cy, b["commands"][e, 2], ch], dtype=dt)
    gate = dt(1.0) if np.sqrt(c[0] * c[0] + c[1] * c[1]) > dt(0.25) else dt(0.0)
    b["commands"][e] = c * gate
    b["last_actions"][e] = 0
    b["last_dof_vel"][e] = 0
    b["feet_air_time"][e] = 0
    b["progress_buf"][e] = 0
    b["reset_buf"][e] = 1


def _reset_copies(params, bufs, hound, dt):
    N, nd = int(params["num_envs"]), int(params["num_dofs"])
    na = int(hound["num_actions"]) if hound else nd
    b = dict(dof_state=_f(bufs["dof_state"], dt).reshape(N, na, 2).copy(), root_states=_f(bufs["root_states"], dt).copy(),
             commands=_f(bufs["commands"], dt).copy(), last_actions=_f(bufs["last_actions"], dt).reshape(N, na).copy(),
             last_dof_vel=_f(bufs["last_dof_vel"], dt).reshape(N, nd).copy(),
             feet_air_time=_f(bufs["feet_air_time"], dt).copy(),
             progress_buf=np.asarray(bufs["progress_buf"], dtype=np.int64).copy(),
             reset_buf=np.asarray(bufs["reset_buf"], dtype=np.uint8).copy(),
             episode_sums=_f(bufs["episode_sums"], dt).reshape(NUM_TERMS, N).copy())
    return N, nd, na, b


def episode_sum(episode_sums, ids, dtype=np.float64):
    """Per term, the sum over `ids`, added one env at a time in the given order."""
    sums = _f(episode_sums, dtype).reshape(NUM_TERMS, -1)
    ep = np.zeros(NUM_TERMS, dtype=dtype)
    for e in ids:
        ep = ep + sums[:, e]
    return ep


def episode_out(episode_sums, ids, episode_length_s, dtype=np.float64):
    """extras["episode"]: per term, the mean over `ids` (added one env at a time, ascending) / episode_length_s."""
    ep = episode_sum(episode_sums, ids, dtype)
    return ep / dtype(len(ids)) / dtype(np.float32(episode_length_s)) if len(ids) else ep


def reset_flagged(params, bufs, masks, draws, terrain=None, hound=None, episode_length_s=20.0, dtype=np.float64,
                  per_env_norm=False):
    """gt_anymal_reset_flagged: reset_idx for the envs flagged in `masks`, row t of the draws to the t-th flagged env.
    draws: u_pos / u_vel [k][nd], u_cmd_x / u_cmd_y / u_cmd_h [k] uniforms and the *_range / *_lower of
    torch_rand_float's map range * u + lower.  terrain: None (plane) or a dict with the fields of
    gt_anymal_terrain_reset (u_root_xy [k][2]).  hound: additionally u_arm [k][6], pos_control / effort_control [N][6].
    per_env_norm: a deliberately wrong variant (each env's own command norm in update_terrain_level).
    Returns env_ids, every written buffer, and episode_out [13] (+ the terrain-level mean at [13] with terrain)."""
    dt = dtype
    N, nd, na, b = _reset_copies(params, bufs, hound, dt)
    ids = ids_of(masks, N)
    k = len(ids)
    f32 = lambda x: dt(np.float32(x))  # noqa: E731
    u = {n: _f(draws[n], dt).reshape(k, -1) for n in ("u_pos", "u_vel", "u_cmd_x", "u_cmd_y", "u_cmd_h")}
    base_init = _f(params["base_init_state"], dt)
    if terrain is not None:
        lv = np.asarray(terrain["terrain_levels"], dtype=np.int64).copy()
        ty = np.asarray(terrain["terrain_types"], dtype=np.int64)
        eo = _f(terrain["env_origins"], dt).copy()
        to = _f(terrain["terrain_origins"], dt)
        uxy = _f(terrain["u_root_xy"], dt).reshape(k, 2)
    if hound:
        pc, ec = _f(hound["pos_control"], dt).copy(), _f(hound["effort_control"], dt).copy()
        ua = _f(hound["u_arm"], dt).reshape(k, 6)
    ep = np.zeros(NUM_TERMS + (1 if terrain is not None else 0), dtype=dt)
    # torch.norm(self.commands[env_ids, :2]) has no dim: ONE number over every env reset in this step, taken before
    # any command is redrawn (per_env_norm: the per-env reading, a deliberately wrong variant)
    cn_all = dt(0.0)
    for e in ids:
        cn_all = cn_all + (b["commands"][e, 0] * b["commands"][e, 0] + b["commands"][e, 1] * b["commands"][e, 1])
    cn_all = np.sqrt(cn_all)
    for t, e in enumerate(ids):
        off = f32(draws["pos_range"]) * u["u_pos"][t] + f32(draws["pos_lower"])
        vel = f32(draws["vel_range"]) * u["u_vel"][t] + f32(draws["vel_lower"])
        if terrain is not None:
            # update_terrain_level on the state before the reset
            if terrain["update_levels"]:
                dx, dy = b["root_states"][e, 0] - eo[e, 0], b["root_states"][e, 1] - eo[e, 1]
                dist = np.sqrt(dx * dx + dy * dy)
                c0, c1 = b["commands"][e, 0], b["commands"][e, 1]
                cn = np.sqrt(c0 * c0 + c1 * c1) if per_env_norm else cn_all
                lvl = int(lv[e])
                lvl -= int(dist < cn * f32(terrain["max_episode_length_s"]) * dt(0.25))
                lvl += int(dist > f32(terrain["env_length"]) / dt(2.0))
                lv[e] = max(lvl, 0) % int(terrain["env_rows"])
                eo[e] = to[lv[e], ty[e]]
            r = base_init.copy()
            r[:3] = r[:3] + eo[e]
            r[0] = r[0] + (f32(terrain["xy_range"]) * uxy[t, 0] + f32(terrain["xy_lower"]))
            r[1] = r[1] + (f32(terrain["xy_range"]) * uxy[t, 1] + f32(terrain["xy_lower"]))
            b["root_states"][e] = r
        else:
            b["root_states"][e] = base_init
        cx = f32(draws["cmd_x_range"]) * u["u_cmd_x"][t, 0] + f32(draws["cmd_x_lower"])
        cy = f32(draws["cmd_y_range"]) * u["u_cmd_y"][t, 0] + f32(draws["cmd_y_lower"])
        ch = f32(draws["cmd_h_range"]) * u["u_cmd_h"][t, 0] + f32(draws["cmd_h_lower"])
        _reset_common(params, b, e, off, vel, cx, cy, ch, nd, na, dt)
        if hound:  # useful_hound.py: tensor_clamp(default + noise * 2.0 * (u - 0.5), lower, upper)
            x = _f(hound["arm_default"], dt) + (ua[t] - dt(0.5)) * f32(hound["arm_noise2"])
            qa = np.maximum(np.minimum(x, _f(hound["arm_upper"], dt)), _f(hound["arm_lower"], dt))
            b["dof_state"][e, nd:nd + 6, 0] = qa
            b["dof_state"][e, nd:nd + 6, 1] = 0
            pc[e], ec[e] = qa, 0
        b["episode_sums"][:, e] = 0
    ep[:NUM_TERMS] = episode_out(bufs["episode_sums"], ids, episode_length_s, dt)
    out = dict(b, env_ids=ids, episode_out=ep)
    if terrain is not None:
        ep[NUM_TERMS] = lv.astype(dt).sum() / dt(N)
        out.update(terrain_levels=lv, env_origins=eo)
    if hound:
        out.update(pos_control=pc, effort_control=ec)
    return out


def reset(params, bufs, env_ids, pos_offset, dof_vel, cmd_x, cmd_y, cmd_heading, dtype=np.float64):
    """gt_anymal_reset: reset_idx for explicit ids with the draws already mapped; ids outside [0, N) are skipped and
    not summed.  episode_out[13] = the per-term sums over the valid ids (the caller divides)."""
    dt = dtype
    N, nd, na, b = _reset_copies(params, bufs, None, dt)
    k = len(env_ids)
    off, vel = _f(pos_offset, dt).reshape(k, nd), _f(dof_vel, dt).reshape(k, nd)
    cx, cy, ch = (_f(x, dt).reshape(k) for x in (cmd_x, cmd_y, cmd_heading))
    ids = np.asarray(env_ids, dtype=np.int64)
    ep = episode_sum(bufs["episode_sums"], ids[(ids >= 0) & (ids < N)], dt)
    for t, e in enumerate(ids):
        if e < 0 or e >= N:
            continue
        b["root_states"][e] = _f(params["base_init_state"], dt)
        _reset_common(params, b, e, off[t], vel[t], cx[t], cy[t], ch[t], nd, na, dt)
        b["episode_sums"][:, e] = 0
    return dict(b, episode_out=ep)


def measure_heights(samples, border, hs, vs, root_states, points, dtype=np.float64):
    """gt_measure_heights (get_heights, trimesh terrain): p = quat_apply_yaw(q, point) + root + border,
    (ix, iy) = clip(trunc(p.xy / hs), 0, (rows - 2, cols - 2)), height = vs min(samples[ix][iy], samples[ix+1][iy+1]).
    Returns (ix, iy, heights, cells): cells [N][np][2] = p.xy / hs before truncation."""
    dt = dtype
    hf = np.asarray(samples)
    rows, cols = hf.shape
    root = _f(root_states, dt)
    N = root.shape[0]
    pts = _f(points, dt).reshape(N, -1, 3)
    qz, qw = root[:, 5], root[:, 6]
    nrm = np.maximum(np.sqrt(qz * qz + qw * qw), dt(1e-9))
    z, w = (qz / nrm)[:, None], (qw / nrm)[:, None]
    vx, vy = pts[:, :, 0], pts[:, :, 1]
    two = dt(2.0)
    tx, ty = (-(z * vy)) * two, (z * vx) * two  # t = 2 q x v with q = (0, 0, z)
    cx, cy = -(z * ty), z * tx                  # q x t
    px = vx + w * tx + cx + root[:, 0:1] + dt(np.float32(border))
    py = vy + w * ty + cy + root[:, 1:2] + dt(np.float32(border))
    cells = np.stack([px / dt(np.float32(hs)), py / dt(np.float32(hs))], axis=-1)
    ix = np.clip(np.trunc(cells[..., 0]).astype(np.int64), 0, rows - 2)
    iy = np.clip(np.trunc(cells[..., 1]).astype(np.int64), 0, cols - 2)
    h = np.minimum(hf[ix, iy], hf[ix + 1, iy + 1]).astype(dt) * dt(np.float32(vs))
    return ix, iy, h, cells
