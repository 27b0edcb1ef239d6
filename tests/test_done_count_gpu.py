"""The done-count protocol and the flagged rank (isaacgymenv_amd/csrc/gt_wave.h) in the Ant and the flat-ground
kernels, at the C ABI on hand-built buffers with no sim: gt_ant_post_physics / gt_flat_post_physics record the per-wave
ballots, publish {count, seq} and re-arm the accumulator; gt_ant_reset_flagged / gt_flat_reset_flagged rank the
flagged envs in torch.nonzero order.  N = 1, 63, 65, 130 (one lane, a partial wave, two waves, three) and 4161 (66
waves: the second pass of the rank's prefix loop), every pattern of tests/helpers.py reset_masks_cases.  Every
comparison is exact: masks, counts and ids are integers, and the reset rows are the reference's torch_rand_float
expressions evaluated in numpy float32 one operation at a time on the uniforms gt_torch_rand gives for the same plans
(tests/test_philox_gpu.py pins that stream to torch).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
SIZES = (1, 63, 65, 130, 4161)
MAX_LEN = 50   # max_episode_length of both tasks here
SENTINEL = -77.0
BOUNDS = ((0.5, 1.5), (-0.1, 0.1), (-2.0, 2.0), (-1.0, 1.0), (-3.14, 3.14))  # flat: pos, vel, command x, y, yaw


def _gt():
    from isaacgymenv_amd import gymtask
    return gymtask


def _ok(rc, what):
    assert rc == 0, f"{what}: {_gt().lib().gt_last_error().decode()}"


def _t(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def _bits(words, N):
    w = np.asarray(words, dtype=np.uint64)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:N].astype(bool)


@pytest.fixture(scope="module")
def host_word():
    L = _gt().lib()
    h, d = C.c_void_p(), C.c_void_p()
    _ok(L.gt_host_alloc(8, C.byref(h), C.byref(d)), "gt_host_alloc")
    yield (C.c_int32 * 2).from_address(h.value), d.value
    _ok(L.gt_host_free(h), "gt_host_free")


def _identity_roots(N, z):
    root = np.zeros((N, 13), F32)
    root[:, 2], root[:, 6] = z, 1.0
    return root


def _task(task, N, host_dev):
    """(params, buffers struct, {name: device tensor}, post-physics entry point, reset entry point) with benign
    inputs: identity quaternions, zero contact forces, Ant's root above its termination height, lower < upper."""
    g = _gt()
    e = np.arange(N)
    if task == "ant":
        nd = 8
        p = g.GtAntParams()
        p.num_envs, p.num_dofs, p.dt = N, nd, 1.0 / 60.0
        p.dof_vel_scale, p.contact_force_scale, p.heading_weight, p.up_weight = 0.2, 0.1, 0.5, 0.1
        p.actions_cost_scale, p.energy_cost_scale, p.joints_at_limit_cost_scale = 0.005, 0.05, 0.1
        p.termination_height, p.death_cost, p.max_episode_length = 0.31, -2.0, float(MAX_LEN)
        p.dof_lower[:] = [-1.0 + 0.05 * j for j in range(nd)]
        p.dof_upper[:] = [1.0 - 0.05 * j for j in range(nd)]
        quat = np.tile(np.array([0, 0, 0, 1], F32), (N, 1))
        s = (e % 7 + 1).astype(F32)  # target - initial root = (3 s, 4 s): the planar norm 5 s is exact
        init_root = _identity_roots(N, 0.55)
        targets = np.stack([init_root[:, 0] + 3 * s, init_root[:, 1] + 4 * s, np.zeros(N, F32)], 1).astype(F32)
        arrays = dict(root_states=_identity_roots(N, 0.55), dof_state=np.zeros((N, nd, 2), F32),
                      sensors=np.zeros((N, 24), F32), actions=np.zeros((N, nd), F32), targets=targets,
                      inv_start_rot=quat, potentials=np.zeros(N, F32), prev_potentials=np.zeros(N, F32),
                      up_vec=np.zeros((N, 3), F32), heading_vec=np.zeros((N, 3), F32), obs_buf=np.zeros((N, 60), F32),
                      rew_buf=np.zeros(N, F32), true_objective=np.zeros(N, F32))
        B, post, reset = g.GtAntBuffers(), g.lib().gt_ant_post_physics, g.lib().gt_ant_reset_flagged
        # the reset's own inputs: initial positions on both sides of the limits, so the clamp takes all three branches
        extra = dict(initial_dof_pos=(1.15 * np.sin(0.7 * e[:, None] + 1.3 * np.arange(nd)[None])).astype(F32),
                     initial_root_states=init_root)
    else:
        nd, nb = 12, 5
        p = g.GtFlatParams()
        p.num_envs, p.num_dofs, p.num_bodies, p.base_index, p.num_knees = N, nd, nb, 0, 1
        p.knee_idx[0] = 2
        p.max_episode_length = MAX_LEN
        p.lin_vel_scale, p.ang_vel_scale, p.dof_pos_scale, p.dof_vel_scale = 2.0, 0.25, 1.0, 0.05
        p.rew_lin_vel_xy, p.rew_ang_vel_z, p.rew_torque = 1.0, 0.5, -0.000025
        gravity = np.tile(np.array([0, 0, -1], F32), (N, 1))
        default = (0.4 * np.cos(0.3 * e[:, None] + 0.9 * np.arange(nd)[None]) + 0.1).astype(F32)
        arrays = dict(root_states=_identity_roots(N, 0.62), dof_state=np.zeros((N, nd, 2), F32),
                      contact_forces=np.zeros((N, nb, 3), F32), torques=np.zeros((N, nd), F32),
                      actions=np.zeros((N, nd), F32), commands=np.zeros((N, 3), F32), default_dof_pos=default,
                      gravity_vec=gravity, obs_buf=np.zeros((N, 48), F32), rew_buf=np.zeros(N, F32))
        B, post, reset = g.GtFlatBuffers(), g.lib().gt_flat_post_physics, g.lib().gt_flat_reset_flagged
        extra = {}
    arrays.update(extra, reset_buf=np.zeros(N, np.int64), progress_buf=np.zeros(N, np.int64),
                  reset_count=np.zeros(3, np.int32), reset_masks=np.zeros((N + 63) // 64, np.int64),
                  env_ids=np.zeros(N, np.int32))
    ten = {k: _t(v) for k, v in arrays.items()}
    for name, _ in B._fields_:
        if name in ten:
            setattr(B, name, ten[name].data_ptr())
    B.host_count = host_dev
    return p, B, ten, post, reset


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("task", ["ant", "flat"])
def test_post_physics_records_and_counts_the_done_mask(task, N, host_word):
    """One launch per pattern on the same buffers, each under its own seq: the done mask forced through progress_buf,
    its ballots, the device and host counts, the seq, and the accumulator re-armed for the next launch."""
    words, host_dev = host_word
    p, B, ten, post, _ = _task(task, N, host_dev)
    for i, (name, masks) in enumerate(H.reset_masks_cases(N).items()):
        what = f"{task} N={N} {name}"
        flagged = _bits(masks, N)
        seq = 1000 * N + 17 * i + 3
        ten["progress_buf"].copy_(_t(np.where(flagged, MAX_LEN - 1, 0).astype(np.int64)))
        ten["reset_buf"].zero_()  # (Ant keeps a reset_buf that is already set)
        B.seq = seq
        _ok(post(C.byref(p), C.byref(B), None), what)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ten["reset_buf"].cpu().numpy(), flagged.astype(np.int64), err_msg=what)
        np.testing.assert_array_equal(ten["reset_masks"].cpu().numpy().view(np.uint64), masks, err_msg=what)
        k = H.popcount(masks)
        assert k == int(flagged.sum())
        assert ten["reset_count"].tolist() == [0, 0, k], what
        assert (words[0], words[1]) == (k, seq), what


def _plans(sizes):
    if not any(sizes):  # k = 0: nothing is drawn (and nothing planned: torch.rand(0) launches no kernel)
        return [_gt().GtTorchRandPlan(4242, 0, 256, 0) for _ in sizes]
    torch.manual_seed(4242)
    return _gt().TorchRandPlanner(DEV).plan_many(sizes)


def _uniforms(plan, shape):
    out = torch.full((max(int(np.prod(shape)), 1),), 9.0, dtype=torch.float32, device=DEV)
    _ok(_gt().lib().gt_torch_rand(C.byref(plan), out.data_ptr(), None), "gt_torch_rand")
    return out.cpu().numpy()[:int(np.prod(shape))].reshape(shape)


def _affine(lo, hi, u):
    """torch_rand_float: (upper - lower) * rand + lower, the range a Python double cast to the struct's float"""
    return F32(hi - lo) * u + F32(lo)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("task", ["ant", "flat"])
def test_reset_flagged_ranks_in_nonzero_order(task, N, host_word):
    """Given a pattern as reset_masks and k = its popcount: env_ids_out[:k] = flatnonzero, unflagged rows keep their
    sentinel, flagged rows are the reference's expression in float32 on draw row t = the env's rank; k = 0 launches
    nothing."""
    g = _gt()
    p, B, ten, _, reset = _task(task, N, host_word[1])
    nd = p.num_dofs
    for name, masks in H.reset_masks_cases(N).items():
        what = f"{task} N={N} {name}"
        flagged = _bits(masks, N)
        ids = np.flatnonzero(flagged)
        k = len(ids)
        assert k == H.popcount(masks)
        ten["reset_masks"].copy_(_t(masks.view(np.int64)))
        ten["env_ids"].fill_(-1)
        ten["progress_buf"].fill_(5)
        ten["reset_buf"].fill_(5)
        ten["dof_state"].fill_(SENTINEL)
        exp_dof = np.full((N, nd, 2), SENTINEL, F32)
        if task == "ant":
            r = g.GtAntResetArgs()
            r.plan_pos, r.plan_vel = plans = _plans((k * nd, k * nd))
            r.pos_range, r.pos_lower, r.vel_range, r.vel_lower = 0.2 - (-0.2), -0.2, 0.1 - (-0.1), -0.1
            r.initial_dof_pos, r.initial_root_states = ten["initial_dof_pos"].data_ptr(), \
                ten["initial_root_states"].data_ptr()
            for f in ("potentials", "prev_potentials"):
                ten[f].fill_(SENTINEL)
        else:
            r = g.GtFlatResetArgs()
            plans = _plans((k * nd, k * nd, k, k, k))
            for i, (lo, hi) in enumerate(BOUNDS):
                r.plan[i], r.range[i], r.lower[i] = plans[i], hi - lo, lo
            r.commands = ten["commands"].data_ptr()
            ten["commands"].fill_(SENTINEL)
        r.dof_state, r.progress_buf, r.env_ids_out = (ten[f].data_ptr() for f in ("dof_state", "progress_buf",
                                                                                   "env_ids"))
        _ok(reset(C.byref(p), C.byref(B), k, C.byref(r), None), what)
        torch.cuda.synchronize()
        got_ids = ten["env_ids"].cpu().numpy()
        np.testing.assert_array_equal(got_ids[:k], ids, err_msg=what)
        assert (got_ids[k:] == -1).all(), what
        np.testing.assert_array_equal(ten["progress_buf"].cpu().numpy(), np.where(flagged, 0, 5), err_msg=what)
        if k:
            u_pos, u_vel = _uniforms(plans[0], (k, nd)), _uniforms(plans[1], (k, nd))
        if task == "ant":
            np.testing.assert_array_equal(ten["reset_buf"].cpu().numpy(), np.where(flagged, 0, 5), err_msg=what)
            exp_pot = np.full(N, SENTINEL, F32)
            if k:
                lower, upper = np.array(p.dof_lower[:], F32), np.array(p.dof_upper[:], F32)
                x = ten["initial_dof_pos"].cpu().numpy()[ids] + _affine(-0.2, 0.2, u_pos)
                exp_dof[ids, :, 0] = np.maximum(np.minimum(x, upper), lower)  # tensor_clamp
                exp_dof[ids, :, 1] = _affine(-0.1, 0.1, u_vel)
                assert k < 8 or ((x > upper).any() and (x < lower).any()), "the clamp's branches are not all taken"
                d = (ten["targets"].cpu().numpy() - ten["initial_root_states"].cpu().numpy()[:, :3])[ids]
                exp_pot[ids] = -np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + F32(0)) * (F32(1) / F32(p.dt))
            for f in ("potentials", "prev_potentials"):
                np.testing.assert_array_equal(ten[f].cpu().numpy(), exp_pot, err_msg=f"{what} {f}")
        else:
            np.testing.assert_array_equal(ten["reset_buf"].cpu().numpy(), np.where(flagged, 1, 5), err_msg=what)
            exp_cmd = np.full((N, 3), SENTINEL, F32)
            if k:
                default = ten["default_dof_pos"].cpu().numpy()[ids]
                exp_dof[ids, :, 0] = default * _affine(*BOUNDS[0], u_pos)
                exp_dof[ids, :, 1] = _affine(*BOUNDS[1], u_vel)
                for c in range(3):
                    exp_cmd[ids, c] = _affine(*BOUNDS[2 + c], _uniforms(plans[2 + c], (k,)))
            np.testing.assert_array_equal(ten["commands"].cpu().numpy(), exp_cmd, err_msg=f"{what} commands")
        np.testing.assert_array_equal(ten["dof_state"].cpu().numpy(), exp_dof, err_msg=f"{what} dof_state")
