"""gt_anymal_post_physics_a / _b / _ab, gt_anymal_reset_flagged, gt_anymal_reset and gt_measure_heights at the C ABI
(include/gymtask.h) against the float64 restatement of the same statements (oracle/task_oracle.py), on constructed
inputs (tests/helpers.py tail_inputs, reset_masks_cases, heights_inputs; what is claimed of them is asserted on the CPU
in tests/test_task_oracle.py).  No env object is involved: every call goes through gymtask.lib() with the ctypes
structs of isaacgymenv_amd/gymtask.py on buffers allocated here.

Every float field is judged by tests/helpers.py field_check,
    max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|,
ref32 being the same oracle in float32; copies, integers, masks, ids, counts and zeroed fields are compared exactly.
Every buffer lies inside a larger allocation filled with the byte 0xA5 (before it, where the buffer is offset, and
64 bytes after it) that must be intact after the call; const inputs must be unchanged; refusals are nonzero, name
their entry point and write nothing.  One-number outputs (episode_out) take err_f32 as the largest |ref32 - ref64|
over the episode sums of seeds 0..15 of the same shape.

MEASURED on an MI355X (124 cases, 5.3 s): the largest err_kernel / bar per field (<= 1 passes) -- commands[:, 2] 0.26,
rew_buf 0.22, terrain level mean 0.17, base_ang_vel 0.13, base_lin_vel 0.13, projected_gravity 0.12, reset dof_state
0.11, episode_sums 0.10, reset commands 0.10, episode_out 0.09, obs_buf 0.08, reset root_states 0.07, pos_control
0.07, feet_air_time 0.06, gt_anymal_reset's sums 0.05; every height probe on the float64 oracle's cell.  The kernels
agree with the float32 oracle to the bit in most fields (err_kernel / err_f32 = 1).

What the tests found: check_params accepted num_dofs 1..9 although post_a_env reads dofs 0, 3, 6, 9 for the hip term
unconditionally (registers nothing wrote); it now refuses fewer than 10.  k_reset_flagged took the terrain
curriculum's command norm per env, where the task's (the reference's) torch.norm(self.commands[env_ids, :2]) is one
number over every env reset in the step: with the parent's library all 8 test_reset_flagged_terrain cases with
update_levels = 1 and more than one env fail (the levels differ); k_flagged_cmd_norm now takes that norm before the
reset kernel.  Every float field was inside its bar.

Deliberate mutations, each built into a scratch copy of the library and run against this module (tests failed of
124): wrap_to_pi as a floored remainder 60; k_post_ab without the clearing of the trailing 16-bit slices 16 (every N
that is no multiple of 64); k_reset_flagged's rank base from the first 64 mask words only 4 and its final staging
loop stopping after one pass 4 (the N = 4161 cases of the plane and terrain tests: below 4097 envs neither loop runs
twice); first contact from the updated air time 76; the clip after the termination term 66.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import task_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, FILL = 64, 0xA5
F32, F64 = np.float32, np.float64
SEEN = {}
ROWS = ("torques", "actions", "last_actions", "last_dof_vel", "dof_state")  # post_a's vector rows
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for f, (r32, rbar) in sorted(SEEN.items()):
        print(f"[task ratios] {f}: err_kernel / err_f32 <= {r32:.3g}, err_kernel / bar <= {rbar:.3g}")


def _gt():
    from isaacgymenv_amd import gymtask
    return gymtask


def _lib():
    return _gt().lib()


def _err():
    return _lib().gt_last_error().decode()


def _field(fails, what, field, got, r64, r32, err_32=None, zeros=False):
    H.field_check("task", SEEN, fails, what, field, got, r64, r32, zeros=zeros, err_32=err_32)


class Dev:
    """Device buffers, each inside its own 0xA5-filled allocation at byte offset `off`."""

    def __init__(self):
        self.raw, self.init = {}, {}

    def add(self, name, arr, off=0):
        arr = np.ascontiguousarray(arr)
        raw = torch.full((off + arr.nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        if arr.nbytes:
            raw[off:off + arr.nbytes].copy_(torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()))
        self.raw[name] = (raw, off, arr.nbytes, arr.dtype, arr.shape)
        self.init[name] = arr.copy()
        return raw.data_ptr() + off

    def ptr(self, name):
        raw, off = self.raw[name][:2]
        return raw.data_ptr() + off

    def get(self, name):
        raw, off, nb, dt, shape = self.raw[name]
        return raw[off:off + nb].cpu().numpy().view(dt).reshape(shape)

    def set(self, name, arr):
        raw, off, nb, dt, shape = self.raw[name]
        arr = np.ascontiguousarray(arr, dtype=dt)
        raw[off:off + nb].copy_(torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()))
        self.init[name] = arr.reshape(shape).copy()

    def intact(self, what):
        torch.cuda.synchronize()
        for name, (raw, off, nb, _, _) in self.raw.items():
            assert bool((raw[:off] == FILL).all()) and bool((raw[off + nb:] == FILL).all()), \
                f"{what}: wrote outside {name}"

    def unchanged(self, names, what):
        self.intact(what)
        for name in names:
            a, b = self.get(name), self.init[name]
            assert a.tobytes() == b.tobytes(), f"{what}: {name} changed"

    def all_unchanged(self, what):
        self.unchanged(list(self.raw), what)


def _cparams(p):
    s = _gt().GtAnymalParams()
    for k, v in p.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(s, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(s, k, v)
    return s


CONST = ("contact_forces", "torques", "actions", "timeout_buf", "noise_scale")
NAN = float("nan")


def _setup(p, b, hd=None, off=0, masks=True, obs_out=True, time_outs=True, mirror=False, heights=None,
           clip_obs=np.inf, timeout64=False):
    """(Dev, GtAnymalBuffers, keepalive) for the inputs of tail_inputs; the row tensors at byte offset `off`."""
    N, no = p["num_envs"], p["num_obs"]
    d = Dev()
    B = _gt().GtAnymalBuffers()
    f = lambda *s: np.full(s, NAN, F32)  # noqa: E731
    tb = b["timeout_buf"].astype(np.int64) if timeout64 else b["timeout_buf"].astype(np.uint8)
    arrays = dict(root_states=b["root_states"], contact_forces=b["contact_forces"], dof_state=b["dof_state"],
                  torques=b["torques"], actions=b["actions"], last_actions=b["last_actions"],
                  last_dof_vel=b["last_dof_vel"], commands=b["commands"], feet_air_time=b["feet_air_time"],
                  progress_buf=b["progress_buf"], randomize_buf=b["randomize_buf"],
                  reset_buf=np.full(N, 7, np.uint8) if "reset_in" not in b else b["reset_in"], timeout_buf=tb,
                  rew_buf=f(N), episode_sums=b["episode_sums"],
                  base_lin_vel=b.get("base_lin_vel", f(N, 3)), base_ang_vel=b.get("base_ang_vel", f(N, 3)),
                  projected_gravity=b.get("projected_gravity", f(N, 3)), obs_buf=f(N, no),
                  noise_scale=b["noise_scale"], reset_count=np.zeros(3, np.int32))
    for name, arr in arrays.items():
        setattr(B, name, d.add(name, arr, off if name in ROWS else 0))
    B.timeout_is_int64 = int(timeout64)
    if masks:
        B.reset_masks = d.add("reset_masks", np.full((N + 63) // 64, ALL_ONES, np.uint64))
    if obs_out:
        B.obs_out = d.add("obs_out", f(N, no))
    if time_outs:
        B.time_outs = d.add("time_outs", np.full(N, 7, np.uint8))
    if mirror:
        B.obs_mirror = d.add("obs_mirror", f(N, no))
    if heights is not None:
        B.measured_heights = d.add("measured_heights", heights)
    B.clip_obs = clip_obs
    keep = []
    if hd is not None:
        h = _gt().GtAnymalHound()
        h.num_actions, h.num_shoulders = hd["num_actions"], hd["num_shoulders"]
        for i, x in enumerate(hd["shoulder_idx"]):
            h.shoulder_idx[i] = x
        h.eef_state = d.add("eef_state", hd["eef_rows"])
        h.eef_stride = 13
        h.arm_commands = d.add("arm_commands", hd["arm_commands"])
        h.pos_control = d.add("pos_control", hd.get("pos_control", f(N, 6)))
        h.effort_control = d.add("effort_control", hd.get("effort_control", f(N, 6)))
        for name in ("arm_default", "arm_lower", "arm_upper"):
            getattr(h, name)[:] = hd[name]
        h.arm_noise2 = hd["arm_noise2"]
        if "u_arm" in hd:
            h.u_arm = d.add("u_arm", hd["u_arm"])
        B.hound = C.cast(C.pointer(h), C.c_void_p)
        keep.append(h)
    return d, B, keep


def _sync():
    torch.cuda.synchronize()


# ============================================================================================ gt_anymal_post_physics_a
A_FLOAT = ("base_lin_vel", "base_ang_vel", "projected_gravity", "feet_air_time", "rew_buf", "episode_sums")


def _check_post_a(what, p, b, d, hd=None, masks=True, timeout64=False):
    """The buffers of `d` after gt_anymal_post_physics_a against the oracle on (p, b)."""
    bb = dict(b, timeout_buf=b["timeout_buf"].astype(np.int64) if timeout64 else b["timeout_buf"])
    o64, o32 = O.post_a(p, bb, hound=hd), O.post_a(p, bb, hound=hd, dtype=F32)
    fails = []
    for f in ("progress_buf", "randomize_buf", "reset_buf"):
        np.testing.assert_array_equal(d.get(f), o64[f], err_msg=f"{what} {f}")
    if masks:
        np.testing.assert_array_equal(d.get("reset_masks"), o64["reset_masks"], err_msg=f"{what} masks")
    assert d.get("reset_count").tolist() == [0, 0, o64["count"]], (what, d.get("reset_count"), o64["count"])
    for f in A_FLOAT:
        _field(fails, what, f, d.get(f), o64[f], o32[f], zeros=f in ("rew_buf", "feet_air_time"))
    cmd = d.get("commands")
    _field(fails, what, "commands2", cmd[:, 2], o64["commands2"], o32["commands2"])
    np.testing.assert_array_equal(cmd[:, [0, 1, 3]], b["commands"][:, [0, 1, 3]], err_msg=f"{what} commands")
    nf = p["num_feet"]
    assert d.get("feet_air_time")[:, nf:].tobytes() == b["feet_air_time"][:, nf:].tobytes(), f"{what}: air time past feet"
    d.unchanged(CONST + ("root_states", "dof_state", "last_actions", "last_dof_vel"), what)
    assert not fails, "\n".join(fails)
    return o64, o32


def _post_a(p, B, what, expect=0):
    rc = _lib().gt_anymal_post_physics_a(C.byref(_cparams(p)), C.byref(B), None)
    _sync()
    assert rc == expect, (what, rc, _err())


A_NS = (1, 15, 17, 63, 64, 65, 130, 4161)
A_FORMS = {"nd12": (12, 0), "nd16": (16, 0), "nd12_unaligned": (12, 4), "nd10": (10, 0), "nd13": (13, 0)}


@pytest.mark.parametrize("form", list(A_FORMS))
@pytest.mark.parametrize("N", A_NS)
def test_post_a_matches_float64_reference(N, form):
    """The straight-line form (nd 12 aligned), the runtime-nd vector form (nd 16) and the scalar form (rows offset by
    one float; nd 10, 13) on every kind of env, the mask words pre-filled with ones; run twice: the same bits."""
    nd, off = A_FORMS[form]
    p, b, _ = H.tail_inputs(N, nd, seed=N)
    what = f"post_a N={N} {form}"
    outs = []
    for rep in range(2):
        d, B, _ = _setup(p, b, off=off)
        _post_a(p, B, what)
        _check_post_a(what, p, b, d) if rep == 0 else None
        outs.append({f: d.get(f).tobytes() for f in A_FLOAT + ("commands", "reset_masks", "reset_buf")})
    assert outs[0] == outs[1], f"{what}: two runs differ"
    # a second call on the same words counts again from a re-armed accumulator
    before = d.get("reset_count")[2]
    d.set("progress_buf", b["progress_buf"])
    _post_a(p, B, what)
    assert d.get("reset_count").tolist() == [0, 0, before]


@pytest.mark.parametrize("num_shoulders", [0, 2, 4])
def test_post_a_hound_form(num_shoulders):
    N = 65
    p, b, kind = H.tail_inputs(N, 12, seed=N, hound=True)
    hd = H.tail_hound(N, num_shoulders=num_shoulders)
    d, B, keep = _setup(p, b, hd=hd)
    what = f"post_a hound shoulders={num_shoulders}"
    _post_a(p, B, what)
    o64, _ = _check_post_a(what, p, b, d, hd=hd)
    sh = kind == H.TAIL_KINDS.index("shoulder")
    # tail_inputs loads shoulder slot 1: counted with 2 and 4 shoulders, not with 0
    assert (o64["sh_count"][sh] == (1 if num_shoulders else 0)).all() and bool(o64["reset_buf"][sh].all()) == (num_shoulders > 0)
    d.unchanged(("eef_state", "arm_commands", "pos_control", "effort_control"), what)


@pytest.mark.parametrize("form", ["nd12", "nd16", "nd12_unaligned"])
@pytest.mark.parametrize("over", [dict(allow_knee_contacts=1), dict(num_knees=2, num_feet=3), dict(timeout64=True),
                                  dict(masks=False), dict(host=True)],
                         ids=["allow_knees", "knees2_feet3", "timeout_int64", "no_masks", "host_count"])
def test_post_a_switches(over, form):
    N = 130
    nd, off = A_FORMS[form]
    over = dict(over)
    t64, masks, host = over.pop("timeout64", False), over.pop("masks", True), over.pop("host", False)
    p, b, kind = H.tail_inputs(N, nd, seed=N)
    p.update(over)
    d, B, _ = _setup(p, b, off=off, masks=masks, timeout64=t64)
    what = f"post_a {form} {over} t64={t64} masks={masks} host={host}"
    hp = C.c_void_p()
    if host:
        dp = C.c_void_p()
        assert _lib().gt_host_alloc(8, C.byref(hp), C.byref(dp)) == 0
        B.host_count, B.seq = dp.value, 77
    try:
        _post_a(p, B, what)
        o64, _ = _check_post_a(what, p, b, d, masks=masks, timeout64=t64)
        if host:
            words = (C.c_int32 * 2).from_address(hp.value)
            assert [words[0], words[1]] == [o64["count"], 77]
    finally:
        if host:
            _lib().gt_host_free(hp)
    if "allow_knee_contacts" in over:
        assert not o64["reset_buf"][kind == H.TAIL_KINDS.index("knee_many")].any()
    if t64:  # ~int64: -1 for 0 (the penalty's sign flips), -2 for 1
        tr = kind == H.TAIL_KINDS.index("timeout_reset")
        bc = kind == H.TAIL_KINDS.index("base_contact")
        assert (o64["rew_buf"][bc] > np.maximum(o64["rew_preclip"][bc], 0)).all()
        pen = -float(np.float32(p["s_termination"]))
        assert np.allclose(o64["rew_buf"][tr] - np.maximum(o64["rew_preclip"][tr], 0), 2 * pen, rtol=1e-6)
        assert np.allclose(o64["rew_buf"][bc] - np.maximum(o64["rew_preclip"][bc], 0), pen, rtol=1e-6)


def test_num_dofs_below_10_is_refused():
    """The hip term reads dofs 0, 3, 6, 9: 9 dofs are refused by every gt_anymal_* entry point, nothing written."""
    N = 17
    p, b, _ = H.tail_inputs(N, 10, seed=1)
    q = H.tail_params(N, 9)
    b9 = dict(b, dof_state=b["dof_state"][:, :9], torques=b["torques"][:, :9], actions=b["actions"][:, :9],
              last_actions=b["last_actions"][:, :9], last_dof_vel=b["last_dof_vel"][:, :9],
              noise_scale=b["noise_scale"][:q["num_obs"]])
    d, B, _ = _setup(q, b9)
    L, P = _lib(), _cparams(q)
    for name, call in (("post_physics_a", lambda: L.gt_anymal_post_physics_a(C.byref(P), C.byref(B), None)),
                       ("post_physics_b", lambda: L.gt_anymal_post_physics_b(C.byref(P), C.byref(B), None, None, None)),
                       ("post_physics_ab", lambda: L.gt_anymal_post_physics_ab(C.byref(P), C.byref(B), None, None))):
        assert call() != 0, name
        assert "0, 3, 6, 9" in _err() and "num_dofs" in _err(), _err()
        d.all_unchanged(f"num_dofs 9 {name}")
    p10 = H.tail_params(N, 10)
    d, B, _ = _setup(p10, b)
    _post_a(p10, B, "num_dofs 10")


# ============================================================================================ gt_anymal_post_physics_b
def _b_inputs(N, nd=12, hound=False, **over):
    """Inputs of post_b: tail_inputs with post_a's float32 results in place (the oracle's)."""
    p, b, _ = H.tail_inputs(N, nd, seed=N, hound=hound)
    p.update(over)
    hd = H.tail_hound(N) if hound else None
    a = O.post_a(p, b, hound=hd, dtype=F32)
    b = dict(b, base_lin_vel=a["base_lin_vel"], base_ang_vel=a["base_ang_vel"], projected_gravity=a["projected_gravity"],
             commands=a["commands"], progress_buf=a["progress_buf"], reset_in=a["reset_buf"], reset_buf=a["reset_buf"])
    if hd:
        hd = dict(hd, eef=hd["eef_rows"][:, :7])
    return p, b, hd


def _post_b(p, B, noise, plan, what, expect=0):
    rc = _lib().gt_anymal_post_physics_b(C.byref(_cparams(p)), C.byref(B), noise, plan, None)
    _sync()
    assert rc == expect, (what, rc, _err())


def _check_post_b(what, p, b, d, hd, noise, heights, clip, obs_out=True, time_outs=True, mirror=False):
    bb = dict(b, measured_heights=heights, clip_obs=clip)
    o64, o32 = O.post_b(p, bb, noise, hound=hd), O.post_b(p, bb, noise, hound=hd, dtype=F32)
    fails = []
    _field(fails, what, "obs_buf", d.get("obs_buf"), o64["obs_buf"], o32["obs_buf"])
    got = d.get("obs_buf")
    if obs_out:  # the clamped copy of what the kernel itself stored
        assert d.get("obs_out").tobytes() == np.clip(got, -F32(clip), F32(clip)).tobytes(), f"{what}: obs_out"
    if mirror:
        assert d.get("obs_mirror").tobytes() == d.get("obs_out").tobytes(), f"{what}: obs_mirror"
    if time_outs:
        np.testing.assert_array_equal(d.get("time_outs"), o64["time_outs"], err_msg=f"{what} time_outs")
    assert d.get("last_actions").tobytes() == b["actions"].tobytes(), f"{what}: last_actions"
    nd = p["num_dofs"]
    assert d.get("last_dof_vel").tobytes() == np.ascontiguousarray(b["dof_state"][:, :nd, 1]).tobytes(), f"{what}: last_dof_vel"
    d.unchanged(CONST + ("root_states", "dof_state", "commands", "base_lin_vel", "base_ang_vel", "projected_gravity",
                         "progress_buf", "reset_buf", "episode_sums", "feet_air_time"), what)
    assert not fails, "\n".join(fails)
    return o64


@pytest.mark.parametrize("shape", ["anymal188", "nd16_200", "hound204"])
@pytest.mark.parametrize("N", [1, 17, 65])
def test_post_b_matches_float64_reference(N, shape):
    """num_obs 188 / 200 / 204: no noise, a drawn buffer, and the plan -- which must equal, bit for bit, the buffer
    run fed with torch.rand from the same generator state; obs_out / time_outs / obs_mirror set."""
    nd, hound = dict(anymal188=(12, False), nd16_200=(16, False), hound204=(12, True))[shape]
    p, b, hd = _b_inputs(N, nd, hound)
    no = p["num_obs"]
    assert no == dict(anymal188=188, nd16_200=200, hound204=204)[shape]
    what = f"post_b N={N} {shape}"
    d, B, keep = _setup(p, b, hd=hd, mirror=True)
    _post_b(p, B, None, None, what + " no noise")
    _check_post_b(what + " no noise", p, b, d, hd, None, None, np.inf, mirror=True)
    planner = _gt().TorchRandPlanner("cuda:0")
    g = planner.gen
    g.manual_seed(99 + N)
    torch.rand(77, device=DEV)
    off0 = g.get_offset()
    noise = torch.rand(N, no, device=DEV)
    off1 = g.get_offset()
    d1, B1, keep1 = _setup(p, b, hd=hd)
    _post_b(p, B1, noise.data_ptr(), None, what + " buffer")
    _check_post_b(what + " buffer", p, b, d1, hd, noise.cpu().numpy(), None, np.inf)
    g.set_offset(off0)
    plan = planner.plan(N * no)
    assert g.get_offset() == off1
    d2, B2, keep2 = _setup(p, b, hd=hd)
    _post_b(p, B2, None, C.byref(plan), what + " plan")
    for f in ("obs_buf", "obs_out", "time_outs", "last_actions", "last_dof_vel"):
        assert d2.get(f).tobytes() == d1.get(f).tobytes(), f"{what}: plan and buffer runs differ in {f}"
    d2.intact(what + " plan")


@pytest.mark.parametrize("N", [1, 17, 65])
def test_post_b_switches(N):
    """clip_obs 5 with observations beyond it on both sides; measured heights with the +-1 clip binding on both sides;
    obs_out / time_outs NULL."""
    p, b, hd = _b_inputs(N, dof_pos_scale=30.0)
    heights = H.tail_heights(N)
    d, B, _ = _setup(p, b, heights=heights, clip_obs=5.0)
    what = f"post_b N={N} clip 5 heights"
    _post_b(p, B, None, None, what)
    o = _check_post_b(what, p, b, d, None, None, heights, 5.0)
    assert (o["obs_buf"] > 5).any() and (o["obs_buf"] < -5).any() and np.abs(o["obs_out"]).max() == 5.0
    hcols = o["obs_buf"][:, 36:176] / p["height_meas_scale"]
    if N > 1:
        assert (hcols == 1).any() and (hcols == -1).any() and (np.abs(hcols) < 1).any()
    d.unchanged(("measured_heights",), what)
    d, B, _ = _setup(p, b, obs_out=False, time_outs=False)
    what = f"post_b N={N} no obs_out, no time_outs"
    _post_b(p, B, None, None, what)
    _check_post_b(what, p, b, d, None, None, None, np.inf, obs_out=False, time_outs=False)


# =========================================================================================== gt_anymal_post_physics_ab
AB_OUT = ("progress_buf", "randomize_buf", "reset_buf", "reset_masks", "reset_count", "rew_buf", "episode_sums",
          "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "feet_air_time", "obs_buf", "obs_out",
          "time_outs", "last_actions", "last_dof_vel", "obs_mirror")


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 40, 64, 65, 80, 4161])
def test_post_ab_equals_a_then_b(N, noise):
    """One launch = post_a followed by post_b on copies of the same buffers, bit for bit (mask words pre-filled with
    ones: the 16-bit slices past the last env must be cleared), and inside the rule against the oracle."""
    p, b, _ = H.tail_inputs(N, 12, seed=N)
    what = f"post_ab N={N} noise={noise}"
    planner = _gt().TorchRandPlanner("cuda:0")
    planner.gen.manual_seed(5 + N)
    plan = planner.plan(N * p["num_obs"]) if noise else None
    pl = C.byref(plan) if noise else None
    d1, B1, _ = _setup(p, b, mirror=True, clip_obs=5.0)
    _post_a(p, B1, what)
    o64, o32 = _check_post_a(what + " (a)", p, b, d1)
    _post_b(p, B1, None, pl, what)
    d2, B2, _ = _setup(p, b, mirror=True, clip_obs=5.0)
    rc = _lib().gt_anymal_post_physics_ab(C.byref(_cparams(p)), C.byref(B2), pl, None)
    _sync()
    assert rc == 0, (what, _err())
    for f in AB_OUT:
        assert d2.get(f).tobytes() == d1.get(f).tobytes(), f"{what}: {f} differs from post_a + post_b"
    d2.unchanged(CONST + ("root_states", "dof_state"), what)
    if not noise:  # the observations against the oracle, as a function of part A's stored results
        bb = dict(b, clip_obs=5.0, **{f: d2.get(f) for f in ("base_lin_vel", "base_ang_vel", "projected_gravity",
                                                             "commands", "progress_buf", "reset_buf")})
        r64, r32 = O.post_b(p, bb), O.post_b(p, bb, dtype=F32)
        fails = []
        _field(fails, what, "ab obs_buf", d2.get("obs_buf"), r64["obs_buf"], r32["obs_buf"])
        np.testing.assert_array_equal(d2.get("time_outs"), r64["time_outs"])
        assert not fails, "\n".join(fails)


def test_post_ab_refusals():
    """Every refusal of its header comment: UsefulHound, num_dofs != 12, measured heights, reset_count / reset_masks
    NULL, each row tensor off 16-byte alignment, a noise plan that does not cover obs_buf."""
    N = 17
    L = _lib()

    def refused(p, d, B, plan, what):
        rc = L.gt_anymal_post_physics_ab(C.byref(_cparams(p)), C.byref(B), plan, None)
        _sync()
        assert rc != 0 and "gt_anymal_post_physics_ab" in _err(), (what, rc, _err())
        d.all_unchanged(what)

    p, b, _ = H.tail_inputs(N, 12, seed=3)
    hp, hb, _ = H.tail_inputs(N, 12, seed=3, hound=True)
    d, B, keep = _setup(hp, hb, hd=H.tail_hound(N))
    refused(hp, d, B, None, "hound")
    p16, b16, _ = H.tail_inputs(N, 16, seed=3)
    d, B, _ = _setup(p16, b16)
    refused(p16, d, B, None, "nd 16")
    d, B, _ = _setup(p, b, heights=H.tail_heights(N))
    refused(p, d, B, None, "measured heights")
    d, B, _ = _setup(p, b, masks=False)
    refused(p, d, B, None, "no masks")
    d, B, _ = _setup(p, b)
    B.reset_count = None
    refused(p, d, B, None, "no reset_count")
    for row in ROWS:
        d, B, _ = _setup(p, b)
        extra = d.add(row + "_off", d.init[row], off=4)
        setattr(B, row, extra)
        refused(p, d, B, None, f"{row} unaligned")
    GT = _gt()
    for plan in (GT.GtTorchRandPlan(1, 0, 256, N * p["num_obs"] - 1), GT.GtTorchRandPlan(1, 0, 0, N * p["num_obs"])):
        d, B, _ = _setup(p, b)
        refused(p, d, B, C.byref(plan), "short plan")


# ============================================================================================= gt_anymal_reset_flagged
RESET_OUT = ("dof_state", "root_states", "commands", "last_actions", "last_dof_vel", "feet_air_time", "progress_buf",
             "reset_buf", "episode_sums")


def _draws_struct(d, draws, k):
    s = _gt().GtAnymalResetDraws()
    for n in ("u_pos", "u_vel", "u_cmd_x", "u_cmd_y", "u_cmd_h"):
        if draws.get(n) is not None:
            setattr(s, n, d.add(n, draws[n]))
    for n, v in draws.items():
        if n.endswith("_range") or n.endswith("_lower"):
            setattr(s, n, v)
    return s


def _terrain_struct(d, tr):
    s = _gt().GtAnymalTerrainReset()
    for n in ("terrain_levels", "terrain_types", "env_origins", "terrain_origins", "u_root_xy"):
        if tr.get(n) is not None:
            setattr(s, n, d.add(n, tr[n]))
    for n in ("env_rows", "env_cols", "update_levels", "env_length", "max_episode_length_s", "xy_range", "xy_lower"):
        setattr(s, n, tr[n])
    return s


def _ep_err32(N, ids, len_s):
    """The float32 oracle's error of episode_out over the episode sums of seeds 0..15 of this shape."""
    if not len(ids):
        return 0.0
    return max(float(np.abs(O.episode_out(s, ids, len_s, F32) - O.episode_out(s, ids, len_s)).max())
               for s in (H.tail_episode_sums(N, seed) for seed in range(16)))


def _reset_flagged_case(N, masks, what, terrain=False, hound=False, update_levels=1, scratch=None, batch_norm=0.4):
    """One gt_anymal_reset_flagged call on hand-built masks, compared in full.  Returns (Dev, scratch)."""
    k = H.popcount(masks)
    p, b, _ = H.tail_inputs(N, 12, seed=N, hound=hound)
    b["reset_in"] = np.zeros(N, np.uint8)
    b["reset_buf"] = b["reset_in"]
    draws, extra = H.reset_draws(k, 12, seed=N, terrain=terrain, hound=hound)
    hd = dict(H.tail_hound(N), pos_control=np.full((N, 6), 3.0, F32), effort_control=np.full((N, 6), 4.0, F32),
              **{n: v for n, v in extra.items() if n == "u_arm"}) if hound else None
    tr = None
    if terrain:
        tr, root_xy, cmd_xy, _ = H.terrain_reset_inputs(N, O.ids_of(masks, N), update_levels=update_levels,
                                                        batch_norm=batch_norm)
        tr["u_root_xy"] = extra["u_root_xy"]
        b["root_states"] = b["root_states"].copy()
        b["commands"] = b["commands"].copy()
        b["root_states"][:, :2], b["commands"][:, :2] = root_xy, cmd_xy
    d, B, keep = _setup(p, b, hd=hd)
    d.set("reset_masks", masks)
    ds = _draws_struct(d, draws, k)
    ts = _terrain_struct(d, tr) if terrain else None
    ids_ptr = d.add("env_ids", np.full(k, -7, np.int32))
    ne = 14 if terrain else 13
    ep_ptr = d.add("episode_out", np.full(ne, NAN, F32))
    words = 16 + 14 * ((N + 63) // 64)
    if scratch is None:
        scratch = torch.zeros(words + 16, dtype=torch.float32, device=DEV)
        scratch[words:] = NAN
    len_s = 20.0
    L = _lib()
    rc = L.gt_anymal_reset_flagged(C.byref(_cparams(p)), C.byref(B), k, C.byref(ds), C.byref(ts) if ts else None,
                                   ids_ptr, ep_ptr, len_s, scratch.data_ptr(), None)
    _sync()
    assert rc == 0, (what, _err())
    assert bool(torch.isnan(scratch[words:]).all()), f"{what}: scratch written past its documented size"
    assert bool((scratch[:16].view(torch.int32) == 0).all()), f"{what}: the scratch counter is not re-armed"
    if k == 0:
        d.all_unchanged(what + " k=0")
        return d, scratch
    hh = dict(hd, u_arm=extra["u_arm"]) if hound else None
    r64 = O.reset_flagged(p, b, masks, draws, terrain=tr, hound=hh, episode_length_s=len_s)
    r32 = O.reset_flagged(p, b, masks, draws, terrain=tr, hound=hh, episode_length_s=len_s, dtype=F32)
    ids = r64["env_ids"]
    np.testing.assert_array_equal(d.get("env_ids"), ids, err_msg=what)
    flagged = np.zeros(N, bool)
    flagged[ids] = True
    fails = []
    for f in ("dof_state", "root_states", "commands"):
        _field(fails, what, "reset " + f, d.get(f), r64[f], r32[f], zeros=True)
        assert d.get(f)[~flagged].tobytes() == d.init[f][~flagged].tobytes(), f"{what}: {f} of unflagged envs"
    for f in ("last_actions", "last_dof_vel", "feet_air_time", "progress_buf", "reset_buf"):
        np.testing.assert_array_equal(d.get(f), r64[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(d.get("episode_sums"), r64["episode_sums"].astype(F32), err_msg=f"{what} sums")
    _field(fails, what, "episode_out", d.get("episode_out")[:13], r64["episode_out"][:13], r32["episode_out"][:13],
           err_32=_ep_err32(N, ids, len_s))
    if terrain:
        np.testing.assert_array_equal(d.get("terrain_levels"), r64["terrain_levels"], err_msg=what)
        assert d.get("env_origins").tobytes() == r64["env_origins"].astype(F32).tobytes(), f"{what}: env_origins"
        _field(fails, what, "terrain level mean", d.get("episode_out")[13:], r64["episode_out"][13:], r32["episode_out"][13:])
        d.unchanged(("terrain_types", "terrain_origins", "u_root_xy"), what)
    if hound:
        for f in ("pos_control", "effort_control"):
            _field(fails, what, "reset " + f, d.get(f), r64[f], r32[f])
            assert d.get(f)[~flagged].tobytes() == d.init[f][~flagged].tobytes(), f"{what}: {f} of unflagged envs"
    d.unchanged(CONST + ("rew_buf", "obs_buf", "base_lin_vel", "randomize_buf", "reset_masks", "u_pos", "u_vel",
                         "u_cmd_x", "u_cmd_y", "u_cmd_h"), what)
    assert not fails, "\n".join(fails)
    return d, scratch


RESET_NS = (1, 63, 65, 130, 4161)


@pytest.mark.parametrize("N", RESET_NS)
def test_reset_flagged_plane_every_mask_pattern(N):
    """Every hand-built pattern; the same pattern twice (the same bits); then all patterns in a row on ONE scratch
    buffer (the counter re-arms itself)."""
    cases = H.reset_masks_cases(N)
    scratch = None
    for name, m in cases.items():
        d1, _ = _reset_flagged_case(N, m, f"reset_flagged N={N} {name}")
        d2, scratch = _reset_flagged_case(N, m, f"reset_flagged N={N} {name} (shared scratch)", scratch=scratch)
        for f in RESET_OUT + ("episode_out", "env_ids"):
            assert d1.get(f).tobytes() == d2.get(f).tobytes(), f"N={N} {name}: {f} differs between two runs"


@pytest.mark.parametrize("update_levels,batch_norm", [(0, 0.4), (1, 0.4), (1, 2.0)])
@pytest.mark.parametrize("N", RESET_NS)
def test_reset_flagged_terrain(N, update_levels, batch_norm):
    """The curriculum on the norm of ALL flagged envs' commands (levels down, up, neither, both at once, the clip at 0,
    the wrap at env_rows), the unflagged envs' commands not counted; two calls in a row on one scratch buffer."""
    cases = H.reset_masks_cases(N)
    scratch = None
    for name in ("all", "alternating") + (("first_and_last_wave",) if N > 4096 else ()):
        _, scratch = _reset_flagged_case(N, cases[name], f"reset_flagged terrain N={N} {name} update={update_levels} "
                                         f"norm={batch_norm}", terrain=True, update_levels=update_levels,
                                         batch_norm=batch_norm, scratch=scratch)


@pytest.mark.parametrize("N", [1, 65, 130])
def test_reset_flagged_hound(N):
    cases = H.reset_masks_cases(N)
    for name in ("all", "alternating", "last"):
        _reset_flagged_case(N, cases[name], f"reset_flagged hound N={N} {name}", hound=True)
    _reset_flagged_case(N, cases["all"], f"reset_flagged hound terrain N={N}", hound=True, terrain=True)


@pytest.mark.parametrize("N,pattern", [(130, "alternating"), (4161, "first_and_last_wave")])
def test_reset_flagged_plans_equal_drawn_buffers(N, pattern):
    """The five plans evaluated in-kernel = the drawn-buffer run fed with torch.rand from the same generator state."""
    masks = H.reset_masks_cases(N)[pattern]
    k = H.popcount(masks)
    p, b, _ = H.tail_inputs(N, 12, seed=N)
    planner = _gt().TorchRandPlanner("cuda:0")
    g = planner.gen
    g.manual_seed(1000 + N)
    torch.rand(5, device=DEV)
    off0 = g.get_offset()
    us = [torch.rand(s, device=DEV).cpu().numpy() for s in ((k, 12), (k, 12), (k,), (k,), (k,))]
    g.set_offset(off0)
    plans = planner.plan_many((k * 12, k * 12, k, k, k))
    base, _ = H.reset_draws(k, 12)
    outs = []
    for mode in ("buffers", "plans"):
        d, B, _ = _setup(p, b)
        d.set("reset_masks", masks)
        draws = dict(base, **dict(zip(("u_pos", "u_vel", "u_cmd_x", "u_cmd_y", "u_cmd_h"),
                                      us if mode == "buffers" else [None] * 5)))
        ds = _draws_struct(d, draws, k)
        if mode == "plans":
            ds.plan_pos, ds.plan_vel, ds.plan_cmd_x, ds.plan_cmd_y, ds.plan_cmd_h = plans
        ids_ptr, ep_ptr = d.add("env_ids", np.zeros(k, np.int32)), d.add("episode_out", np.zeros(13, F32))
        scratch = torch.zeros(16 + 14 * ((N + 63) // 64), dtype=torch.float32, device=DEV)
        rc = _lib().gt_anymal_reset_flagged(C.byref(_cparams(p)), C.byref(B), k, C.byref(ds), None, ids_ptr, ep_ptr,
                                            20.0, scratch.data_ptr(), None)
        _sync()
        assert rc == 0, _err()
        d.intact(mode)
        outs.append({f: d.get(f).tobytes() for f in RESET_OUT + ("env_ids", "episode_out")})
    assert outs[0] == outs[1]


def test_reset_flagged_refusals():
    N = 65
    masks = H.reset_masks_cases(N)["alternating"]
    k = H.popcount(masks)
    p, b, _ = H.tail_inputs(N, 12, seed=N)
    draws, extra = H.reset_draws(k, 12, terrain=True)
    tr, _, _, _ = H.terrain_reset_inputs(N)
    tr["u_root_xy"] = extra["u_root_xy"]
    L = _lib()
    scratch = torch.zeros(16 + 14 * 2, dtype=torch.float32, device=DEV)
    for what in ("k<0", "k>N", "draws", "ids", "episode_out", "scratch", "masks", "terrain_levels", "terrain_types",
                 "env_origins", "terrain_origins", "env_rows", "env_cols"):
        d, B, _ = _setup(p, b, masks=what != "masks")
        if what != "masks":
            d.set("reset_masks", masks)
        ds = _draws_struct(d, draws, k)
        ts = _terrain_struct(d, tr)
        if what in ("terrain_levels", "terrain_types", "env_origins", "terrain_origins"):
            setattr(ts, what, None)
        elif what in ("env_rows", "env_cols"):
            setattr(ts, what, 0)
        terr = what.startswith("terrain") or what.startswith("env_")
        ids_ptr, ep_ptr = d.add("env_ids", np.zeros(k, np.int32)), d.add("episode_out", np.zeros(14, F32))
        rc = L.gt_anymal_reset_flagged(C.byref(_cparams(p)), C.byref(B), -1 if what == "k<0" else N + 1 if what == "k>N" else k,
                                       None if what == "draws" else C.byref(ds), C.byref(ts) if terr else None,
                                       None if what == "ids" else ids_ptr, None if what == "episode_out" else ep_ptr,
                                       20.0, None if what == "scratch" else scratch.data_ptr(), None)
        _sync()
        assert rc != 0 and "gt_anymal_reset_flagged" in _err(), (what, rc, _err())
        d.all_unchanged("refusal " + what)
        assert bool((scratch == 0).all())


# ===================================================================================================== gt_anymal_reset
@pytest.mark.parametrize("k", [0, 1, 65, 130])
def test_reset_explicit_ids(k):
    """Explicit ids with -1 and N mixed in: skipped, not summed; k = 0 zeroes episode_out and writes nothing else."""
    N = 200
    p, b, _ = H.tail_inputs(N, 12, seed=k)
    rng = np.random.RandomState(k)
    ids = rng.permutation(N)[:k].astype(np.int32)
    if k > 1:
        ids[3::7] = -1
        ids[5::11] = N
    draws, _ = H.reset_draws(k, 12, seed=k)
    off = (draws["u_pos"] + F32(0.5)).astype(F32)
    vel = (draws["u_vel"] * F32(0.2) - F32(0.1)).astype(F32)
    cx, cy, ch = (draws[n] * F32(2) - F32(1) for n in ("u_cmd_x", "u_cmd_y", "u_cmd_h"))
    d, B, _ = _setup(p, b)
    ptrs = [d.add(n, a) for n, a in (("ids", ids), ("off", off), ("vel", vel), ("cx", cx), ("cy", cy), ("ch", ch))]
    ep = d.add("episode_out", np.full(13, NAN, F32))
    rc = _lib().gt_anymal_reset(C.byref(_cparams(p)), C.byref(B), ptrs[0], k, *ptrs[1:], ep, None)
    _sync()
    what = f"gt_anymal_reset k={k}"
    assert rc == 0, (what, _err())
    bb = dict(b, reset_buf=np.full(N, 7, np.uint8))
    r64 = O.reset(p, bb, ids, off, vel, cx, cy, ch)
    r32 = O.reset(p, bb, ids, off, vel, cx, cy, ch, dtype=F32)
    if k == 0:
        assert (d.get("episode_out") == 0).all()
        d.unchanged([n for n in d.raw if n != "episode_out"], what)
        return
    valid = ids[(ids >= 0) & (ids < N)]
    touched = np.zeros(N, bool)
    touched[valid] = True
    fails = []
    for f in ("dof_state", "root_states", "commands"):
        _field(fails, what, "reset " + f, d.get(f), r64[f], r32[f], zeros=True)
        assert d.get(f)[~touched].tobytes() == d.init[f][~touched].tobytes(), f"{what}: {f} of other envs"
    for f in ("last_actions", "last_dof_vel", "feet_air_time", "progress_buf", "reset_buf"):
        np.testing.assert_array_equal(d.get(f), r64[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(d.get("episode_sums"), r64["episode_sums"].astype(F32))
    err32 = max(float(np.abs(O.episode_sum(s, valid, F32) - O.episode_sum(s, valid)).max())
                for s in (H.tail_episode_sums(N, seed) for seed in range(16)))
    _field(fails, what, "reset episode_out", d.get("episode_out"), r64["episode_out"], r32["episode_out"], err_32=err32)
    d.unchanged(CONST + ("ids", "off", "vel", "cx", "cy", "ch", "rew_buf", "randomize_buf"), what)
    assert not fails, "\n".join(fails)


def test_reset_explicit_ids_refuses_hound():
    N = 17
    p, b, _ = H.tail_inputs(N, 12, seed=N, hound=True)
    d, B, keep = _setup(p, b, hd=H.tail_hound(N))
    z = d.add("z", np.zeros(N * 12, F32))
    ids = d.add("ids", np.arange(N, dtype=np.int32))
    ep = d.add("episode_out", np.full(13, NAN, F32))
    rc = _lib().gt_anymal_reset(C.byref(_cparams(p)), C.byref(B), ids, N, z, z, z, z, z, ep, None)
    _sync()
    assert rc != 0 and "gt_anymal_reset" in _err() and "UsefulHound" in _err(), _err()
    d.all_unchanged("gt_anymal_reset hound")


# ================================================================================================== gt_measure_heights
@pytest.mark.parametrize("N,npts", H.HEIGHTS_SHAPES)
def test_measure_heights(N, npts):
    """Every probe farther than HEIGHTS_NEAR cells from an integer takes the float64 oracle's cell and exactly
    vs * min(...) in float32; the rest (at most 1 %) either neighbouring cell's value.  1, 420 and 259 elements: none
    a multiple of the 256-lane block."""
    samples, border, hs, vs, root, pts, kindp = H.heights_inputs(N, npts)
    rows, cols = samples.shape
    d = Dev()
    ps = [d.add(n, a) for n, a in (("samples", samples), ("root", root), ("pts", pts))]
    out = d.add("heights", np.full((N, npts), NAN, F32))
    rc = _lib().gt_measure_heights(ps[0], rows, cols, border, hs, vs, ps[1], ps[2], N, npts, out, None)
    _sync()
    what = f"measure_heights N={N} points={npts}"
    assert rc == 0, (what, _err())
    ix, iy, h64, cells = O.measure_heights(samples, border, hs, vs, root, pts)
    near = np.abs(cells - np.round(cells)).min(-1) < H.HEIGHTS_NEAR
    assert near.mean() <= 0.01
    got = d.get("heights")

    def value(i, j):
        i, j = np.clip(i, 0, rows - 2), np.clip(j, 0, cols - 2)
        return np.minimum(samples[i, j], samples[i + 1, j + 1]).astype(F32) * F32(vs)

    want = value(ix, iy)
    bad = (got != want) & ~near
    print(f"[task] {what}: {int((got != want).sum())} of {got.size} probes off the float64 cell, {int(near.sum())} near a cell edge")
    assert not bad.any(), (what, np.argwhere(bad)[:8].tolist())
    for e, k in np.argwhere((got != want) & near):
        fx, fy = int(np.floor(cells[e, k, 0])), int(np.floor(cells[e, k, 1]))
        nbrs = {float(value(np.int64(i), np.int64(j))) for i in (fx - 1, fx, fx + 1) for j in (fy - 1, fy, fy + 1)}
        assert float(got[e, k]) in nbrs, (what, e, k)
    if N * npts >= 7:  # off-map probes land in cells 0 and rows - 2 / cols - 2 (the samples are distinct: the value tells)
        assert (ix[kindp == 2] == 0).all() and (ix[kindp == 3] == rows - 2).all()
        assert (iy[kindp == 4] == 0).all() and (iy[kindp == 5] == cols - 2).all()
    d.unchanged(("samples", "root", "pts"), what)
