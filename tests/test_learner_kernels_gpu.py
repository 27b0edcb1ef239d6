"""rl_rms_normalize(_h), rl_opt_step(_h), rl_policy_kl / rl_policy_kl_step / rl_adaptive_lr, rl_act_heads /
rl_policy_head and rl_colsum_accum at the C ABI against the float64 references of the same statements
(oracle/learner_oracle.py), on the inputs of tests/helpers.py (what is claimed of them is asserted on the CPU in
tests/test_learner_oracle.py), at the smallest shapes that reach each branch of each kernel.

Every real-valued output field is judged by the rule of tests/test_ppo_loss_gpu.py (tests/helpers.py field_check):
    max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|
ref32 being the same reference in float32 on the CPU.  The running moments are float64 outputs under the same rule:
the kernel rounds the batch moments to float32 by design and ref32 does the same.  rl_rms_normalize's fields are
judged whole and, so that the mean-1e4 column's magnitude does not set the floor of the others, once more per column
kind (unit scale, mean 1e4, scale 1e-4, constant, outliers: tests/helpers.py RMS_KINDS).  A kind is a few columns,
and a column's error is one draw of the rounding of its batch mean (every y of the column moves with it), so the
per-kind err_f32 is the largest over the inputs of seeds 0..15 of the shape, as for one-number outputs.  The optimizer is judged on m, v and the step
p_new - p_old taken in float64 from the stored f32 values, never on p_new, whose ulp is hundreds of times the step.
A one-number output (kl) takes err_f32 as the largest |ref32 - ref64| over seeds 0..15 of its shape.  Every step of
a sequence is judged as a function of its stated inputs: the references start from the state the kernel left.
Beyond the rule: counts, steps, scales and learning rates exact; repeated calls the same bits; NaN guards behind
every output and every scratch buffer of exactly its documented size intact; refusals nonzero, named, and silent.

MEASURED on an MI355X: the largest err_kernel / err_f32 per field over all cases, and in brackets the largest
err_kernel / bar (<= 1 passes).
    rms mean 1.0 [0.52]   per kind: unit 1.8 [0.24]  offset 0.38 [0.05]  small 2.3 [0.32]  constant exact  outlier 2.5 [0.63]
    rms var 1.5 [0.10]    per kind: unit 1.7 [0.11]  offset 0.37 [0.06]  small 2.0 [0.06]  constant exact  outlier 1.4 [0.09]
    rms y 1.5 [0.25]      per kind: unit 0.99 [0.12]  offset 1.0 [0.25]  small 1.0 [0.12]  constant 1.0 [0.25]  outlier 1.3 [0.01]
    opt p_new - p_old 1.1 [0.27]   m 2.9 [0.24]   v 4.6 [0.34]
    kl far 1.0 [0.25]   near 0.78 [0.20]   same 0.46 [0.12]   the sigma written back 1.0 [0.07]
    heads mu 1.0 [0.09]  actions 1.0 [0.09]  sigmas 1.1 [0.06]  neglogp 1.7 [0.19]  value 1.1 [0.15]
    heads, logstd = -5 and |mu| ~ 1e3: mu 1.0 [0.05]  actions 1.0 [0.08]  sigmas 1.0 [0.0002]  neglogp 1.0 [0.25]  value 1.0 [0.17]
    rl_policy_head on the same mu and value: the same figures (bit-identical outputs)
    colsum grad 1.7 [0.26]

What the tests found.  With k_rms_part as it was (a float32 Welford pass over each block of 64 rows) the running
variance of the mean-1e4 columns missed the bar from the count = 100 state: 6.4e-05 against a bar of 5.4e-06 at 4097 x 7
(52 x err_f32, 11.9 x the bar) and 2.5e-04 against 6.3e-05 at 1000 x 255 (16 x, 4.0 x): a float32 running mean at 1e4
moves in steps of 1e-3, a thousandth of the deviations it is subtracted from.  The block sums are now float64 sums of
x - x[0][c] (csrc/rl_rms.hip); every other kernel was inside its bar as it stood.

Deliberate mutations, each built into a scratch copy of the library and run against this module (the tests that
failed, and the largest err_kernel / bar among the fields beyond it):
    k_rms_fin's variance with the biased divisor N: 12 of test_rms_update_matches_float64_reference (every init and
        count = 100 case with rows > 1) and test_rms_three_successive_updates; var 5.5e5, var[unit] 3.4e5, y 2.5e5
    the merge without its na nb / tot factor: the same 13 tests; var 5.5e5, var[outlier] 4.5e5, var[offset] 3.1e3, y 1.6e5
    Adam's eps inside the square root: all 40 of test_opt_step_matches_float64_reference; p_new - p_old 1.0e6
    bc2 without its square root: the same 40; p_new - p_old 1.3e6
    the KL's log without its 1e-5: all 30 of test_policy_kl_matches_float64_reference and all 8 of
        test_policy_kl_near_the_old_policy; kl far 624, near 226, same 171
    the heads' remainder loop skipped: the 16 cases of test_act_heads_match_float64_reference with H % 4 != 0; mu 1.5e6,
        value 2.3e6
    the column sum's row loop stepping row_lanes + 1: the 22017 x 24 and 130 x 2048 cases of
        test_colsum_accum_matches_float64_reference, fp16 and f32; grad 8.6e5 (below 21761 rows a 24-column call never
        takes the loop twice, so the 16385-row case alone would not have seen it)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import learner_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
F16, F32, F64 = torch.float16, torch.float32, torch.float64
EPS = 1e-5
SEEN = {}  # field -> [largest err_kernel / err_f32, largest err_kernel / bar] of this run


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for f, (r32, rbar) in sorted(SEEN.items()):
        print(f"[learner ratios] {f}: err_kernel / err_f32 <= {r32:.3g}, err_kernel / bar <= {rbar:.3g}")


def _lib():
    from isaacgymenv_amd.rl import gae
    return gae.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().rl_last_error().decode()


def _guarded(n, dtype=F32, init=None):
    """(buffer of n + GUARD elements filled with NaN, its first n, set to `init` if given)."""
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    if init is not None:
        buf[:n] = torch.as_tensor(init, dtype=dtype).reshape(-1).to(DEV)
    return buf, buf[:n]


def _tail_intact(bufs, what):
    for k, (buf, view) in bufs.items():
        assert bool(torch.isnan(buf[view.numel():]).all()), f"{what}: {k} written past its {view.numel()} elements"


def _untouched(bufs, what):
    for k, (buf, _) in bufs.items():
        assert bool(torch.isnan(buf).all()), f"{what}: wrote {k}"


_np, _bits, _same_bits = H.np64, H.bits, H.same_bits  # shared with the other float64-referenced kernel modules


def _field(fails, what, field, got, r64, r32, err_32=None):
    H.field_check("learner", SEEN, fails, what, field, _np(got), _np(r64), _np(r32), err_32=err_32)


# ===================================================================================================== rl_rms_normalize
def _rms_call(x_dev, rows, cols, state, update, half=False, with_partials=True):
    """One rl_rms_normalize(_h) call from `state` = (mean, var, count); every buffer NaN-guarded, partials exactly
    ceil(rows / 64) * cols * 2.  Returns (rc, bufs)."""
    L = _lib()
    bufs = dict(mean=_guarded(cols, F64, state[0]), var=_guarded(cols, F64, state[1]),
                count=_guarded(1, F64, [state[2]]), y=_guarded(rows * cols, F16 if half else F32))
    if with_partials:
        bufs["partials"] = _guarded(((rows + 63) // 64) * cols * 2)
    fn = L.rl_rms_normalize_h if half else L.rl_rms_normalize
    rc = fn(x_dev.data_ptr(), rows, cols, bufs["mean"][1].data_ptr(), bufs["var"][1].data_ptr(),
            bufs["count"][1].data_ptr(), EPS, update, bufs["partials"][1].data_ptr() if with_partials else None,
            bufs["y"][1].data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, bufs


def _rms_kind_fields(x, r, update):
    """{field: float64 array} of one reference result, per column kind: mean / var (update only) and y."""
    kinds, out = H.rms_kinds(x.shape[1]), {}
    for k, name in enumerate(H.RMS_KINDS):
        sel = torch.from_numpy(kinds == k)
        if bool(sel.any()):
            if update:
                out[f"rms mean[{name}]"], out[f"rms var[{name}]"] = _np(r[0][sel]), _np(r[1][sel])
            out[f"rms y[{name}]"] = _np(r[3][:, sel])
    return out


def _rms_worst(rows, cols, state, update):
    """{per-kind field: the largest |ref32 - ref64| over the inputs of seeds 0..15 of this shape from `state`}."""
    worst = {}
    for seed in range(16):
        x = H.rms_input(rows, cols, seed=seed)
        f64 = _rms_kind_fields(x, O.rms_normalize(x, *state, EPS, update), update)
        f32 = _rms_kind_fields(x, O.rms_normalize(x, *state, EPS, update, dtype=F32), update)
        for f in f64:
            worst[f] = max(worst.get(f, 0.0), float(np.abs(f32[f] - f64[f]).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _rms_worst_named(rows, cols, which, update):
    return _rms_worst(rows, cols, _rms_state(cols, which), update)


def _rms_judge(fails, what, x, state, update, bufs, worst):
    """The moments, the count and y of one call against the two references from the same state: each field whole,
    and per column kind with err_f32 over seeds 0..15 (`worst`; this input's own draw included)."""
    rows, cols = x.shape
    r64 = O.rms_normalize(x, *state, EPS, update)
    r32 = O.rms_normalize(x, *state, EPS, update, dtype=F32)
    mean, var, y = (bufs[k][1].cpu() for k in ("mean", "var", "y"))
    assert float(bufs["count"][1][0]) == r64[2], f"{what}: count {float(bufs['count'][1][0])} != {r64[2]}"
    if not update:
        assert _same_bits(mean, state[0]) and _same_bits(var, state[1]), f"{what}: eval changed the moments"
    y = y.reshape(rows, cols)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 5.0, f"{what}: y outside [-5, 5]"
    raw = (x.double() - r64[0]) / (r64[1] + EPS).sqrt()
    decided = raw.abs() > 5.0 + H.RMS_CLAMP_MARGIN
    assert torch.equal(y.double()[decided], 5.0 * raw[decided].sign()), f"{what}: y past the clamp is not exactly +-5"
    if update:
        _field(fails, what, "rms mean", mean, r64[0], r32[0])
        _field(fails, what, "rms var", var, r64[1], r32[1])
    _field(fails, what, "rms y", y, r64[3], r32[3])
    got, f64, f32 = (_rms_kind_fields(x, r, update) for r in ((mean, var, None, y), r64, r32))
    for f in f64:
        own = float(np.abs(f32[f] - f64[f]).max())
        _field(fails, what, f, got[f], f64[f], f32[f], err_32=max(own, worst[f]))
    return r64


def _rms_state(cols, which):
    if which == "init":
        return torch.zeros(cols, dtype=F64), torch.ones(cols, dtype=F64), 1.0
    return H.rms_state(cols, float(which.split()[1]))  # "count 100", "count 1e9": moments of the columns' own scale


@pytest.mark.parametrize("which", ["init", "count 100", "count 1e9"])
@pytest.mark.parametrize("rows,cols", H.RMS_SHAPES)
def test_rms_update_matches_float64_reference(rows, cols, which):
    """One train-mode call per shape (1 and 65 row blocks, a last block of one row, rows == 1, cols 1 .. 256), from
    the module's initial state, from a state with count 1e9, and from one with count 100 whose moments are of each
    column's own scale (there the batch moments carry most of the weight and no prior variance of 1 hides the 1e-4
    column's): moments, exact count, y, the clamp, the same bits from a second call, and the fp16 variant: the same
    moments and fp16(y) bit for bit."""
    x = H.rms_input(rows, cols, seed=rows % 16)
    state = _rms_state(cols, which)
    xd = x.to(DEV)
    what = f"rms rows={rows} cols={cols} {which}"
    fails = []
    rc, bufs = _rms_call(xd, rows, cols, state, 1)
    assert rc == 0, _err()
    _tail_intact(bufs, what)
    _rms_judge(fails, what, x, state, 1, bufs, _rms_worst_named(rows, cols, which, 1))
    rc, again = _rms_call(xd, rows, cols, state, 1)
    rc_h, half = _rms_call(xd, rows, cols, state, 1, half=True)
    assert rc == 0 and rc_h == 0, _err()
    _tail_intact(half, what + " fp16")
    for k in ("mean", "var", "count", "y"):
        assert _same_bits(again[k][1], bufs[k][1]), f"{what}: {k} differs between calls"
    for k in ("mean", "var", "count"):
        assert _same_bits(half[k][1], bufs[k][1]), f"{what}: {k} differs in the fp16 variant"
    assert _same_bits(half["y"][1], bufs["y"][1].to(F16)), f"{what}: the fp16 y is not the rounded f32 y"
    assert not fails, "\n".join(fails)


def test_rms_three_successive_updates():
    """130, 1 and 4097 rows in turn from the initial state; each update judged from the state the kernel left."""
    cols, fails = 10, []
    state = _rms_state(cols, "init")
    for k, rows in enumerate((130, 1, 4097)):
        x = H.rms_input(rows, cols, seed=100 + k)
        what = f"rms successive update {k} rows={rows}"
        rc, bufs = _rms_call(x.to(DEV), rows, cols, state, 1)
        assert rc == 0, _err()
        _tail_intact(bufs, what)
        _rms_judge(fails, what, x, state, 1, bufs, _rms_worst(rows, cols, state, 1))
        state = (bufs["mean"][1].cpu().clone(), bufs["var"][1].cpu().clone(), float(bufs["count"][1][0]))
    assert state[2] == 1.0 + 130 + 1 + 4097
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows,cols", H.RMS_SHAPES)
def test_rms_eval_path(rows, cols):
    """update = 0: y from the given moments, which stay untouched with the count; no partials (a null pointer)."""
    x = H.rms_input(rows, cols, seed=rows % 16)
    state = _rms_state(cols, "count 1e9")
    what = f"rms eval rows={rows} cols={cols}"
    fails = []
    rc, bufs = _rms_call(x.to(DEV), rows, cols, state, 0, with_partials=False)
    assert rc == 0, _err()
    _tail_intact(bufs, what)
    _rms_judge(fails, what, x, state, 0, bufs, _rms_worst_named(rows, cols, "count 1e9", 0))
    rc, half = _rms_call(x.to(DEV), rows, cols, state, 0, half=True, with_partials=False)
    assert rc == 0 and _same_bits(half["y"][1], bufs["y"][1].to(F16))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("half", [False, True])
def test_rms_refusals(half):
    """cols = 257 and rows = 0: nonzero, named, and nothing written (buffers sized for the larger shape)."""
    L = _lib()
    x = torch.zeros(4 * 257, device=DEV)
    fn = L.rl_rms_normalize_h if half else L.rl_rms_normalize
    for rows, cols in ((4, 257), (0, 8)):
        bufs = dict(mean=_guarded(257, F64), var=_guarded(257, F64), count=_guarded(1, F64),
                    y=_guarded(4 * 257, F16 if half else F32), partials=_guarded(2 * 257))
        rc = fn(x.data_ptr(), rows, cols, bufs["mean"][1].data_ptr(), bufs["var"][1].data_ptr(),
                bufs["count"][1].data_ptr(), EPS, 1, bufs["partials"][1].data_ptr(), bufs["y"][1].data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"rl_rms_normalize" in L.rl_last_error(), (rows, cols)
        _untouched(bufs, f"rms rows={rows} cols={cols}")


# ========================================================================================================== rl_opt_step
OPT_N = (1, 255, 256, 257, 65537)  # 257: slices of 2, workgroups 129.. empty; 65537: slices of 257 > 256 threads
# (loss scaling, clip binding, weight decay)
OPT_CONFIGS = {"scaler, clip binds": (True, True, 0.0), "no scaler, clip loose, decay": (False, False, 1e-2),
               "scaler, clip loose, decay": (True, False, 1e-2), "no scaler, clip binds": (False, True, 0.0)}
OPT_LR = 3e-4


def _hyper_struct(h):
    from isaacgymenv_amd.rl import gae
    return gae.OptHyper(h["max_norm"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["backoff"], h["growth"],
                        h["growth_interval"])


class _OptDevice:
    """Device state of one optimizer: p, m, v (and the fp16 shadow) NaN-guarded, the scalars, the partials at exactly
    rl_opt_partials_size() (zeroed once: rl_opt_step_h's counter word)."""

    def __init__(self, n, p, m, v, step, scale, tracker, half):
        L = _lib()
        self.n, self.half = n, half
        self.bufs = dict(p=_guarded(n, F32, p), m=_guarded(n, F32, m), v=_guarded(n, F32, v),
                         partials=_guarded(L.rl_opt_partials_size(), F32, torch.zeros(L.rl_opt_partials_size())))
        if half:
            self.bufs["phalf"] = _guarded(n, F16, torch.as_tensor(p).to(F16))
        self.step = torch.tensor(float(step), device=DEV)
        self.lr = torch.tensor(OPT_LR, device=DEV)
        self.scale = None if scale is None else torch.tensor(float(scale), device=DEV)
        self.tracker = None if scale is None else torch.tensor(int(tracker), dtype=torch.int32, device=DEV)

    def call(self, g_dev, hyper):
        L = _lib()
        b = self.bufs
        hs = _hyper_struct(hyper)
        sc = None if self.scale is None else self.scale.data_ptr()
        tr = None if self.tracker is None else self.tracker.data_ptr()
        if self.half:
            rc = L.rl_opt_step_h(b["p"][1].data_ptr(), b["phalf"][1].data_ptr(), g_dev.data_ptr(), b["m"][1].data_ptr(),
                                 b["v"][1].data_ptr(), self.n, self.step.data_ptr(), self.lr.data_ptr(), sc, tr,
                                 ctypes.byref(hs), b["partials"][1].data_ptr(), _stream())
        else:
            rc = L.rl_opt_step(b["p"][1].data_ptr(), g_dev.data_ptr(), b["m"][1].data_ptr(), b["v"][1].data_ptr(), self.n,
                               self.step.data_ptr(), self.lr.data_ptr(), sc, tr, ctypes.byref(hs),
                               b["partials"][1].data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, _err()
        _tail_intact(b, f"opt n={self.n} half={self.half}")
        if self.half:
            assert int(_bits(b["partials"][1][-1:])[0]) == 0, "rl_opt_step_h left its counter word nonzero"

    def state(self):
        b = self.bufs
        return dict(p=b["p"][1].cpu().clone(), m=b["m"][1].cpu().clone(), v=b["v"][1].cpu().clone(),
                    step=float(self.step), scale=None if self.scale is None else float(self.scale),
                    tracker=None if self.tracker is None else int(self.tracker))


def _opt_sequence(n, step0, steps, scaler, binds, wd):
    scale0 = 1024.0 if scaler else None
    grads = [H.opt_grad(n, seed=10 * n % 997 + k, scale=scale0) for k in range(steps)]
    norms = [float(g.double().norm()) / (scale0 or 1.0) for g in grads]
    # the clip threshold from the gradients themselves: half the smallest norm binds on every step, twice the
    # largest on none
    hyper = dict(O.OPT_HYPER, max_norm=0.5 * min(norms) if binds else 2.0 * max(norms), weight_decay=wd, growth_interval=3)
    return scale0, grads, hyper


@pytest.mark.parametrize("config", list(OPT_CONFIGS))
@pytest.mark.parametrize("step0,steps", [(0, 4), (1000, 2)])
@pytest.mark.parametrize("n", OPT_N)
def test_opt_step_matches_float64_reference(n, step0, steps, config):
    """Consecutive steps of rl_opt_step and rl_opt_step_h side by side: m, v and the step p_new - p_old of each call
    against the references from the state the kernel had; step, scale and tracker exact (the tracker starts at 1
    with a growth interval of 3: the scale doubles on the second call); rl_opt_step_h bit-identical in p, m, v with
    param_half = fp16(p) and its counter word back at zero after every call."""
    scaler, binds, wd = OPT_CONFIGS[config]
    scale0, grads, hyper = _opt_sequence(n, step0, steps, scaler, binds, wd)
    p, m, v = H.opt_state(n, step0, seed=n)
    plain = _OptDevice(n, p, m, v, step0, scale0, 1, half=False)
    shadow = _OptDevice(n, p, m, v, step0, scale0, 1, half=True)
    fails = []
    for k, g in enumerate(grads):
        what = f"opt n={n} step={step0 + k} {config}"
        before = plain.state()
        gd = g.to(DEV)
        plain.call(gd, hyper)
        shadow.call(gd, hyper)
        after, after_h = plain.state(), shadow.state()
        args = (before["p"], g, before["m"], before["v"], before["step"], OPT_LR, before["scale"], before["tracker"], hyper)
        r64, r32 = O.opt_step(*args), O.opt_step(*args, dtype=F32)
        assert not r64[6] and (after["step"], after["scale"], after["tracker"]) == r64[3:6], \
            f"{what}: step / scale / tracker {(after['step'], after['scale'], after['tracker'])} != {r64[3:6]}"
        p0 = before["p"].double()
        _field(fails, what, "opt p_new - p_old", after["p"].double() - p0, r64[0] - p0, r32[0].double() - p0)
        _field(fails, what, "opt m", after["m"], r64[1], r32[1])
        _field(fails, what, "opt v", after["v"], r64[2], r32[2])
        for f in ("p", "m", "v"):
            assert _same_bits(after_h[f], after[f]), f"{what}: rl_opt_step_h differs in {f}"
        assert (after_h["step"], after_h["scale"], after_h["tracker"]) == (after["step"], after["scale"], after["tracker"])
        assert _same_bits(shadow.bufs["phalf"][1], after["p"].to(F16)), f"{what}: param_half is not fp16(p)"
    if scaler:
        assert after["scale"] == 2048.0  # grown once, at the second call
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("scaler", [True, False])
@pytest.mark.parametrize("n", [255, 257, 65537])
def test_opt_step_non_finite_gradient(n, scaler, half):
    """inf at the first element, NaN at the last, inf at the first element of the last non-empty slice.  With the
    scaler: p, m, v, step (and param_half) keep their bits, the scale backs off, the tracker restarts.  Without: the
    step is taken, and what became non-finite is what the reference says."""
    chunk = (n + 255) // 256
    places = [(0, float("inf")), (n - 1, float("nan")), (((n - 1) // chunk) * chunk, float("-inf"))]
    hyper = dict(O.OPT_HYPER)
    p, m, v = H.opt_state(n, 1000, seed=n)
    for at, bad in places:
        what = f"opt n={n} non-finite at {at} scaler={scaler} half={half}"
        g = H.opt_grad(n, seed=at, scale=1024.0 if scaler else None)
        g[at] = bad
        dev = _OptDevice(n, p, m, v, 1000, 1024.0 if scaler else None, 5, half)
        before_half = dev.bufs["phalf"][1].clone() if half else None
        dev.call(g.to(DEV), hyper)
        after = dev.state()
        r64 = O.opt_step(p, g, m, v, 1000.0, OPT_LR, 1024.0 if scaler else None, 5 if scaler else None, hyper)
        assert r64[6] and (after["step"], after["scale"], after["tracker"]) == r64[3:6], what
        if scaler:
            assert (after["step"], after["scale"], after["tracker"]) == (1000.0, 512.0, 0), what
            for f, old in (("p", p), ("m", m), ("v", v)):
                assert _same_bits(after[f], old), f"{what}: {f} changed on a skipped step"
            if half:
                assert _same_bits(dev.bufs["phalf"][1], before_half), f"{what}: param_half changed on a skipped step"
        else:
            assert after["step"] == 1001.0, what
            for f, ref in (("p", r64[0]), ("m", r64[1]), ("v", r64[2])):
                assert torch.equal(torch.isfinite(after[f]), torch.isfinite(ref)), f"{what}: non-finite pattern of {f}"
            assert not bool(torch.isfinite(after["p"][at]))


# ============================================================================================ rl_policy_kl and the scheduler
@functools.lru_cache(maxsize=None)
def _kl_refs(M, A, kind, mode, half):
    """(inputs of seed 0, its ref64 kl, its ref32 kl, the largest |ref32 - ref64| over seeds 0..15 of this shape)."""
    worst, first = 0.0, None
    for seed in range(16):
        d = H.kl_inputs(M, A, kind, mode, half, seed=seed)
        args = (d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], d["sigma_is_log"])
        r64, r32 = float(O.policy_kl(*args)), float(O.policy_kl(*args, dtype=F32))
        worst = max(worst, abs(r32 - r64))
        if seed == 0:
            first = (d, r64, r32)
    return (*first, worst)


class _KlDevice:
    def __init__(self, d):
        L = _lib()
        self.d = d
        self.M, self.A = d["mu_old"].shape
        self.mu_new, self.sigma_new = d["mu_new"].to(DEV), d["sigma_new"].to(DEV)
        n = self.M * self.A
        self.bufs = dict(mu_old=_guarded(n, F32, d["mu_old"]), sigma_old=_guarded(n, F32, d["sigma_old"]), kl=_guarded(1),
                         partials=_guarded(L.rl_kl_partials_size(), F32, torch.zeros(L.rl_kl_partials_size())))
        self.lr = torch.tensor(0.0, dtype=F64, device=DEV)
        self.opt_lr = torch.tensor(0.0, device=DEV)
        self.stats = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV)
        self.losses = torch.tensor([0.25, 0.5, 0.125], device=DEV)

    def _common(self, write_back):
        b, d = self.bufs, self.d
        return (self.mu_new.data_ptr(), int(self.mu_new.dtype == F16), self.sigma_new.data_ptr(), d["sigma_row_stride"],
                d["sigma_is_log"], b["mu_old"][1].data_ptr(), b["sigma_old"][1].data_ptr(), self.M, self.A, int(write_back),
                b["kl"][1].data_ptr(), b["partials"][1].data_ptr())

    def _losses(self):
        return tuple(self.losses[i:i + 1].data_ptr() for i in range(3))

    def kl(self, write_back=0):
        rc = _lib().rl_policy_kl(*self._common(write_back), _stream())
        torch.cuda.synchronize()
        assert rc == 0, _err()
        _tail_intact(self.bufs, "rl_policy_kl")
        return self.bufs["kl"][1].cpu().clone()

    def lr_step(self, thr, lr, inv_world=1.0, adaptive=1):
        self.lr.fill_(lr)
        self.opt_lr.fill_(0.0)
        rc = _lib().rl_adaptive_lr(self.bufs["kl"][1].data_ptr(), inv_world, adaptive, thr, self.lr.data_ptr(),
                                   self.opt_lr.data_ptr(), self.stats.data_ptr(), *self._losses(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, _err()

    def kl_step(self, thr, lr, write_back=0, adaptive=1):
        self.lr.fill_(lr)
        self.opt_lr.fill_(0.0)
        rc = _lib().rl_policy_kl_step(*self._common(write_back), adaptive, thr, self.lr.data_ptr(), self.opt_lr.data_ptr(),
                                      self.stats.data_ptr(), *self._losses(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, _err()
        _tail_intact(self.bufs, "rl_policy_kl_step")
        assert int(_bits(self.bufs["partials"][1][-1:])[0]) == 0, "rl_policy_kl_step left its counter word nonzero"
        return self.bufs["kl"][1].cpu().clone()

    def scheduler(self):
        return float(self.lr), self.opt_lr.cpu().clone(), self.stats.cpu().clone()


def _kl_case(M, A, kind, mode, half, fails):
    d, r64, r32, worst = _kl_refs(M, A, kind, mode, half)
    what = f"kl M={M} A={A} {kind} sigma={mode} mu={'f16' if half else 'f32'}"
    dev = _KlDevice(d)
    kl = dev.kl(0)
    _field(fails, what, f"kl {kind}", kl, [r64], [r32], err_32=worst)
    assert _same_bits(dev.bufs["mu_old"][1], d["mu_old"].reshape(-1)) and \
        _same_bits(dev.bufs["sigma_old"][1], d["sigma_old"].reshape(-1)), f"{what}: write_back = 0 changed the old tensors"
    assert _same_bits(dev.kl(0), kl), f"{what}: kl differs between calls"
    return d, r64, dev, kl, what


@pytest.mark.parametrize("mode", H.KL_SIGMA_MODES)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M,A", H.KL_SHAPES)
def test_policy_kl_matches_float64_reference(M, A, half, mode):
    """kl on every shape (M = 1; 255 / 257: trailing workgroups empty; 65537: 257 rows a workgroup), mu dtype and
    sigma layout; the old tensors untouched without write_back and bit for bit the new ones with it; the one-launch
    rl_policy_kl_step bit-identical to rl_policy_kl + rl_adaptive_lr in kl, lr, opt_lr and stats over three calls
    on one partials buffer; lr exact in every scheduler case, both clamps included."""
    fails = []
    d, r64, dev, kl, what = _kl_case(M, A, "far", mode, half, fails)
    for thr, lr, want in H.kl_scheduler_cases(r64)[:3]:  # three launches of each on one partials buffer
        dev.stats.copy_(torch.tensor([1.0, 2.0, 3.0, 4.0]))
        assert _same_bits(dev.kl(0), kl)
        dev.lr_step(thr, lr)
        two = dev.scheduler()
        dev.stats.copy_(torch.tensor([1.0, 2.0, 3.0, 4.0]))
        assert _same_bits(dev.kl_step(thr, lr), kl), f"{what}: rl_policy_kl_step's kl differs"
        one = dev.scheduler()
        assert two[0] == want and one[0] == want, f"{what}: lr {two[0]} / {one[0]}, expected {want}"
        assert float(two[1]) == float(np.float32(want)) and _same_bits(one[1], two[1])
        assert _same_bits(one[2], two[2]), f"{what}: stats differ"
        exp = torch.tensor([1.0, 2.0, 3.0, 4.0]) + torch.stack([dev.losses[0].cpu(), dev.losses[1].cpu(), kl[0], dev.losses[2].cpu()])
        assert _same_bits(two[2], exp), f"{what}: stats {two[2].tolist()} != {exp.tolist()}"
    for thr, lr, want in H.kl_scheduler_cases(r64)[3:]:  # the clamps
        dev.kl(0)
        dev.lr_step(thr, lr)
        assert dev.scheduler()[0] == want, f"{what}: lr at the clamp"
    # write_back, by both entry points
    for step in (False, True):
        dev = _KlDevice(d)
        got = dev.kl_step(r64, 3e-4, write_back=1) if step else dev.kl(1)
        assert _same_bits(got, kl), f"{what}: kl with write_back differs"
        mo, so = dev.bufs["mu_old"][1].cpu().reshape(M, A), dev.bufs["sigma_old"][1].cpu().reshape(M, A)
        assert _same_bits(mo, d["mu_new"].float()), f"{what}: mu_old is not the new mu"
        if mode == "log":  # s0 = exp(log sigma) on the device: the same row everywhere, judged as a field
            assert _same_bits(so, so[:1].expand(M, A)), f"{what}: sigma_old rows differ"
            ls = d["sigma_new"]
            _field(fails, what, "kl sigma written back", so[0], ls.double().exp(), ls.exp())
        else:
            assert _same_bits(so, d["sigma_new"].expand(M, A)), f"{what}: sigma_old is not the new sigma"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ["near", "same"])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M,A", [(257, 12), (65537, 2)])
def test_policy_kl_near_the_old_policy(M, A, half, kind):
    """mu_old = mu_new + 1e-3 noise, and mu_old == mu_new exactly, with equal sigmas: every term a cancellation
    against 0.5, the KL of the order of the two 1e-5 terms."""
    fails = []
    for mode in ("log", "row"):
        d, r64, dev, kl, what = _kl_case(M, A, kind, mode, half, fails)
        assert _same_bits(dev.kl_step(1.0, 3e-4, adaptive=0), kl), f"{what}: rl_policy_kl_step's kl differs"
        assert dev.scheduler()[0] == 3e-4  # not adaptive: lr untouched
    assert not fails, "\n".join(fails)


def test_adaptive_lr_rank_average():
    """kl * inv_world in f32, then the scheduler on the product."""
    d, r64, _, _ = _kl_refs(255, 12, "far", "log", False)
    dev = _KlDevice(d)
    kl = dev.kl(0)
    dev.bufs["kl"][1].mul_(4.0)
    dev.lr_step(r64 * 4, 3e-4, inv_world=0.25)
    want_kl, want_lr = O.adaptive_lr(float(kl[0]) * 4.0, 0.25, 1, r64 * 4, 3e-4)
    assert float(dev.bufs["kl"][1][0]) == want_kl and dev.scheduler()[0] == want_lr == 3e-4 * 1.5


# ========================================================================================= rl_act_heads, rl_policy_head
HEAD_OUT = ("mu", "actions", "sigmas", "neglogp", "value")


def _heads_call(dev, N, Hd, A, vnorm, ld=None, check=True):
    L = _lib()
    ld = 2 * Hd + 4 if ld is None else ld
    bufs = dict(mu=_guarded(N * A), actions=_guarded(N * A), sigmas=_guarded(N * A), neglogp=_guarded(N), value=_guarded(N))
    hid = dev["hidden"]
    rc = L.rl_act_heads(hid.data_ptr(), ld, hid.data_ptr() + 4 * Hd, ld, Hd, dev["w_mu"].data_ptr(), dev["b_mu"].data_ptr(),
                        dev["w_v"].data_ptr(), dev["b_v"].data_ptr(), dev["noise"].data_ptr(), dev["logstd"].data_ptr(),
                        dev["vmean"].data_ptr() if vnorm else None, dev["vvar"].data_ptr() if vnorm else None, EPS, N, A,
                        *[bufs[k][1].data_ptr() for k in HEAD_OUT], _stream())
    torch.cuda.synchronize()
    if check:
        assert rc == 0, _err()
        _tail_intact(bufs, "rl_act_heads")
    return rc, bufs


def _head_call(dev, mu, value, N, A, vnorm):
    L = _lib()
    bufs = dict(actions=_guarded(N * A), sigmas=_guarded(N * A), neglogp=_guarded(N), value=_guarded(N))
    rc = L.rl_policy_head(mu.data_ptr(), dev["noise"].data_ptr(), dev["logstd"].data_ptr(), value.data_ptr(),
                          dev["vmean"].data_ptr() if vnorm else None, dev["vvar"].data_ptr() if vnorm else None, EPS, N, A,
                          *[bufs[k][1].data_ptr() for k in HEAD_OUT[1:]], _stream())
    torch.cuda.synchronize()
    assert rc == 0, _err()
    _tail_intact(bufs, "rl_policy_head")
    return bufs


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("vnorm", [False, True])
@pytest.mark.parametrize("N,Hd,A", H.ACT_HEADS_SHAPES)
def test_act_heads_match_float64_reference(N, Hd, A, vnorm, sharp):
    """Real-valued heads on strided hidden rows (ld = 2H + 4, the pad NaN): H % 4 != 0 (the remainder loop), N % 16
    != 0, A = 1, two workgroups (N = 17, 33), 55 KB of LDS (H = 130, A = 64); value normalisation on and off with raw
    values on both sides of +-5; sharp: logstd = -5 against |mu| ~ 1e3, where x - mu cancels.  Then rl_policy_head on
    the kernel's own mu and raw value: bit for bit rl_act_heads' outputs, and judged by the same rule."""
    d = H.act_heads_inputs(N, Hd, A, seed=N, sharp=sharp)
    dev = {k: v.to(DEV) for k, v in d.items()}
    ha, hc = d["hidden"][:, :Hd], d["hidden"][:, Hd:2 * Hd]
    vm = (d["vmean"], d["vvar"], EPS) if vnorm else (None, None, EPS)
    args = (ha, hc, d["w_mu"], d["b_mu"], d["w_v"], d["b_v"], d["noise"], d["logstd"], *vm)
    r64, r32 = O.act_heads(*args), O.act_heads(*args, dtype=F32)
    what = f"heads N={N} H={Hd} A={A} vnorm={int(vnorm)} sharp={int(sharp)}"
    fails = []
    _, bufs = _heads_call(dev, N, Hd, A, vnorm)
    for k in HEAD_OUT:
        _field(fails, what, f"heads {k}" + (" (sharp)" if sharp else ""), bufs[k][1], r64[k], r32[k])
    _, again = _heads_call(dev, N, Hd, A, vnorm)
    for k in HEAD_OUT:
        assert _same_bits(again[k][1], bufs[k][1]), f"{what}: {k} differs between calls"
    # rl_policy_head from the same mu and the raw value (rl_act_heads without the value normalisation returns it)
    _, raw = _heads_call(dev, N, Hd, A, False)
    head = _head_call(dev, bufs["mu"][1], raw["value"][1], N, A, vnorm)
    mu_k, v_k = bufs["mu"][1].cpu().reshape(N, A), raw["value"][1].cpu()
    p64 = O.policy_head(mu_k, v_k, d["noise"], d["logstd"], *vm)
    p32 = O.policy_head(mu_k, v_k, d["noise"], d["logstd"], *vm, dtype=F32)
    for k in HEAD_OUT[1:]:
        assert _same_bits(head[k][1], bufs[k][1]), f"{what}: rl_policy_head differs from rl_act_heads in {k}"
        _field(fails, what, f"head {k}" + (" (sharp)" if sharp else ""), head[k][1], p64[k], p32[k])
    assert not fails, "\n".join(fails)


def test_act_heads_refusals():
    """ld < H, and an LDS stage over the limit (H = 1024, A = 12): nonzero, named, nothing written."""
    N, Hd, A = 16, 1024, 12
    d = H.act_heads_inputs(N, Hd, A)
    dev = {k: v.to(DEV) for k, v in d.items()}
    rc, bufs = _heads_call(dev, N, Hd, A, True, check=False)
    assert rc != 0 and b"rl_act_heads" in _lib().rl_last_error() and b"LDS" in _lib().rl_last_error()
    _untouched(bufs, "LDS refusal")
    rc, bufs = _heads_call(dev, N, 128, A, True, ld=127, check=False)
    assert rc != 0 and b"rl_act_heads" in _lib().rl_last_error()
    _untouched(bufs, "ld < H")


# ====================================================================================================== rl_colsum_accum
def _colsum_call(g_dev, rows, cols, grad0, g_ptr=None, check=True):
    L = _lib()
    parts = min(256, (rows + 63) // 64)
    bufs = dict(work=_guarded(parts * cols))
    # the gradient at an odd float offset inside a larger buffer
    whole = torch.full((1 + cols + GUARD,), float("nan"), device=DEV)
    whole[1:1 + cols] = grad0.to(DEV)
    rc = L.rl_colsum_accum(g_ptr or g_dev.data_ptr(), rows, cols, int(g_dev.dtype == F16), whole[1:].data_ptr(),
                           bufs["work"][1].data_ptr(), _stream())
    torch.cuda.synchronize()
    if check:
        assert rc == 0, _err()
        _tail_intact(bufs, "rl_colsum_accum")
        assert bool(torch.isnan(whole[0])) and bool(torch.isnan(whole[1 + cols:]).all()), "written outside grad"
    return rc, whole, bufs


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 8), (63, 24), (65, 24), (16385, 24), (22017, 24), (130, 2048)])
def test_colsum_accum_matches_float64_reference(rows, cols, half):
    """cols = 24: three column vectors a row, 85 rows side by side and one idle thread; cols = 2048: one row at a
    time; rows = 1; 16385 rows: 256 partials of 65 rows (the last of 5); 22017 rows: partials of 87 rows, more than the
    85 side by side, so the first lanes take a second row (below 21761 rows no 24-column call gets there); accumulated
    onto a nonzero gradient at an odd float offset, the scratch at exactly parts * cols."""
    g, grad0 = H.colsum_inputs(rows, cols, half, seed=rows)
    gd = g.to(DEV)
    what = f"colsum rows={rows} cols={cols} {'f16' if half else 'f32'}"
    fails = []
    _, whole, _ = _colsum_call(gd, rows, cols, grad0)
    _field(fails, what, "colsum grad", whole[1:1 + cols], O.colsum(g, grad0), O.colsum(g, grad0, dtype=F32))
    _, again, _ = _colsum_call(gd, rows, cols, grad0)
    assert _same_bits(again[1:1 + cols], whole[1:1 + cols]), f"{what}: differs between calls"
    assert not fails, "\n".join(fails)


def test_colsum_accum_refusals():
    g, grad0 = H.colsum_inputs(8, 2056 + 8, False)
    gd = g.to(DEV)
    for name, cols, off in (("cols = 12", 12, 0), ("cols = 2056", 2056, 0), ("g not 16-byte aligned", 24, 4)):
        rc, whole, bufs = _colsum_call(gd, 8, cols, grad0[:cols], g_ptr=gd.data_ptr() + off, check=False)
        assert rc != 0 and b"rl_colsum_accum" in _lib().rl_last_error(), name
        _untouched(bufs, name)
        assert _same_bits(whole[1:1 + cols], grad0[:cols]) and bool(torch.isnan(whole[0])), f"{name}: grad written"
