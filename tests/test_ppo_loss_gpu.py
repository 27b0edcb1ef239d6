"""rl_ppo_loss, rl_ppo_loss_backward, rl_ppo_heads_loss and rl_ppo_heads_loss_backward (csrc/rl_ppo_loss.hip) at the
C ABI against the float64 reference of the same statements (oracle/ppo_oracle.py ppo_loss / ppo_heads_loss), on
minibatches that reach every branch of the loss on known rows (tests/helpers.py ppo_minibatch; the coverage and the
margins are asserted on the CPU in tests/test_ppo_loss_oracle.py).

Every output field is compared on its own:  max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|,  ref32
being the same reference run in float32 on the CPU (4x: the kernel's expf / logf and its reduction tree differ from
the CPU's, each worth about a factor of 2; the floor covers fields where the CPU's float32 happens to be exact).
The bar comes from the reference pair alone.  Elements the reference has at exactly 0 must be exactly 0 and no
other may be; repeated calls must give the same bits; nothing may be written past the stated sizes.

The backward of the heads starts, in the kernel and in both references, from ref64's loss gradients rounded to f32:
rl_ppo_heads_loss_backward is a function of the f32 gradients it is handed, and s = 1024 is a power of two, so
fp16(dmu s) is then the same number for all three (from the forward kernel's own dmu, an f32 rounding apart, the
fp16 rounding would flip on some elements and say nothing about the backward).

MEASURED on an MI355X: the largest err_kernel / err_f32 per field over all cases, and in brackets the largest
err_kernel / bar (<= 1 passes).  Ratios above 4 inside the bar are fields whose CPU float32 run is exact or nearly so:
the floor covers them.
    dmu 5.8 [0.48]   dvalues 1.0 [0.09]   dlogstd 15 [0.54]
    loss 80 [0.35]   stats: actor 1.0 [0.07]  critic 14.5 [0.24]  entropy 164 [0.23]  bound 16 [0.23]
    heads backward: dhidden actor 1.0 [0.22]  dhidden critic exact  grad_w_mu 12.8 [0.39]  grad_b_mu 8 [0.23]
    grad_w_v, grad_b_v, grad_logstd: ref32 exact, the kernel inside the floor [0.38, 0.15, 0.25]
With the fp16 rounding of mu +- 1.1 applied to f32 mu as well (k_ppo_rows as it was before these tests): stats[3] bound at
8.2e4 (rows = 129, A = 12, f32 / f32), the loss of every f32-mu case and dmu of the A = 1 ones beyond the bar.

The actor mean and the loss.  A mean is one number, so its err_f32 is one draw of the CPU's rounding error, not a
maximum over elements: over seeds 0..39 at rows = 385, A = 12 the float32 reference's own error in stats[0] runs
from 7.9e-10 to 1.4e-07.  The actor mean adds terms of both signs (|mean| 0.02 .. 0.04 against terms up to 4), so
the floor, relative to |mean|, gives it no cover either, and an f32 evaluation of it (the f32 rounding of neglogp,
17 .. 45, inside the ratio) lands beyond the bar whenever the CPU's draw is a lucky one: with the actor term in f32
the kernels measured stats[0] at 79 [1.75] and the loss at 277 [1.2], six cases beyond the bar.  The kernels
therefore evaluate the row's actor term and its sums in float64 (csrc/rl_ppo_loss.hip), which puts stats[0] within
a rounding of the float64 reference whatever the CPU's draw.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
E = H.PPO_E_CLIP
NAMES = H.PPO_INPUTS
COEF = dict(critic_coef=2.0, entropy_coef=1e-3, bounds_loss_coef=1e-2)
GUARD = 64
F16, F32 = torch.float16, torch.float32
SEEN = {}  # field -> [largest err_kernel / err_f32, largest err_kernel / bar] of this run


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for f, (r32, rbar) in sorted(SEEN.items()):
        print(f"[ppo-loss ratios] {f}: err_kernel / err_f32 <= {r32:.3g}, err_kernel / bar <= {rbar:.3g}")


def _lib():
    from isaacgymenv_amd.rl import gae
    return gae.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype=F32, fill=float("nan")):
    """(buffer of n + GUARD elements filled with `fill`, its first n)."""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _np(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _field(fails, what, field, got, r64, r32, zeros=False):
    """The rule of the module docstring for one field (tests/helpers.py field_check); its figures printed and kept
    for the report."""
    H.field_check("ppo-loss", SEEN, fails, what, field, got, r64, r32, zeros=zeros)


GRADS, MEANS = "gradients", "means"  # the two halves of the outputs, a test each


def _loss_fields(fails, what, out, r64, r32, which):
    """which = GRADS: d mu, d values, d logstd, each with its pattern of exact zeros; MEANS: the loss and stats[4]."""
    if which == MEANS:
        _field(fails, what, "loss", out["loss"], r64["loss"], r32["loss"])
        for k, name in enumerate(("actor", "critic", "entropy", "bound")):
            _field(fails, what, f"stats[{k}] {name}", out["stats"][k], r64["stats"][k], r32["stats"][k])
    else:
        for f in ("dmu", "dvalues", "dlogstd"):
            _field(fails, what, f, out[f], r64[f], r32[f], zeros=True)


@functools.lru_cache(maxsize=None)
def _loss_refs(B, A, mu16, v16, clip_value, bounds_loss_coef, seed):
    """(minibatch, ref64, ref32) of one case: computed once, shared by its tests, never changed."""
    mb = H.ppo_minibatch(B, A, seed=seed, mu_f16=bool(mu16), values_f16=bool(v16))
    args = [mb[k] for k in NAMES] + [E, clip_value, COEF["critic_coef"], COEF["entropy_coef"], bounds_loss_coef, bool(mu16)]
    return mb, O.ppo_loss(*args), O.ppo_loss(*args, dtype=F32)


def _run_loss(dev, B, A, clip_value, coef):
    """One rl_ppo_loss call on device inputs `dev`; every output with a NaN guard after it, partials exactly the
    size include/gymrl.h states.  Returns {name: (buffer, view)}."""
    sizes = dict(dmu=B * A, dvalues=B, partials=((B + 127) // 128) * 36, loss=1, stats=4, dlogstd=A)
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    L = _lib()
    rc = L.rl_ppo_loss(dev["mu"].data_ptr(), int(dev["mu"].dtype == F16), dev["values"].data_ptr(),
                       int(dev["values"].dtype == F16), *[dev[k].data_ptr() for k in NAMES[2:]], B, A, E, clip_value,
                       coef["critic_coef"], coef["entropy_coef"], coef["bounds_loss_coef"], p["dmu"], p["dvalues"],
                       p["partials"], p["loss"], p["stats"], p["dlogstd"], _stream())
    assert rc == 0, L.rl_last_error().decode()
    torch.cuda.synchronize()
    return bufs


def _guards_intact(bufs):
    for k, (buf, view) in bufs.items():
        tail = buf[view.numel():]
        assert bool(torch.isnan(tail).all()), f"{k}: written past its {view.numel()} elements"
        if k != "partials":
            assert bool(torch.isfinite(view).all()), f"{k}: not every element written"


def _out(bufs):
    return dict(loss=_np(bufs["loss"][1])[0], stats=_np(bufs["stats"][1]), dmu=_np(bufs["dmu"][1]),
                dvalues=_np(bufs["dvalues"][1]), dlogstd=_np(bufs["dlogstd"][1]))


# rows, A, mu fp16, values fp16, clip_value: every value of every parameter, every dtype pair at the aligned size
# (128) and at ragged ones, sum_partials' tail alone (< 4 blocks), its unrolled chains (35 blocks)
LOSS_CASES = [
    (1, 12, 1, 1, 1), (1, 32, 1, 0, 0),
    (127, 12, 1, 1, 1), (127, 1, 0, 0, 0),
    (128, 12, 1, 1, 1), (128, 12, 1, 0, 1), (128, 12, 0, 1, 0), (128, 32, 0, 0, 1),
    (129, 12, 1, 0, 1), (129, 32, 0, 1, 1), (129, 1, 1, 1, 0), (129, 12, 0, 0, 1),
    (385, 12, 0, 0, 0), (385, 32, 1, 1, 1), (385, 1, 0, 1, 1),
    (4357, 32, 1, 1, 1), (4357, 12, 0, 0, 1), (4357, 1, 1, 0, 0), (4357, 32, 0, 1, 0),
]


def _loss_case(B, A, mu16, v16, clip_value, which, fails, bounds_loss_coef=COEF["bounds_loss_coef"], seed=None,
               repeat=True):
    seed = B + A if seed is None else seed
    mb, r64, r32 = _loss_refs(B, A, mu16, v16, clip_value, bounds_loss_coef, seed)
    coef = dict(COEF, bounds_loss_coef=bounds_loss_coef)
    dev = {k: v.to(DEV) for k, v in mb.items()}
    bufs = _run_loss(dev, B, A, clip_value, coef)
    _guards_intact(bufs)
    what = f"loss rows={B} A={A} mu={'f16' if mu16 else 'f32'} v={'f16' if v16 else 'f32'} clip={clip_value} " \
           f"bc={bounds_loss_coef:g} seed={seed}"
    _loss_fields(fails, what, _out(bufs), r64, r32, which)
    if repeat:  # the fixed-order sums: the same bits from every call
        for _ in range(2):
            again = _run_loss(dev, B, A, clip_value, coef)
            for k in ("loss", "stats", "dmu", "dvalues", "dlogstd"):
                assert torch.equal(_bits(again[k][1]), _bits(bufs[k][1])), f"{what}: {k} differs between calls"
    return r64


@pytest.mark.parametrize("B,A,mu16,v16,clip_value", LOSS_CASES)
def test_ppo_loss_gradients_match_float64_reference(B, A, mu16, v16, clip_value):
    """d mu, d values, d logstd, their exact zeros, the same bits from three calls, nothing written past the sizes."""
    fails = []
    _loss_case(B, A, mu16, v16, clip_value, GRADS, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,A,mu16,v16,clip_value", LOSS_CASES)
def test_ppo_loss_value_and_means_match_float64_reference(B, A, mu16, v16, clip_value):
    """The loss and the four means ("The actor mean and the loss" in the module docstring)."""
    fails = []
    _loss_case(B, A, mu16, v16, clip_value, MEANS, fails, repeat=False)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("which", [GRADS, MEANS])
def test_ppo_loss_one_row_minibatches(which):
    """rows = 1, A = 1, f32: one launch per phase of the generator's cycles, together every branch."""
    fails = []
    for seed in H.PPO_ONE_ROW_SEEDS:
        _loss_case(1, 1, 0, 0, 1, which, fails, seed=seed, repeat=seed == 0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mu16", [0, 1])
def test_ppo_loss_exact_zeros_without_bound_loss(mu16):
    """bounds_loss_coef = 0: d mu of every row whose clipped surrogate is selected, or whose advantage is 0, is
    exactly 0 (as d values where the clipped value wins outside +-e), and those rows exist."""
    fails = []
    r64 = _loss_case(385, 12, mu16, mu16, 1, GRADS, fails, bounds_loss_coef=0.0, seed=7)
    assert not fails, "\n".join(fails)
    zero_rows = (r64["dmu"] == 0).all(axis=1)
    assert 0.3 < zero_rows.mean() < 0.8 and 0.1 < (r64["dvalues"] == 0).mean() < 0.4


@pytest.mark.parametrize("mu16", [0, 1])
def test_ppo_loss_value_and_means_without_bound_loss(mu16):
    fails = []
    _loss_case(385, 12, mu16, mu16, 1, MEANS, fails, bounds_loss_coef=0.0, seed=7, repeat=False)
    assert not fails, "\n".join(fails)


def test_device_fp16_add_is_the_reference_bound_sum():
    """The reference's fp16 bound term (ppo_oracle.fp16_bound_sum) is torch's fp16 add on the device, bit for bit,
    on every fp16 value in [-4, 4]."""
    pos = torch.arange(0, 0x4401, dtype=torch.int32).to(torch.int16).view(F16)
    x = torch.cat([pos, -pos])
    for c in (O.SOFT_BOUND, -O.SOFT_BOUND):
        dev = (x.to(DEV) + c) if c > 0 else (x.to(DEV) - O.SOFT_BOUND)
        assert dev.dtype == F16 and torch.equal(_bits(dev), _bits(O.fp16_bound_sum(x, c)))


@pytest.mark.parametrize("v16", [0, 1])
@pytest.mark.parametrize("mu16", [0, 1])
@pytest.mark.parametrize("A", [1, 32])
@pytest.mark.parametrize("B", [1, 129])
def test_ppo_loss_backward_scales_and_casts(B, A, mu16, v16):
    """rl_ppo_loss_backward: (gradient * s) in f32, cast as torch's .half() / kept f32, bit for bit (s = 4096; tiny
    values reach fp16 subnormals, 20 overflows to inf)."""
    g = torch.Generator().manual_seed(B * 100 + A)
    dmu = torch.randn(B, A, generator=g) * 1e-3
    dv = torch.randn(B, generator=g) * 1e-3
    dls = torch.randn(A, generator=g)
    dmu.view(-1)[::5] *= 1e-5
    dmu.view(-1)[::7] = 0.0
    dv[::3] = 20.0
    s = torch.tensor(4096.0)
    want = ((dmu * s).to(F16 if mu16 else F32), (dv * s).to(F16 if v16 else F32), dls * s)
    outs = (_guarded(B * A, F16 if mu16 else F32), _guarded(B, F16 if v16 else F32), _guarded(A))
    L = _lib()
    d = [t.to(DEV) for t in (s, dmu, dv, dls)]
    rc = L.rl_ppo_loss_backward(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, A, outs[0][1].data_ptr(), mu16, outs[1][1].data_ptr(), v16,
                                outs[2][1].data_ptr(), _stream())
    assert rc == 0, L.rl_last_error().decode()
    torch.cuda.synchronize()
    for (buf, view), w, name in zip(outs, want, ("dmu", "dvalues", "dlogstd")):
        assert torch.equal(_bits(view), _bits(w.reshape(-1))), name
        assert bool(torch.isnan(buf[view.numel():]).all()), f"{name}: written past its end"


# ---------------------------------------------------------------------------------------------------------------
# the heads kernels

HEADS_CASES = [(32, 1, 200), (32, 4, 200), (64, 8, 200), (128, 12, 200), (128, 16, 200), (256, 24, 200),
               (256, 32, 200), (64, 32, 200), (128, 12, 4165), (256, 32, 4165)]
HEADS_SCALE = 1024.0
HEAD_GRADS = ("grad_w_mu", "grad_b_mu", "grad_w_v", "grad_b_v", "grad_logstd")
SENTINEL = 7.0  # pre-fill of dhidden: columns outside the two ranges and rows past `rows` keep it


@functools.lru_cache(maxsize=None)
def _heads_refs(Hd, A, B, clip_value):
    """(heads, minibatch, ref64, ref32, the f32 loss gradients both backward references and the kernel start from).
    Computed once per shape and shared; nothing changes them."""
    heads, mb = H.ppo_heads_minibatch(B, Hd, A, seed=Hd + A)
    args = list(heads.values()) + [mb[k] for k in NAMES[2:]] + [E, clip_value, *COEF.values(), HEADS_SCALE]
    r64 = O.ppo_heads_loss(*args)
    # the backward is a function of the f32 gradients it is handed: both references and the kernel get ref64's,
    # rounded to f32 (s is a power of two, so fp16(f32(dmu) s) is then one and the same number for all three)
    g32 = tuple(torch.from_numpy(r64[k]).to(F32) for k in ("dmu", "dvalues", "dlogstd"))
    r32 = O.ppo_heads_loss(*args, dtype=F32, grads=g32)
    return heads, mb, r64, r32, g32


def _heads_layout(Hd, layout):
    """(ld, actor column, critic column): 2H actor first, or 2H + 16 critic first at column 8."""
    return (2 * Hd, 0, Hd) if layout == 0 else (2 * Hd + 16, Hd + 8, 8)


def _heads_device(heads, mb, B, Hd, A, ld, acol, ccol):
    rng = np.random.RandomState(5)
    hid = torch.from_numpy(rng.randint(-1, 2, (B, ld)).astype(np.float32)).to(F16)  # lattice filler elsewhere
    hid[:, acol:acol + Hd] = heads["hidden_a"]
    hid[:, ccol:ccol + Hd] = heads["hidden_c"]
    # the fp16 parameter shadows at odd element offsets of one flat buffer (2-byte alignment only)
    flat = torch.zeros(1 + A * Hd + A + Hd + 1 + 8, dtype=F16)
    views, o = {}, 1
    for k in ("w_mu", "b_mu", "w_v", "b_v"):
        n = heads[k].numel()
        flat[o:o + n] = heads[k].reshape(-1)
        views[k] = (o, n)
        o += n
    flat = flat.to(DEV)
    dev = {k: flat[o:o + n] for k, (o, n) in views.items()}
    dev["hidden"] = hid.to(DEV)
    dev.update({k: mb[k].to(DEV) for k in NAMES[2:]})
    dev["_flat"] = flat
    return dev


def _heads_fwd(dev, B, Hd, A, ld, acol, ccol, clip_value):
    L = _lib()
    sizes = dict(dmu=B * A, dvalues=B, partials=max(1, L.rl_ppo_heads_partials_size(max(B, 1), Hd, A)), loss=1, stats=4,
                 dlogstd=A)
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    bufs["mu_out"] = _guarded(B * A, F16)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    rc = L.rl_ppo_heads_loss(dev["hidden"].data_ptr(), ld, acol, ccol, Hd, dev["w_mu"].data_ptr(),
                             dev["b_mu"].data_ptr(), dev["w_v"].data_ptr(), dev["b_v"].data_ptr(),
                             *[dev[k].data_ptr() for k in NAMES[2:]], B, A, E, clip_value, *COEF.values(), p["mu_out"],
                             p["dmu"], p["dvalues"], p["partials"], p["loss"], p["stats"], p["dlogstd"], _stream())
    torch.cuda.synchronize()
    return rc, bufs


def _heads_bwd(dev, g32, B, Hd, A, ld, acol, ccol, store, grad_bufs, dh, hidden_ptr=None):
    L = _lib()
    part = _guarded(max(1, L.rl_ppo_heads_partials_size(max(B, 1), Hd, A)))
    s = torch.tensor(HEADS_SCALE, device=DEV)
    gd = [t.to(DEV).contiguous() for t in g32]
    rc = L.rl_ppo_heads_loss_backward(s.data_ptr(), gd[0].data_ptr(), gd[1].data_ptr(), gd[2].data_ptr(),
                                      hidden_ptr or dev["hidden"].data_ptr(), ld, acol, ccol, Hd, dev["w_mu"].data_ptr(),
                                      dev["w_v"].data_ptr(), B, A, dh.data_ptr(), part[1].data_ptr(),
                                      *[grad_bufs[k][1].data_ptr() for k in HEAD_GRADS], store, _stream())
    torch.cuda.synchronize()
    return rc, part


def _heads_setup(Hd, A, B, layout, clip_value):
    heads, mb, r64, r32, g32 = _heads_refs(Hd, A, B, clip_value)
    ld, acol, ccol = _heads_layout(Hd, layout)
    dev = _heads_device(heads, mb, B, Hd, A, ld, acol, ccol)
    what = f"heads H={Hd} A={A} rows={B} ld={ld} acol={acol} clip={clip_value}"
    return r64, r32, g32, ld, acol, ccol, dev, what


@pytest.mark.parametrize("which", [GRADS, MEANS])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("Hd,A,B", HEADS_CASES)
def test_heads_loss_matches_float64_reference(Hd, A, B, layout, which):
    """Every (AM, NC) instantiation of k_heads_fwd, ragged row counts, both layouts (clip_value on with the first,
    off with the second): mu bit for bit the exact product on the lattice, then the loss fields against ppo_loss
    on that mu and v (GRADS: the gradients, their zeros, the same bits from two calls; MEANS: loss and stats)."""
    clip_value = 1 - layout
    r64, r32, g32, ld, acol, ccol, dev, what = _heads_setup(Hd, A, B, layout, clip_value)
    fails = []
    rc, bufs = _heads_fwd(dev, B, Hd, A, ld, acol, ccol, clip_value)
    assert rc == 0, _lib().rl_last_error().decode()
    _guards_intact(bufs)
    want_mu = torch.from_numpy(r64["mu"]).to(F16).reshape(-1)
    assert torch.equal(_bits(bufs["mu_out"][1]), _bits(want_mu)), \
        f"{what}: mu differs from the exact product at {torch.nonzero(bufs['mu_out'][1].cpu() != want_mu)[:8].flatten().tolist()}"
    _loss_fields(fails, what, _out(bufs), r64, r32, which)
    if which == GRADS:
        rc, again = _heads_fwd(dev, B, Hd, A, ld, acol, ccol, clip_value)
        for k in ("loss", "stats", "dmu", "dvalues", "dlogstd", "mu_out"):
            assert torch.equal(_bits(again[k][1]), _bits(bufs[k][1])), f"{what}: {k} differs between calls"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("Hd,A,B", HEADS_CASES)
def test_heads_backward_matches_float64_reference(Hd, A, B, layout, store):
    """Every instantiation of k_heads_bwd (H = 256: the two-pass row loop; H = 32: 16 row groups; AM = 32: 76 KB of
    LDS), both layouts, store and accumulate, from the reference's f32 loss gradients at s = 1024: d hidden (both
    column ranges, the other columns and the rows past `rows` untouched) and the five parameter gradients."""
    r64, r32, g32, ld, acol, ccol, dev, what = _heads_setup(Hd, A, B, layout, 1)
    what += f" store={store}"
    fails = []
    sizes = dict(grad_w_mu=A * Hd, grad_b_mu=A, grad_w_v=Hd, grad_b_v=1, grad_logstd=A)
    grad_bufs = {k: _guarded(n) for k, n in sizes.items()}
    old = {}
    if not store:  # accumulate into gradients of the reference's own size
        gen = torch.Generator().manual_seed(3)
        for k, n in sizes.items():
            old[k] = (torch.randn(n, generator=gen) * float(np.abs(r64[k]).max())).to(F32)
            grad_bufs[k][1].copy_(old[k])
    dh = torch.full((B + 2, ld), SENTINEL, dtype=F16, device=DEV)
    rc, part = _heads_bwd(dev, g32, B, Hd, A, ld, acol, ccol, store, grad_bufs, dh)
    assert rc == 0, _lib().rl_last_error().decode()
    assert bool(torch.isnan(part[0][part[1].numel():]).all()), f"{what}: backward partials written past their size"
    for k, (buf, view) in grad_bufs.items():
        assert bool(torch.isnan(buf[view.numel():]).all()), f"{what}: {k} written past its end"
        got = _np(view) - (_np(old[k]) if not store else 0.0)
        _field(fails, what, k, got, r64[k], r32[k])
    dhc = dh.cpu()
    _field(fails, what, "dhidden actor", dhc[:B, acol:acol + Hd].double().numpy(), r64["dhidden_a"], r32["dhidden_a"])
    _field(fails, what, "dhidden critic", dhc[:B, ccol:ccol + Hd].double().numpy(), r64["dhidden_c"], r32["dhidden_c"])
    keep = torch.ones(B + 2, ld, dtype=torch.bool)
    keep[:B, acol:acol + Hd] = False
    keep[:B, ccol:ccol + Hd] = False
    assert bool((dhc[keep] == SENTINEL).all()), f"{what}: dhidden written outside the two column ranges / the rows"
    assert not fails, "\n".join(fails)


def test_refusals_launch_nothing():
    """What heads_check and rl_ppo_loss's argument check refuse: a non-zero return, a message naming the call, and
    every output as it was (NaN-filled)."""
    Hd, A, B = 64, 8, 64
    _, mb = H.ppo_heads_minibatch(B, Hd, A)
    L = _lib()
    # inputs large enough for every refused shape (the refusal itself is what is checked)
    HM, AM, ld_alloc = 256, 33, 2 * 256 + 16
    z = lambda *shape: torch.zeros(*shape, dtype=F16)  # noqa: E731
    dev = _heads_device(dict(w_mu=z(AM, HM), b_mu=z(AM), w_v=z(HM), b_v=z(1), hidden_a=z(B, HM), hidden_c=z(B, HM)),
                        dict(mb, actions=torch.zeros(B, AM), logstd=torch.zeros(AM)), B, HM, AM, ld_alloc, 0, HM)
    g_big = (torch.zeros(B, AM), torch.zeros(B), torch.zeros(AM))
    base = dict(Hd=Hd, A=A, ld=2 * Hd, acol=0, ccol=Hd, off=0)
    refused = {"hidden 48": dict(Hd=48, ccol=48, ld=96), "33 actions": dict(A=33),
               "overlapping column ranges": dict(acol=0, ccol=32), "actor column 4": dict(acol=4, ccol=72, ld=144),
               "actor range past ld": dict(acol=72, ccol=0), "mis-aligned hidden": dict(off=2)}
    for name, over in refused.items():
        c = dict(base, **over)
        ptr = dev["hidden"].data_ptr() + c["off"]
        rc, bufs = _refused_fwd(dev, B, c, ptr)
        assert rc != 0 and b"rl_ppo_heads_loss" in L.rl_last_error(), name
        for k, (buf, view) in bufs.items():
            assert bool(torch.isnan(buf).all()), f"{name}: forward wrote {k}"
        grad_bufs = {k: _guarded(AM * HM) for k in HEAD_GRADS}
        dh = torch.full((B + 2, ld_alloc), float("nan"), dtype=F16, device=DEV)
        rc, part = _heads_bwd(dev, g_big, B, c["Hd"], c["A"], c["ld"], c["acol"], c["ccol"], 1, grad_bufs, dh,
                              hidden_ptr=ptr)
        assert rc != 0 and b"rl_ppo_heads_loss_backward" in L.rl_last_error(), name
        assert bool(torch.isnan(dh).all()) and bool(torch.isnan(part[0]).all()), f"{name}: backward wrote"
        for k, (buf, view) in grad_bufs.items():
            assert bool(torch.isnan(buf).all()), f"{name}: backward wrote {k}"
    # rl_ppo_loss with no rows
    d = {k: v.to(DEV) for k, v in H.ppo_minibatch(4, 3).items()}
    bufs = {k: _guarded(16) for k in ("dmu", "dvalues", "partials", "loss", "stats", "dlogstd")}
    rc = L.rl_ppo_loss(d["mu"].data_ptr(), 0, d["values"].data_ptr(), 0, *[d[k].data_ptr() for k in NAMES[2:]], 0, 3, E, 1,
                       *COEF.values(), *[bufs[k][1].data_ptr() for k in ("dmu", "dvalues", "partials", "loss", "stats",
                                                                         "dlogstd")], _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"rl_ppo_loss" in L.rl_last_error()
    assert all(bool(torch.isnan(buf).all()) for buf, _ in bufs.values())


def _refused_fwd(dev, B, c, ptr):
    """_heads_fwd with output buffers sized for the largest shape (a refused call must not touch them)."""
    L = _lib()
    bufs = {k: _guarded(B * 33 + 4096) for k in ("dmu", "dvalues", "partials", "loss", "stats", "dlogstd")}
    bufs["mu_out"] = _guarded(B * 33, F16)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    rc = L.rl_ppo_heads_loss(ptr, c["ld"], c["acol"], c["ccol"], c["Hd"], dev["w_mu"].data_ptr(), dev["b_mu"].data_ptr(),
                             dev["w_v"].data_ptr(), dev["b_v"].data_ptr(), *[dev[k].data_ptr() for k in NAMES[2:]], B,
                             c["A"], E, 1, *COEF.values(), p["mu_out"], p["dmu"], p["dvalues"], p["partials"], p["loss"],
                             p["stats"], p["dlogstd"], _stream())
    torch.cuda.synchronize()
    return rc, bufs
