"""rl_linear_fwd(_g), rl_linear_fwd_f32_g, rl_linear_bwd(_g), rl_linear_transpose and rl_splitk_accum(_multi) at the
C ABI against the float64 references of the same statements (oracle/linear_oracle.py), on the inputs and shape lists
of tests/helpers.py (what is claimed of them is asserted on the CPU in tests/test_linear_oracle.py), at the smallest
shapes that reach each branch of each kernel (csrc/rl_linear.hip, csrc/rl_grad.hip).

Every real-valued output is judged by two rules.  The max-norm rule of tests/test_ppo_loss_gpu.py (tests/helpers.py
field_check; fp16 outputs against the references rounded to fp16):
    max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|
(err_f32 of an fp16 field: a flip of the fp16 rounding is a rare event, a few elements in 8192, and lands in any
binade, so one small draw does not measure what float32 rounding does to the field; as for the one-number outputs of
tests/test_learner_kernels_gpu.py, err_f32 is the largest over the draws of seeds 1000 .. of the shape, 2^21 elements'
worth and 16 at the most, this input's own included) and, per element, against the unrounded float64 reference
(tests/helpers.py elementwise_check):
    |kernel - ref64| <= h + (terms + 2) 2^-24 S + 4 2^-24 |ref64|
with S the same sum on absolute values, `terms` the length of the reduction and h half an fp16 spacing for fp16
outputs.  Beyond the rules: every byte a call may not write keeps its NaN sentinel (gap columns, other groups' rows,
partial blocks past `splits`, 64-element tails of exactly sized buffers); every call is made twice and must repeat
bit for bit; the bias partials equal the f32 sum of the reference's rounded dZ in the documented order bit for bit;
the finishes equal the ascending f32 sum bit for bit; refusals are nonzero, named, and write nothing.

MEASURED on an MI355X (191 tests in 7.9 s of the whole suite's 63.5 s): per field the largest err_kernel / err_f32,
in brackets the largest err_kernel / bar (<= 1 passes), then the largest elementwise err / bound (<= 1 passes) over
all cases.
    fwd y 1.0 [0.25] 0.998          fwd y elu 2.0 [0.50] 0.998       (0.998: the fp16 rounding of the output itself)
    f32 fwd y 1.4 [0.23] 0.27       f32 fwd y elu 1.4 [0.21] 0.27
    bwd dx 1.0 [0.25] 0.98          bwd wpart 0.84 [0.16] 0.036      bwd bpart 2.7 [0.15] 0.014 (and bit-equal)
    chain grad added 0.59 [0.10]    stored 0.53 [0.10]               (max-norm rule only)

What the tests found.  No kernel's arithmetic: every field was inside both rules as the kernels stood.  Two things in
the entry points: rl_linear_bwd_g checked wpart's alignment and pstride after it had launched the dx kernel, so that
refusal left dx written (every check now comes before the first launch), and rl_linear_fwd_g / rl_linear_bwd_g took
ldx < K (now refused, as rl_linear_fwd_f32_g did).  And one thing in the rule: with err_f32 from the one draw under
test, three of the 88 fp16 forward cases (64 x 128 at K = 60 and 64, 128 x 128 K = 68 grouped) missed the max-norm
bar by 11 .. 26 x while at 0.998 of the elementwise bound -- the kernel's one flipped fp16 rounding fell in a higher
binade than the float32 reference's few; hence the draws described above.

Deliberate mutations, each built into a scratch copy of the library and run against this module (the tests that
failed; the largest err_kernel / bar and elementwise err / bound among the fields beyond them).  The small-integer
tests of tests/test_ppo_gpu.py (test_linear_kernels_exact_on_integers, test_linear_f32_kernel_exact_on_integers_and_elu)
pass with each of the first three.
    (a) k_gemm_nt's accumulator through fp16 once per stage: 76 of the 88 of
        test_linear_fwd_matches_float64_reference (all but the 12 with one stage, no bias and no ELU, where the extra
        rounding is the output's own); fwd y and fwd y elu bar 8.0, elementwise 34.8
    (b) k_gemm_tn summing the unrounded dZ into the bias sum: all 10 of test_linear_bwd_partials_match_float64_reference
        and both of test_linear_bwd_then_finish_matches_float64_gradients; bpart bar 255, elementwise 19.1, not
        bit-equal; chain grad bar 21
    (c) ELU evaluated on the fp16-rounded z: 41 of the 44 of test_linear_fwd_matches_float64_reference with act = 1;
        fwd y elu elementwise 2.48, while its max-norm figure stays at 0.5 of the bar: only the elementwise rule sees it
    (d) k_gemm_nt's stage count R / KS, at least 1: the 36 forward tests with K % 64 != 0 and K > 64 (68, 132, 188,
        196); bar 853, elementwise 4e4
    (e) the direct-store arm's columns 4 g + 16 hh: the 16 forward tests of the four direct-store cases and the 3 dx
        cases with lddx = 132 / the groups with gaps; bar 1.3e3, elementwise 5e6
    (f) tile_of's first runs of length q: 36 forward, 6 f32 forward and 7 dx tests (every tile count T with
        T % 8 >= 2; at T % 8 == 1 the mutated run is the one that starts at 0): output tiles left at their sentinel
    (h) k_splitk_accum's spare slots added: the 16 cases of test_splitk_accum_is_the_ascending_f32_sum with
        P = 1, 15, 17, 33 on the vector path (n = 4, 260)
    (i) the f32 kernel's default stage width inverted: nothing fails, and nothing that looks at values can: both
        widths feed the matrix cores the same k in the same order, so every output bit is the same (asserted here for
        the default cases against both forced widths).  It is a performance choice only.
    (g) k_gemm_tn prefetching when st + 1 <= steps was not run: in the last row block it loads the 64 rows past the
        end of dy, y and x.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import linear_oracle as LO
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")
SEEN, SEEN_EL = {}, {}  # field -> [err_kernel / err_f32, err_kernel / bar]; field -> largest elementwise err / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for f, (r32, rbar) in sorted(SEEN.items()):
        print(f"[linear ratios] {f}: err_kernel / err_f32 <= {r32:.3g}, err_kernel / bar <= {rbar:.3g}, "
              f"elementwise err / bound <= {SEEN_EL.get(f, float('nan')):.3g}")


def _lib():
    from isaacgymenv_amd.rl import gae
    return gae.lib()


def _groups(**kw):
    from isaacgymenv_amd.rl import gae
    g = gae.LinearGroups()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().rl_last_error().decode()


def _nan(n, dtype):
    return torch.full((int(n),), NAN, dtype=dtype, device=DEV)


_np, _bits, _same_bits = H.np64, H.bits, H.same_bits  # shared with the other float64-referenced kernel modules


def _judge(fails, what, field, got, r64, r64_out, r32_out, S, terms, out_half, act=False, worst_32=None):
    """Both rules on one output: got (as stored) against the unrounded ref64 per element, and against the references
    as stored (rounded to fp16 for fp16 outputs) in the max norm.  worst_32: err_f32 of other draws of the shape (this
    input's own draw is included here)."""
    H.elementwise_check("linear", SEEN_EL, fails, what, field, _np(got), _np(r64), _np(S), terms, out_half, act)
    err_32 = None if worst_32 is None else max(worst_32, float(np.abs(_np(r32_out) - _np(r64_out)).max()))
    H.field_check("linear", SEEN, fails, what, field, _np(got), _np(r64_out), _np(r32_out), err_32=err_32)


def _draws(elements):
    """Draws of a shape that err_f32 of an fp16 field is taken over: 2^21 elements' worth, 16 at the most."""
    return min(16, -(-2 ** 21 // elements))


@functools.lru_cache(maxsize=None)
def _fwd_worst_half(M, N, K, act, with_bias):
    """The largest |fp16(ref32) - fp16(ref64)| of the forward over _draws inputs of this shape (seeds 1000 ..)."""
    worst = 0.0
    for k in range(_draws(M * N)):
        d = H.linear_inputs(M, K, N, seed=1000 + k)
        a = (d["x"][0], d["w"][0], d["b"][0] if with_bias else None, act)
        worst = max(worst, float((LO.linear_fwd(*a, dtype=F32)[1].double() - LO.linear_fwd(*a)[1].double()).abs().max()))
    return worst


@functools.lru_cache(maxsize=None)
def _dx_worst_half(M, N, K):
    worst = 0.0
    for k in range(_draws(M * K)):
        d = H.linear_bwd_inputs(M, K, N, seed=1000 + k)
        a = (d["dy"][0], d["y"][0], d["x"][0], d["w"][0], 0)
        worst = max(worst, float((LO.linear_bwd(*a, dtype=F32)["dx_half"].double() - LO.linear_bwd(*a)["dx_half"].double()).abs().max()))
    return worst


def _place(buf, off, rows, ld, col0, block):
    """block [rows][cols] into the flat buffer at element off + r * ld + col0 + c."""
    cols = block.shape[1]
    idx = off + torch.arange(rows).reshape(-1, 1) * ld + col0 + torch.arange(cols).reshape(1, -1)
    buf[idx.reshape(-1).to(DEV)] = block.reshape(-1).to(buf.dtype).to(DEV)
    return idx.reshape(-1)


def _only_written(buf_cpu, written, what):
    """Every element of the buffer outside `written` (flat indices) still holds its NaN sentinel, every one inside a
    number."""
    mask = torch.zeros(buf_cpu.numel(), dtype=torch.bool)
    mask[written] = True
    assert bool(torch.isnan(buf_cpu[~mask]).all()), f"{what}: written outside its output"
    assert not bool(torch.isnan(buf_cpu[mask]).any()), f"{what}: output elements left unwritten (or NaN)"


# ========================================================================================================= forward
def _fwd_layout(c):
    """(ldx, x_gstride, w_gstride, b_gstride, ldy, y_gstride, y_off) of a forward case.  Grouped: the groups' inputs
    side by side in the rows of x (as a grouped layer reads the layer before it) and their outputs side by side in
    the rows of y; gaps: every stride distinct, none dense."""
    M, N, K, G = c["M"], c["N"], c["K"], c["G"]
    if G == 1:
        return c.get("ldx", K), 0, 0, 0, c.get("ldy", N), 0, c.get("y_off", 0)
    if c.get("gaps"):
        return G * K + 4, K, N * K + 8, N + 8, G * (N + 4) + 4, N + 4, 0
    gy = c.get("y_gstride", N)
    return G * K, K, N * K, N, c.get("ldy", G * gy), gy, 0


def _fwd_call(c, d, act, with_bias, f32):
    """One forward call of case c on inputs d.  Returns (rc, y buffer on the CPU, per group the flat indices of its
    output in that buffer)."""
    L = _lib()
    M, N, K, G = c["M"], c["N"], c["K"], c["G"]
    ldx, gx, gw, gb, ldy, gy, y_off = _fwd_layout(c)
    dt = F32 if f32 else F16
    sfx = "32" if f32 else ""
    xb, wb, bb = _nan(M * ldx, dt), _nan((G - 1) * gw + N * K, dt), _nan((G - 1) * gb + N, dt)
    yb = _nan(y_off + M * ldy + GUARD, dt)
    where = []
    for g in range(G):
        _place(xb, 0, M, ldx, g * gx, d["x" + sfx][g])
        _place(wb, g * gw, N, K, 0, d["w" + sfx][g])
        _place(bb, g * gb, 1, N, 0, d["b" + sfx][g].reshape(1, N))
        idx = y_off + torch.arange(M).reshape(-1, 1) * ldy + g * gy + torch.arange(N).reshape(1, -1)
        where.append(idx.reshape(-1))
    yp = yb.data_ptr() + y_off * yb.element_size()
    bp = bb.data_ptr() if with_bias else None
    grp = None if G == 1 and ldy == N else _groups(groups=G, ldy=ldy, x_gstride=gx, w_gstride=gw, b_gstride=gb, y_gstride=gy)
    gp = None if grp is None else ctypes.byref(grp)
    if f32:
        rc = L.rl_linear_fwd_f32_g(xb.data_ptr(), M, K, ldx, wb.data_ptr(), N, bp, act, yp, gp, _stream())
    elif grp is None:
        rc = L.rl_linear_fwd(xb.data_ptr(), M, K, ldx, wb.data_ptr(), N, bp, act, yp, _stream())
    else:
        rc = L.rl_linear_fwd_g(xb.data_ptr(), M, K, ldx, wb.data_ptr(), N, bp, act, yp, gp, _stream())
    torch.cuda.synchronize()
    return rc, yb.cpu(), where


def _fwd_case(c, act, with_bias, f32, seed):
    M, N, K, G = c["M"], c["N"], c["K"], c["G"]
    d = H.linear_inputs(M, K, N, seed=seed, G=G)
    extra = {k: v for k, v in c.items() if k not in "MNKG"}
    what = f"{'f32 ' if f32 else ''}fwd {M}x{N} K={K} G={G} act={act} bias={int(with_bias)} {extra}"
    rc, y, where = _fwd_call(c, d, act, with_bias, f32)
    assert rc == 0, _err()
    _only_written(y, torch.cat(where), what)
    rc, again, _ = _fwd_call(c, d, act, with_bias, f32)
    assert rc == 0 and _same_bits(again, y), f"{what}: differs between calls"
    fails = []
    sfx = "32" if f32 else ""
    field = ("f32 fwd y" if f32 else "fwd y") + (" elu" if act else "")
    for g in range(G):
        x, w, b = d["x" + sfx][g], d["w" + sfx][g], d["b" + sfx][g] if with_bias else None
        got = y[where[g]].reshape(M, N)
        S = LO.fwd_magnitudes(x, w, b)
        if f32:
            r64 = LO.linear_fwd(x, w, b, act, out_half=False)
            r32 = LO.linear_fwd(x, w, b, act, dtype=F32, out_half=False)
            _judge(fails, f"{what} g={g}", field, got, r64, r64, r32, S, K, False, act)
        else:
            r64, r64h = LO.linear_fwd(x, w, b, act)
            _, r32h = LO.linear_fwd(x, w, b, act, dtype=F32)
            _judge(fails, f"{what} g={g}", field, got, r64, r64h, r32h, S, K, True, act,
                   worst_32=_fwd_worst_half(M, N, K, act, with_bias))
    assert not fails, "\n".join(fails)
    return y


@pytest.mark.parametrize("act,with_bias", [(0, True), (1, True), (0, False), (1, False)])
@pytest.mark.parametrize("ci", range(len(H.LIN_FWD_CASES)), ids=lambda i: "-".join(f"{k}{v}" for k, v in H.LIN_FWD_CASES[i].items()))
def test_linear_fwd_matches_float64_reference(ci, act, with_bias):
    """k_gemm_nt at every stage edge of its 64-wide reduction (K below, at and just past one and two stages), tile
    counts 1 .. 15 not multiples of 8 (tile_of's uneven runs), both tile forms on either side of the 256-workgroup
    threshold, ldx > K, the direct-store arm (y or its rows off the 16-byte grid; in one group of two only), three
    groups with every stride distinct; with and without bias and ELU."""
    _fwd_case(H.LIN_FWD_CASES[ci], act, with_bias, False, seed=ci)


def test_linear_fwd_overflow_and_deep_negative():
    """Pre-activations beyond 65504 give +-inf exactly where the reference's fp16 rounding does (elements within the
    elementwise bound of the rounding boundary 65520 excepted), the finite rest inside the bound, ELU of them -1;
    pre-activations around -20 give exactly -1."""
    c = dict(M=64, N=128, K=64, G=1)
    d = H.linear_inputs(64, 64, 128, seed=77)
    d["x"] = (d["x32"] * 64.0).to(F16)
    d["w"] = (d["w32"] * 300.0).to(F16)
    for act in (0, 1):
        rc, y, where = _fwd_call(c, d, act, True, False)
        assert rc == 0, _err()
        got = y[where[0]].reshape(64, 128)
        r64, r64h = LO.linear_fwd(d["x"][0], d["w"][0], d["b"][0], act)
        S = LO.fwd_magnitudes(d["x"][0], d["w"][0], d["b"][0])
        bound = torch.from_numpy((64 + 2) * 2.0 ** -24 * _np(S) + 4 * 2.0 ** -24 * np.abs(_np(r64)))
        decided = (r64.abs() - 65520.0).abs() > bound
        assert int(torch.isinf(r64h).sum()) >= 8 and (act or bool((r64h == -float("inf")).any()))
        assert torch.equal(torch.isinf(got)[decided], torch.isinf(r64h)[decided]), "inf pattern differs from the reference's"
        over = torch.isinf(got) & decided
        assert torch.equal(got[over], r64h[over]), "sign of an overflow"
        fin = torch.isfinite(got) & torch.isfinite(r64h)
        fails = []
        H.elementwise_check("linear", {}, fails, f"overflow act={act}", "fwd y", _np(got[fin]), _np(r64[fin]), _np(S[fin]), 64, True, act)
        assert not fails, "\n".join(fails)
        if act:
            assert bool((got[r64 < -20] == -1).all())
    d = H.linear_inputs(64, 64, 128, seed=78)
    d["b"] = (d["b32"] - 24.0).to(F16)
    z, _ = LO.linear_fwd(d["x"][0], d["w"][0], d["b"][0], 0)
    assert float(z.max()) < -12 and float(z.min()) > -40
    rc, y, where = _fwd_call(c, d, 1, True, False)
    assert rc == 0, _err()
    assert torch.equal(y[where[0]], torch.full((64 * 128,), -1.0, dtype=F16)), "ELU of z ~ -24 is not exactly -1"


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("ci", range(len(H.LIN_F32_CASES)), ids=lambda i: "-".join(f"{k}{v}" for k, v in H.LIN_F32_CASES[i].items()))
def test_linear_fwd_f32_matches_float64_reference(ci, act, monkeypatch):
    """k_gemm_nt_f32 at the stage edges of both stage widths (RL_F32_KSTEP), N = 64 ungrouped, 1 .. 15 tiles, three
    groups with gap columns, and the default stage choice on either side of 512 workgroups.  Both widths feed the
    matrix cores the same k in the same order, so they must agree bit for bit: the default cases are compared with
    both forced widths (which of the two a default call took cannot be read from its output)."""
    c = H.LIN_F32_CASES[ci]
    if "kstep" in c:
        monkeypatch.setenv("RL_F32_KSTEP", c["kstep"])
    else:
        monkeypatch.delenv("RL_F32_KSTEP", raising=False)
    y = _fwd_case(c, act, True, True, seed=100 + ci)
    if "kstep" not in c:
        d = H.linear_inputs(c["M"], c["K"], c["N"], seed=100 + ci, G=c["G"])
        for ks in ("32", "64"):
            monkeypatch.setenv("RL_F32_KSTEP", ks)
            rc, forced, _ = _fwd_call(c, d, act, True, True)
            assert rc == 0 and _same_bits(forced, y), f"stage width {ks} differs from the default call"
    if ci == 0:  # bias == NULL, once
        _fwd_case(c, act, False, True, seed=100 + ci)


# ======================================================================================================== backward
def _bwd_layout(c):
    """(ldy, y_gstride, ldx, x_gstride, w_gstride, lddx, dx_gstride) of a dX case."""
    N, K, G = c["N"], c["K"], c["G"]
    if G == 1:
        return N, 0, K, 0, 0, c.get("lddx", K), 0
    return G * (N + 4) + 4, N + 4, G * K + 4, K, N * K + 8, G * (K + 4) + 4, K + 4


def _dx_call(c, d):
    L = _lib()
    M, N, K, G = c["M"], c["N"], c["K"], c["G"]
    ldy, gy, ldx, gx, gw, lddx, gdx = _bwd_layout(c)
    dyb, yb, xb = _nan(M * ldy, F16), _nan(M * ldy, F16), _nan(M * ldx, F16)
    wb, dxb = _nan((G - 1) * gw + N * K, F16), _nan(M * lddx + GUARD, F16)
    where = []
    for g in range(G):
        _place(dyb, 0, M, ldy, g * gy, d["dy"][g])
        _place(yb, 0, M, ldy, g * gy, d["y"][g])
        _place(xb, 0, M, ldx, g * gx, d["x"][g])
        _place(wb, g * gw, N, K, 0, d["w"][g])
        idx = torch.arange(M).reshape(-1, 1) * lddx + g * gdx + torch.arange(K).reshape(1, -1)
        where.append(idx.reshape(-1))
    if G == 1 and lddx == K:
        rc = L.rl_linear_bwd(dyb.data_ptr(), yb.data_ptr(), M, N, xb.data_ptr(), K, ldx, wb.data_ptr(), dxb.data_ptr(), 1,
                             None, None, 0, _stream())
    else:
        grp = _groups(groups=G, ldy=ldy, lddx=lddx, x_gstride=gx, w_gstride=gw, y_gstride=gy, dx_gstride=gdx)
        rc = L.rl_linear_bwd_g(dyb.data_ptr(), yb.data_ptr(), M, N, xb.data_ptr(), K, ldx, wb.data_ptr(), dxb.data_ptr(), 1,
                               None, None, 0, ctypes.byref(grp), _stream())
    torch.cuda.synchronize()
    return rc, dxb.cpu(), where


@pytest.mark.parametrize("ci", range(len(H.LIN_DX_CASES)), ids=lambda i: "-".join(f"{k}{v}" for k, v in H.LIN_DX_CASES[i].items()))
def test_linear_bwd_dx_matches_float64_reference(ci):
    """k_gemm_nn: one and three reduction stages, lddx dense / off the 16-byte grid (direct-store arm) / padded on
    it, both tile forms on either side of the 256-workgroup threshold, three groups with gaps.  The rows of dx whose
    dZ has one nonzero term from a special y (0, -0, the largest fp16 below 0, 65504) are that one product rounded
    once, bit for bit; the row whose y is -1 throughout is exactly 0."""
    c = H.LIN_DX_CASES[ci]
    M, N, K, G = c["M"], c["N"], c["K"], c["G"]
    d = H.linear_bwd_inputs(M, K, N, seed=200 + ci, G=G)
    what = f"dx {M}x{K} N={N} G={G} lddx={c.get('lddx', 0)}"
    rc, dx, where = _dx_call(c, d)
    assert rc == 0, _err()
    _only_written(dx, torch.cat(where), what)
    rc, again, _ = _dx_call(c, d)
    assert rc == 0 and _same_bits(again, dx), f"{what}: differs between calls"
    fails = []
    for g in range(G):
        args = (d["dy"][g], d["y"][g], d["x"][g], d["w"][g], 0)
        r64, r32 = LO.linear_bwd(*args), LO.linear_bwd(*args, dtype=F32)
        S = LO.bwd_magnitudes(r64["dz"], None, d["w"][g], 0)
        got = dx[where[g]].reshape(M, K)
        _judge(fails, f"{what} g={g}", "bwd dx", got, r64["dx"], r64["dx_half"], r32["dx_half"], S["dx"], N, True,
               worst_32=_dx_worst_half(M, N, K))
        for i, (name, _) in enumerate(H.LIN_SPECIAL_Y):
            if name == "minus_one":
                assert bool((got[1 + i] == 0).all()), f"{what} g={g}: the dx row of y == -1 is not 0"
            else:
                assert bool((r64["dx_half"][1 + i] != 0).any())
                assert _same_bits(got[1 + i], r64["dx_half"][1 + i]), f"{what} g={g}: the dx row of y == {name}"
    assert not fails, "\n".join(fails)


DW_LAYOUTS = ("separate", "merged", "grouped merged")


def _dw_call(M, N, K, splits, layout, d, with_bpart=True):
    """One weight / bias partial call.  Returns (rc, [buffers on the CPU], per group (buffer index, flat indices) of
    its wpart [splits][N][K] and of its bpart [splits][N]).  Every buffer holds one block more than `splits`."""
    L = _lib()
    G = 2 if layout == "grouped merged" else 1
    ldy, ldx = G * N, G * K
    dyb, yb, xb = _nan(M * ldy, F16), _nan(M * ldy, F16), _nan(M * ldx, F16)
    for g in range(G):
        _place(dyb, 0, M, ldy, g * N, d["dy"][g])
        _place(yb, 0, M, ldy, g * N, d["y"][g])
        _place(xb, 0, M, ldx, g * K, d["x"][g])
    blocks = torch.arange(splits).reshape(-1, 1)
    if layout == "separate":
        bufs = [_nan((splits + 1) * N * K + GUARD, F32), _nan((splits + 1) * N + GUARD, F32)]
        wp, bp, pstride = bufs[0].data_ptr(), bufs[1].data_ptr(), 0
        wwhere = [(0, (blocks * N * K + torch.arange(N * K).reshape(1, -1)).reshape(-1))]
        bwhere = [(1, (blocks * N + torch.arange(N).reshape(1, -1)).reshape(-1))]
    else:
        pstride = G * (N * K + N)
        bufs = [_nan((splits + 1) * pstride + GUARD, F32)]
        wp, bp = bufs[0].data_ptr(), bufs[0].data_ptr() + 4 * G * N * K
        wwhere = [(0, (blocks * pstride + g * N * K + torch.arange(N * K).reshape(1, -1)).reshape(-1)) for g in range(G)]
        bwhere = [(0, (blocks * pstride + G * N * K + g * N + torch.arange(N).reshape(1, -1)).reshape(-1)) for g in range(G)]
    if not with_bpart:
        bp = None
    if G == 1:
        rc = L.rl_linear_bwd(dyb.data_ptr(), yb.data_ptr(), M, N, xb.data_ptr(), K, ldx, None, None, splits, wp, bp, pstride,
                             _stream())
    else:
        grp = _groups(groups=G, ldy=ldy, x_gstride=K, y_gstride=N, part_gstride=N * K, bpart_gstride=N)
        rc = L.rl_linear_bwd_g(dyb.data_ptr(), yb.data_ptr(), M, N, xb.data_ptr(), K, ldx, None, None, splits, wp, bp, pstride,
                               ctypes.byref(grp), _stream())
    torch.cuda.synchronize()
    return rc, [b.cpu() for b in bufs], wwhere, bwhere


def _written_by_buffer(bufs, regions, what):
    for k, buf in enumerate(bufs):
        mine = [idx for b, idx in regions if b == k]
        _only_written(buf, torch.cat(mine) if mine else torch.zeros(0, dtype=torch.long), f"{what} buffer {k}")


@pytest.mark.parametrize("N", H.LIN_DW_N)
@pytest.mark.parametrize("M,splits", H.LIN_DW_SPLITS)
def test_linear_bwd_partials_match_float64_reference(M, splits, N):
    """k_gemm_tn: row blocks of one stage (no prefetch), two, three and six stages; K = 4 (one 4-group of a k tile),
    124 / 128 / 132 / 188 (the tail on either side of a tile); the separate, merged and grouped merged layouts, each
    with one block more than `splits` that must stay untouched.  bpart: the f32 sum of the reference's rounded dZ in
    the documented order, bit for bit.  bpart == NULL: the same weight partials, the bias regions untouched."""
    R = M // splits
    fails = []
    for K in H.LIN_DW_K:
        d = H.linear_bwd_inputs(M, K, N, seed=300 + K, G=2)
        refs = []
        for g in range(2):
            args = (d["dy"][g], d["y"][g], d["x"][g], None, splits)
            r64 = LO.linear_bwd(*args)
            refs.append((r64, LO.linear_bwd(*args, dtype=F32), LO.bwd_magnitudes(r64["dz"], d["x"][g], None, splits),
                         torch.from_numpy(LO.bpart_kernel_order(r64["dz"], splits))))
        for layout in DW_LAYOUTS:
            what = f"dw M={M} splits={splits} N={N} K={K} {layout}"
            rc, bufs, wwhere, bwhere = _dw_call(M, N, K, splits, layout, d)
            assert rc == 0, _err()
            _written_by_buffer(bufs, wwhere + bwhere, what)
            rc, again, _, _ = _dw_call(M, N, K, splits, layout, d)
            assert rc == 0 and all(_same_bits(a, b) for a, b in zip(again, bufs)), f"{what}: differs between calls"
            for g in range(len(wwhere)):
                r64, r32, S, border = refs[g]
                wgot = bufs[wwhere[g][0]][wwhere[g][1]].reshape(splits, N, K)
                bgot = bufs[bwhere[g][0]][bwhere[g][1]].reshape(splits, N)
                _judge(fails, f"{what} g={g}", "bwd wpart", wgot, r64["wpart"], r64["wpart"], r32["wpart"], S["wpart"], R, False)
                _judge(fails, f"{what} g={g}", "bwd bpart", bgot, r64["bpart"], r64["bpart"], r32["bpart"], S["bpart"], R, False)
                assert _same_bits(bgot, border), \
                    f"{what} g={g}: bpart is not the documented f32 sum of the rounded dZ (max diff " \
                    f"{float((bgot - border).abs().max()):.3e})"
            if layout == "merged":
                rc, nob, wwhere2, _ = _dw_call(M, N, K, splits, layout, d, with_bpart=False)
                assert rc == 0, _err()
                _written_by_buffer(nob, wwhere2, what + " bpart=NULL")
                assert _same_bits(nob[0][wwhere2[0][1]], bufs[0][wwhere[0][1]]), f"{what}: wpart differs without bpart"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("offset", [0, 1])
def test_linear_bwd_then_finish_matches_float64_gradients(offset):
    """rl_linear_bwd (merged layout, 16 row blocks) finished by rl_splitk_accum into a gradient view at float offset
    0 / 1 (vector / scalar path) of a flat buffer, onto a nonzero gradient: against g0 + dZ^T x | sum dZ in float64.
    Then rl_splitk_accum_multi in store mode into a NaN-filled buffer: the sums themselves."""
    from isaacgymenv_amd.rl import gae
    L = _lib()
    M, splits, N, K = 1024, 16, 128, 188
    n = N * K + N
    d = H.linear_bwd_inputs(M, K, N, seed=400)
    rc, bufs, wwhere, bwhere = _dw_call(M, N, K, splits, "merged", d)
    assert rc == 0, _err()
    parts = bufs[0][:splits * n].to(DEV)
    args = (d["dy"][0], d["y"][0], d["x"][0], None, 1)
    r64, r32 = LO.linear_bwd(*args), LO.linear_bwd(*args, dtype=F32)
    tot64 = torch.cat([r64["wpart"].reshape(-1), r64["bpart"].reshape(-1)])
    tot32 = torch.cat([r32["wpart"].reshape(-1), r32["bpart"].reshape(-1)])
    g0 = torch.from_numpy(np.random.RandomState(5).normal(size=n)).to(F32) * float(tot64.abs().max()) * 0.1
    fails = []
    flat = _nan(offset + n + GUARD, F32)
    flat[offset:offset + n] = g0.to(DEV)
    rc = L.rl_splitk_accum(parts.data_ptr(), splits, n, 0, flat.data_ptr() + 4 * offset, _stream())
    torch.cuda.synchronize()
    assert rc == 0, _err()
    out = flat.cpu()
    _only_written(out, torch.arange(offset, offset + n), "finish")
    H.field_check("linear", SEEN, fails, f"chain offset={offset}", "chain grad (added)", _np(out[offset:offset + n]),
                  _np(g0.double() + tot64), _np(g0 + tot32))
    flat = _nan(offset + n + GUARD, F32)
    job = (gae.SplitkJob * 1)(gae.SplitkJob(parts.data_ptr(), flat.data_ptr() + 4 * offset, n, splits, 0))
    rc = L.rl_splitk_accum_multi(job, 1, 1, _stream())
    torch.cuda.synchronize()
    assert rc == 0, _err()
    out = flat.cpu()
    _only_written(out, torch.arange(offset, offset + n), "finish (store)")
    H.field_check("linear", SEEN, fails, f"chain offset={offset}", "chain grad (stored)", _np(out[offset:offset + n]),
                  _np(tot64), _np(tot32))
    assert not fails, "\n".join(fails)


# ================================================================================================== rl_splitk_accum
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n", H.SPLITK_N)
@pytest.mark.parametrize("P", H.SPLITK_PARTS)
def test_splitk_accum_is_the_ascending_f32_sum(P, n, half):
    """One partial, a batch of 15 / 16, a second batch of one (17) and a third (33): the spare slots of the last batch
    reload partial P - 1 and must not add it.  n = 4 (one lane), 260 (two workgroups), 1539 (scalar path); gradient
    views at float offsets 0 and 1; rl_splitk_accum and rl_splitk_accum_multi adding, the latter storing into NaN."""
    from isaacgymenv_amd.rl import gae
    L = _lib()
    rng = np.random.RandomState(P * 1000 + n)
    parts = torch.from_numpy(rng.normal(size=(P, n))).to(F16 if half else F32)
    g0 = torch.from_numpy(rng.normal(size=n)).to(F32)
    total = LO.splitk_sum_kernel_order(parts)
    added = torch.from_numpy((g0.numpy() + total).astype(np.float32))
    pb = _nan(P * n + GUARD, parts.dtype)
    pb[:P * n] = parts.reshape(-1).to(DEV)
    for offset in (0, 1):
        for mode in ("accum", "multi add", "multi store"):
            what = f"splitk P={P} n={n} half={half} offset={offset} {mode}"
            flat = _nan(offset + n + GUARD, F32)
            if mode != "multi store":
                flat[offset:offset + n] = g0.to(DEV)
            gp = flat.data_ptr() + 4 * offset
            if mode == "accum":
                rc = L.rl_splitk_accum(pb.data_ptr(), P, n, int(half), gp, _stream())
            else:
                job = (gae.SplitkJob * 1)(gae.SplitkJob(pb.data_ptr(), gp, n, P, int(half)))
                rc = L.rl_splitk_accum_multi(job, 1, int(mode == "multi store"), _stream())
            torch.cuda.synchronize()
            assert rc == 0, _err()
            out = flat.cpu()
            _only_written(out, torch.arange(offset, offset + n), what)
            want = torch.from_numpy(total) if mode == "multi store" else added
            assert _same_bits(out[offset:offset + n], want), \
                f"{what}: not the ascending f32 sum (max diff {float((out[offset:offset + n] - want).abs().max()):.3e})"
    assert _same_bits(pb[:P * n], parts.reshape(-1)) and bool(torch.isnan(pb[P * n:]).all())


@pytest.mark.parametrize("N,K", H.TRANSPOSE_SHAPES)
def test_linear_transpose_is_the_transpose(N, K):
    w = torch.from_numpy(np.random.RandomState(N).normal(size=(N, K))).to(F16)
    out, wd = _nan(N * K + GUARD, F16), w.to(DEV)
    rc = _lib().rl_linear_transpose(wd.data_ptr(), N, K, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _err()
    assert _same_bits(out[:N * K].cpu().reshape(K, N), w.t().contiguous()) and bool(torch.isnan(out[N * K:]).all())


# ========================================================================================================= refusals
def _refused(rc, name, outs, what):
    assert rc != 0 and name in _err(), f"{what}: rc {rc}, message {_err()!r}"
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert bool(torch.isnan(b).all()), f"{what}: wrote {k}"


@pytest.mark.parametrize("f32", [False, True])
def test_linear_fwd_refusals(f32):
    """Each documented requirement of rl_linear_fwd_g / rl_linear_fwd_f32_g violated alone: nonzero, named, nothing
    written.  ldx < K is refused by both."""
    L = _lib()
    dt, es = (F32, 4) if f32 else (F16, 2)
    M, N, K = 128, 128, 64
    x, w, b = (torch.zeros(n + 64, dtype=dt, device=DEV) for n in (2 * M * (K + 8), 2 * N * K, 2 * N))
    name = "rl_linear_fwd_f32" if f32 else "rl_linear_fwd"
    fn = L.rl_linear_fwd_f32_g if f32 else L.rl_linear_fwd_g
    base = dict(x=x.data_ptr(), M=M, K=K, ldx=K, w=w.data_ptr(), N=N, b=b.data_ptr(), act=1, yoff=0, grp=None)
    two = dict(groups=2, ldy=2 * N, x_gstride=K, w_gstride=N * K, b_gstride=N, y_gstride=N)
    off = 8 if f32 else 4  # bytes: off the 16-byte (f32) / 8-byte (fp16) grid
    cases = {"x null": dict(x=None), "w null": dict(w=None), "y null": dict(yoff=None), "M = 0": dict(M=0), "K = 0": dict(K=0),
             "N = 0": dict(N=0), "M % 64": dict(M=96), "N off its tile": dict(N=64 if not f32 else 96), "K % 4": dict(K=62),
             "ldx % 4": dict(ldx=K + 2), "ldx < K": dict(ldx=K - 4), "x misaligned": dict(x=x.data_ptr() + off),
             "w misaligned": dict(w=w.data_ptr() + off), "y misaligned": dict(yoff=off),
             "groups = 0": dict(grp=dict(two, groups=0)), "groups = 65536": dict(grp=dict(two, groups=65536)),
             "ldy < N": dict(grp=dict(groups=1, ldy=N - 4)), "ldy % 4": dict(grp=dict(groups=1, ldy=N + 2)),
             "x_gstride % 4": dict(grp=dict(two, ldx=2 * K, x_gstride=K + 2)), "w_gstride % 4": dict(grp=dict(two, w_gstride=N * K + 2)),
             "y_gstride % 4": dict(grp=dict(two, y_gstride=N + 2))}
    if not f32:
        cases["b_gstride % 4"] = dict(grp=dict(two, b_gstride=N + 2))
    for what, change in cases.items():
        a = dict(base, **change)
        g = a["grp"]
        if g is not None:
            if "ldx" in g:
                a["ldx"] = g["ldx"]
            elif g.get("groups", 1) == 2 and "ldx" not in change:
                a["ldx"] = 2 * K
            g = _groups(**{k: v for k, v in g.items() if k != "ldx"})
        y = _nan(2 * M * 2 * N + 64, dt)
        yp = None if a["yoff"] is None else y.data_ptr() + a["yoff"]
        rc = fn(a["x"], a["M"], a["K"], a["ldx"], a["w"], a["N"], a["b"], a["act"], yp, None if g is None else ctypes.byref(g),
                _stream())
        _refused(rc, name, dict(y=y), f"{name} {what}")
    # the valid call the cases start from is accepted
    y = _nan(M * N, dt)
    assert fn(base["x"], M, K, K, base["w"], N, base["b"], 1, y.data_ptr(), None, _stream()) == 0, _err()
    torch.cuda.synchronize()


def test_linear_bwd_refusals():
    """Each documented requirement of rl_linear_bwd_g violated alone: nonzero, named, dx / wpart / bpart untouched."""
    L = _lib()
    M, N, K, splits = 128, 128, 128, 2
    z = lambda n: torch.zeros(n + 64, dtype=F16, device=DEV)  # noqa: E731
    dy, yv, x, w = z(2 * M * N), z(2 * M * N), z(2 * M * (K + 8)), z(2 * N * K)
    base = dict(dy=dy.data_ptr(), y=yv.data_ptr(), M=M, N=N, x=x.data_ptr(), K=K, ldx=K, w=w.data_ptr(), dxoff=0, splits=splits,
                wpoff=0, bp=True, pstride=0, grp=None)
    two = dict(groups=2, ldy=2 * N, lddx=2 * K, x_gstride=K, w_gstride=N * K, y_gstride=N, dx_gstride=K, part_gstride=N * K,
               bpart_gstride=N)
    cases = {"dy null": dict(dy=None), "y null": dict(y=None), "x null": dict(x=None), "M = 0": dict(M=0), "M % 128": dict(M=64),
             "N % 128": dict(N=64), "K % 4": dict(K=126, dxoff=None), "ldx % 4": dict(ldx=K + 2), "ldx < K": dict(ldx=K - 4),
             "dy misaligned": dict(dy=dy.data_ptr() + 4), "y misaligned": dict(y=yv.data_ptr() + 4),
             "x misaligned": dict(x=x.data_ptr() + 4), "splits = 0": dict(splits=0), "M % (64 splits)": dict(splits=4),
             "bpart without wpart": dict(wpoff=None), "dx without w": dict(w=None), "w misaligned": dict(w=w.data_ptr() + 4),
             "dx misaligned": dict(dxoff=4), "dx with K % 128": dict(K=64), "wpart misaligned": dict(wpoff=8),
             "pstride % 4": dict(pstride=N * K + N + 2), "pstride < N K": dict(pstride=N * K - 4),
             "groups = 0": dict(grp=dict(two, groups=0)), "splits x groups > 65535": dict(grp=dict(two, groups=40000)),
             "ldy < N": dict(grp=dict(groups=1, ldy=N - 4)), "ldy % 4": dict(grp=dict(groups=1, ldy=N + 2)),
             "lddx < K": dict(grp=dict(groups=1, lddx=K - 4)), "lddx % 4": dict(grp=dict(groups=1, lddx=K + 2)),
             "x_gstride % 4": dict(grp=dict(two, x_gstride=K + 2)), "w_gstride % 4": dict(grp=dict(two, w_gstride=N * K + 2)),
             "y_gstride % 4": dict(grp=dict(two, y_gstride=N + 2)), "dx_gstride % 4": dict(grp=dict(two, dx_gstride=K + 2)),
             "part_gstride % 4": dict(grp=dict(two, part_gstride=N * K + 2)),
             "bpart_gstride % 4": dict(grp=dict(two, bpart_gstride=N + 2))}
    for what, change in cases.items():
        a = dict(base, **change)
        g = a["grp"]
        if g is not None and g.get("groups", 1) != 1:
            a["ldx"] = 2 * K
            a["pstride"] = 2 * (N * K + N)
        outs = dict(dx=_nan(2 * M * 2 * K + 64, F16), wpart=_nan(8 * 2 * (N * K + N) + 64, F32), bpart=_nan(8 * 2 * N + 64, F32))
        dxp = None if a["dxoff"] is None else outs["dx"].data_ptr() + a["dxoff"]
        wpp = None if a["wpoff"] is None else outs["wpart"].data_ptr() + a["wpoff"]
        grp = None if g is None else _groups(**g)
        rc = L.rl_linear_bwd_g(a["dy"], a["y"], a["M"], a["N"], a["x"], a["K"], a["ldx"], a["w"], dxp, a["splits"], wpp,
                               outs["bpart"].data_ptr() if a["bp"] else None, a["pstride"],
                               None if grp is None else ctypes.byref(grp), _stream())
        _refused(rc, "rl_linear_bwd", outs, f"rl_linear_bwd {what}")
    outs = dict(dx=_nan(M * K, F16), wpart=_nan(splits * N * K, F32), bpart=_nan(splits * N, F32))
    assert L.rl_linear_bwd_g(base["dy"], base["y"], M, N, base["x"], K, K, base["w"], outs["dx"].data_ptr(), splits,
                             outs["wpart"].data_ptr(), outs["bpart"].data_ptr(), 0, None, _stream()) == 0, _err()
    torch.cuda.synchronize()


def test_transpose_and_splitk_refusals():
    from isaacgymenv_amd.rl import gae
    L = _lib()
    src = torch.zeros(256, dtype=F16, device=DEV)
    for what, (w, N, K, null_out) in {"w null": (None, 4, 4, False), "wt null": (src.data_ptr(), 4, 4, True),
                                      "N = 0": (src.data_ptr(), 0, 4, False), "K = 0": (src.data_ptr(), 4, 0, False)}.items():
        out = _nan(256, F16)
        rc = L.rl_linear_transpose(w, N, K, None if null_out else out.data_ptr(), _stream())
        _refused(rc, "rl_linear_transpose", dict(wt=out), f"rl_linear_transpose {what}")
    parts = torch.zeros(64, device=DEV)
    for what, (p, P, n, null_grad) in {"num_parts = 0": (parts.data_ptr(), 0, 8, False), "n < 0": (parts.data_ptr(), 2, -4, False),
                                       "parts null": (None, 2, 8, False), "grad null": (parts.data_ptr(), 2, 8, True)}.items():
        grad = _nan(64, F32)
        rc = L.rl_splitk_accum(p, P, n, 0, None if null_grad else grad.data_ptr(), _stream())
        _refused(rc, "rl_splitk_accum", dict(grad=grad), f"rl_splitk_accum {what}")
        job = (gae.SplitkJob * 1)(gae.SplitkJob(p, None if null_grad else grad.data_ptr(), n, P, 0))
        rc = L.rl_splitk_accum_multi(job, 1, 1, _stream())
        _refused(rc, "rl_splitk_accum_multi", dict(grad=grad), f"rl_splitk_accum_multi {what}")
    grad = _nan(64, F32)
    jobs = (gae.SplitkJob * 9)(*[gae.SplitkJob(parts.data_ptr(), grad.data_ptr(), 4, 2, 0) for _ in range(9)])
    for count in (0, 9):
        _refused(L.rl_splitk_accum_multi(jobs, count, 1, _stream()), "rl_splitk_accum_multi", dict(grad=grad), f"{count} jobs")
