"""oracle/linear_oracle.py against torch, what tests/helpers.py claims of the Linear + ELU inputs and shape lists, and
the elementwise rule itself (tests/helpers.py elementwise_check): the float32 reference stays inside it everywhere,
a layer whose accumulator passes through fp16 every 16 terms breaks it at 10 % of the elements or more.  CPU only;
tests/test_linear_kernels_gpu.py relies on all of it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import linear_oracle as LO
from tests import helpers as H

F16, F32, F64 = torch.float16, torch.float32, torch.float64
RULE_K = (4, 36, 68, 188, 512)


def _np(t):
    return t.detach().double().numpy()


@pytest.mark.parametrize("K", [4, 68, 188])
@pytest.mark.parametrize("act", [0, 1])
def test_float64_reference_is_torch_linear_elu_and_its_autograd(K, act):
    """With the dZ rounding switched off: y, dx, the summed weight partials and the summed bias partials equal
    torch.nn.functional.linear + elu and autograd's gradients in float64 (to float64 rounding of another order)."""
    M, N, splits = 128, 128, 2
    d = H.linear_inputs(M, K, N, seed=K)
    x = d["x"][0].double().requires_grad_(True)
    w = d["w"][0].double().requires_grad_(True)
    b = d["b"][0].double().requires_grad_(True)
    z = F.linear(x, w, b)
    y = F.elu(z) if act else z
    got, got16 = LO.linear_fwd(d["x"][0], d["w"][0], d["b"][0], act)
    torch.testing.assert_close(got, y.detach(), rtol=1e-13, atol=1e-14)
    assert got16.dtype == F16 and torch.equal(got16, got.to(F16))
    if not act:
        return
    dy = torch.from_numpy(np.random.RandomState(K).normal(size=(M, N)))
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
    r = LO.linear_bwd(dy, y.detach(), d["x"][0], d["w"][0], splits, round_dz=False)
    torch.testing.assert_close(r["dx"], gx, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r["wpart"].sum(0), gw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["bpart"].sum(0), gb, rtol=1e-12, atol=1e-12)
    assert r["wpart"].shape == (splits, N, K) and r["bpart"].shape == (splits, N)


def test_rounded_dz_is_torch_fp16_elu_backward():
    """dZ with its rounding on = torch's fp16 elu_backward from the result, bit for bit, specials included; and the
    same numbers in both dtypes."""
    d = H.linear_bwd_inputs(128, 36, 128, seed=1)
    dy, y = d["dy"][0], d["y"][0]
    want = torch.ops.aten.elu_backward(dy, 1.0, 1.0, 1.0, True, y)
    assert want.dtype == F16
    dz = LO.dz_of(dy, y)
    assert torch.equal(dz.to(F16).view(torch.int16), want.view(torch.int16))
    assert torch.equal(LO.dz_of(dy, y, F32).double(), dz)


@pytest.mark.parametrize("K", RULE_K)
def test_elementwise_rule_passes_float32_and_refuses_an_fp16_accumulator(K):
    """128 x 128 outputs, with and without ELU: the float32 reference rounded to fp16 breaks the bound at no element;
    the fp16-accumulating restatement breaks it at >= 10 % of the elements.  The f32 output (no fp16 rounding, h = 0)
    of the float32 reference is inside its bound as well."""
    d = H.linear_inputs(128, K, 128, seed=K)
    x, w, b = d["x"][0], d["w"][0], d["b"][0]
    S = _np(LO.fwd_magnitudes(x, w, b))
    for act in (0, 1):
        r64, _ = LO.linear_fwd(x, w, b, act)
        _, y32h = LO.linear_fwd(x, w, b, act, dtype=F32)
        seen, fails = {}, []
        worst, beyond = H.elementwise_check("linear rule", seen, fails, f"K={K} act={act} float32", "y", _np(y32h),
                                            _np(r64), S, K, True, act)
        assert not fails and beyond == 0.0 and worst <= 1.0, fails
        bad = LO.linear_fwd_half_accumulator(x, w, b, act)
        fails = []
        worst, beyond = H.elementwise_check("linear rule", seen, fails, f"K={K} act={act} fp16 accumulator", "y",
                                            _np(bad), _np(r64), S, K, True, act)
        assert fails and beyond >= 0.10, (K, act, worst, beyond)
        y32 = LO.linear_fwd(d["x32"][0], d["w32"][0], d["b32"][0], act, dtype=F32, out_half=False)
        r64f = LO.linear_fwd(d["x32"][0], d["w32"][0], d["b32"][0], act, out_half=False)
        fails = []
        H.elementwise_check("linear rule", seen, fails, f"K={K} act={act} float32, f32 output", "y f32", _np(y32),
                            _np(r64f), _np(LO.fwd_magnitudes(d["x32"][0], d["w32"][0], d["b32"][0])), K, False, act)
        assert not fails, fails


@pytest.mark.parametrize("K,N,M,splits", [(128, 128, 128, 2), (188, 384, 384, 1)])
def test_elementwise_rule_passes_the_float32_backward(K, N, M, splits):
    d = H.linear_bwd_inputs(M, K, N, seed=3)
    args = (d["dy"][0], d["y"][0], d["x"][0], d["w"][0], splits)
    r64, r32 = LO.linear_bwd(*args), LO.linear_bwd(*args, dtype=F32)
    S = LO.bwd_magnitudes(r64["dz"], d["x"][0], d["w"][0], splits)
    seen, fails = {}, []
    H.elementwise_check("linear rule", seen, fails, "bwd", "dx", _np(r32["dx_half"]), _np(r64["dx"]), _np(S["dx"]), N, True)
    H.elementwise_check("linear rule", seen, fails, "bwd", "wpart", _np(r32["wpart"]), _np(r64["wpart"]), _np(S["wpart"]),
                        M // splits, False)
    H.elementwise_check("linear rule", seen, fails, "bwd", "bpart", _np(r32["bpart"]), _np(r64["bpart"]), _np(S["bpart"]),
                        M // splits, False)
    # the documented order of the bias partials is one order of an f32 sum: inside the same bound
    H.elementwise_check("linear rule", seen, fails, "bwd", "bpart in the kernel's order", LO.bpart_kernel_order(r64["dz"], splits),
                        _np(r64["bpart"]), _np(S["bpart"]), M // splits, False)
    assert not fails, fails


@pytest.mark.parametrize("K", [4, 36, 68, 188, 1024])
def test_input_claims(K):
    """Between 25 % and 75 % of the pre-activations are negative; the special y values are where they are listed;
    dZ is exactly 0 where y == -1 and exactly dy where y is +-0; y is otherwise the reference's own fp16 ELU output."""
    M, N = 128, 128
    d = H.linear_bwd_inputs(M, K, N, seed=K, G=2)
    for g in range(2):
        z, _ = LO.linear_fwd(d["x"][g], d["w"][g], d["b"][g], 0)
        neg = float((z < 0).double().mean())
        assert 0.25 <= neg <= 0.75, (K, neg)
        z32 = LO.linear_fwd(d["x32"][g], d["w32"][g], d["b32"][g], 0, out_half=False)
        assert 0.25 <= float((z32 < 0).double().mean()) <= 0.75
        y, dy = d["y"][g], d["dy"][g]
        dz = LO.dz_of(dy, y)
        plain = torch.ones(M, N, dtype=torch.bool)
        for i, (name, (v, rows, cols)) in enumerate(H.linear_special_elements(M, N).items()):
            got = y[rows, cols]
            assert torch.equal(got.view(torch.int16), torch.full_like(got, v).view(torch.int16)), name
            plain[rows, cols] = False
            if name == "minus_one":
                assert bool((dz[rows, cols] == 0).all()) and bool((dy[rows, cols] != 0).any())
            if name in ("zero", "negzero", "max"):
                assert torch.equal(dz[rows, cols], dy[rows, cols].double())
            if name != "minus_one":
                row = dy[1 + i]
                assert int((row != 0).sum()) == 1 and bool(row[H.linear_single_term_column(i, N)] != 0)
        want = LO.linear_fwd(d["x"][g], d["w"][g], d["b"][g], 1)[1]
        assert torch.equal(y[plain], want[plain])
        assert float(y[plain].max()) > 0 > float(y[plain].min()) >= -1.0


def test_shape_lists_meet_the_documented_requirements_and_reach_the_branches():
    fwd = H.LIN_FWD_CASES
    for c in fwd:
        assert c["M"] % 64 == 0 and c["N"] % 128 == 0 and c["K"] % 4 == 0, c
        assert c.get("ldx", 0) % 4 == 0 and c.get("ldy", 0) % 4 == 0 and c.get("y_gstride", 0) % 4 == 0, c
        assert c.get("ldx", c["K"] * c["G"]) >= c["K"]
    tiles = {H.linear_fwd_tiles(c) for c in fwd}
    assert {1, 3, 5, 9, 13, 15} <= tiles and {t % 8 for t in tiles} >= {0, 1, 3, 5, 7} and min(tiles) < 8
    assert {c["K"] for c in fwd} >= {4, 36, 60, 64, 68, 128, 132, 188, 196}
    big = [c for c in fwd if (c["M"] // 128) * (c["N"] // 128) * c["G"] >= 256]
    assert {(c["M"], c["G"]) for c in big} == {(4096, 1), (1024, 8)}
    assert any(H.linear_fwd_tiles(c) == 62 * 8 for c in fwd)  # 248 tiles of 128 rows: the 64-row form
    # the direct-store arm: y or its row stride off the 16-byte grid
    assert sum(1 for c in fwd if c.get("y_off", 0) % 8 == 4 or c.get("ldy", 0) % 8 == 4 or c.get("y_gstride", 0) % 8 == 4) >= 3
    f32 = H.LIN_F32_CASES
    for c in f32:
        assert c["M"] % 64 == 0 and c["N"] % 64 == 0 and c["K"] % 4 == 0 and c.get("ldy", 0) % 4 == 0, c
    t32 = {H.linear_fwd_tiles(c, f32=True) for c in f32}
    assert {1, 3, 9, 15, 512, 528} <= t32
    assert {(c["K"], c["kstep"]) for c in f32 if "kstep" in c} == {(K, s) for K in (4, 28, 32, 36, 60, 64, 68, 188) for s in ("32", "64")}
    for c in H.LIN_DX_CASES:
        assert c["M"] % 128 == 0 and c["N"] % 128 == 0 and c["K"] % 128 == 0 and c.get("lddx", c["K"]) >= c["K"], c
        assert c.get("lddx", 0) % 4 == 0
    assert {H.linear_dx_tiles(c) for c in H.LIN_DX_CASES} >= {2, 6, 256, 496}
    assert {c.get("lddx", 0) % 8 for c in H.LIN_DX_CASES} >= {0, 4}
    for M, splits in H.LIN_DW_SPLITS:
        assert M % 128 == 0 and M % (64 * splits) == 0
    assert [M // s for M, s in H.LIN_DW_SPLITS] == [64, 128, 192, 384, 64]
    assert all(K % 4 == 0 for K in H.LIN_DW_K) and all(N % 128 == 0 for N in H.LIN_DW_N)
    assert set(H.SPLITK_PARTS) == {1, 15, 16, 17, 33} and {n % 4 for n in H.SPLITK_N} == {0, 3}


def test_kernel_order_sums_are_plain_float32_sums():
    rng = np.random.RandomState(0)
    parts = torch.from_numpy(rng.normal(size=(17, 260))).to(F32)
    got = LO.splitk_sum_kernel_order(parts)
    assert got.dtype == np.float32 and np.abs(got - _np(LO.splitk_sum(parts))).max() < 1e-5
    dz = torch.from_numpy(rng.normal(size=(128, 8))).to(F16)
    b = LO.bpart_kernel_order(dz, 2)
    assert b.shape == (2, 8) and np.abs(b - _np(dz.double().reshape(2, 64, 8).sum(1))).max() < 1e-5
