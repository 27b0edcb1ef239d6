"""Matrix-core Linear + ELU oracle -- TEST INFRASTRUCTURE ONLY (imported by tests/ alone).

Plain torch-on-CPU restatements of the statements include/gymrl.h names for rl_linear_fwd(_g), rl_linear_fwd_f32_g,
rl_linear_bwd(_g), rl_linear_transpose and rl_splitk_accum(_multi).  Every function takes ``dtype``: float64 (the
default) is the reference, ``torch.float32`` the same statements in float32, and the pair measures what f32 rounding
alone does to each output.  The roundings the header states are made in both: y and dx are rounded once to fp16, and
dZ = fp16(f32(dy) * f32(y > 0 ? 1 : y + 1)) is one f32 product rounded once to fp16, which both gradients then use
(``round_dz=False`` switches that one rounding off so the rest can be compared with torch's autograd).  A grouped
call is a loop of these functions over strided views: the header defines a group as its own ungrouped call.

The magnitude sums (``fwd_magnitudes`` / ``bwd_magnitudes``: the same products on absolute values, in float64) are
what the per-element error bound of tests/helpers.py elementwise_check scales with.
"""
from __future__ import annotations

import numpy as np
import torch

F64, F32, F16 = torch.float64, torch.float32, torch.float16


def _cpu(x, dt):
    return torch.as_tensor(x).detach().to("cpu").to(dt)


def elu(z):
    """ELU with alpha = 1 in z's own dtype (expm1, as the kernel's epilogue)."""
    return torch.where(z > 0, z, torch.expm1(z))


def linear_fwd(x, w, bias, act, dtype=None, out_half=True):
    """z = x w^T + bias in `dtype` (bias None: none), y = ELU(z) if act.  x [M][K], w [N][K], bias [N]: the fp16 (or,
    for the f32 entry point, f32) tensors the kernel receives, widened.  out_half (the fp16 entry points): returns
    (y unrounded in `dtype`, fp16(y)); else (rl_linear_fwd_f32_g) y in `dtype`."""
    dt = dtype or F64
    z = _cpu(x, dt) @ _cpu(w, dt).t()
    if bias is not None:
        z = z + _cpu(bias, dt)
    y = elu(z) if act else z
    return (y, y.to(F16)) if out_half else y


def linear_fwd_half_accumulator(x, w, bias, act, every=16):
    """A deliberately WRONG forward: the accumulator passes through fp16 after every `every` terms (f32 arithmetic
    otherwise).  tests/test_linear_oracle.py shows that the elementwise rule refuses it.  Returns fp16(y)."""
    x32, w32 = _cpu(x, F32), _cpu(w, F32)
    acc = torch.zeros(x32.shape[0], w32.shape[0], dtype=F32)
    for k0 in range(0, x32.shape[1], every):
        acc = (acc + x32[:, k0:k0 + every] @ w32[:, k0:k0 + every].t()).to(F16).to(F32)
    if bias is not None:
        acc = acc + _cpu(bias, F32)
    return (elu(acc) if act else acc).to(F16)


def fwd_magnitudes(x, w, bias):
    """S_y = |x| |w|^T + |bias| in float64."""
    s = _cpu(x, F64).abs() @ _cpu(w, F64).abs().t()
    return s if bias is None else s + _cpu(bias, F64).abs()


def elu_backward_factor(y, dt):
    """ELU' from the layer's output (torch's elu_backward with is_result): 1 for y > 0, else y + 1."""
    y = _cpu(y, dt)
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def dz_of(dy, y, dtype=None, round_dz=True):
    """dZ.  round_dz: the f32 product rounded once to fp16, returned widened to `dtype` (the same numbers in float64
    and float32); else dy * ELU'(y) in `dtype`, unrounded."""
    dt = dtype or F64
    if round_dz:
        return (_cpu(dy, F32) * elu_backward_factor(y, F32)).to(F16).to(dt)
    return _cpu(dy, dt) * elu_backward_factor(y, dt)


def linear_bwd(dy, y, x, w, splits, dtype=None, round_dz=True):
    """The backward of linear_fwd with ELU from its output y.  dy, y [M][N], x [M][K], w [N][K] (None: no dx).
    Returns a dict: dz [M][N]; dx (unrounded, `dtype`) and dx_half = fp16(dx); wpart [splits][N][K] = dZ[blk]^T
    x[blk] and bpart [splits][N] = column sums of dZ[blk] over the row blocks of M / splits rows, in `dtype`."""
    dt = dtype or F64
    dz = dz_of(dy, y, dt, round_dz)
    M, N = dz.shape
    out = dict(dz=dz)
    if w is not None:
        out["dx"] = dz @ _cpu(w, dt)
        out["dx_half"] = out["dx"].to(F16)
    if splits:
        xb = _cpu(x, dt).reshape(splits, M // splits, -1)
        zb = dz.reshape(splits, M // splits, N)
        out["wpart"] = zb.transpose(1, 2) @ xb
        out["bpart"] = zb.sum(1)
    return out


def bwd_magnitudes(dz, x, w, splits):
    """S_dx = |dZ| |w|, S_w[s] = |dZ[blk]|^T |x[blk]|, S_b[s] = sum |dZ[blk]| in float64 (w / x None: skipped)."""
    az = _cpu(dz, F64).abs()
    M, N = az.shape
    out = {}
    if w is not None:
        out["dx"] = az @ _cpu(w, F64).abs()
    if splits:
        zb = az.reshape(splits, M // splits, N)
        if x is not None:
            out["wpart"] = zb.transpose(1, 2) @ _cpu(x, F64).abs().reshape(splits, M // splits, -1)
        out["bpart"] = zb.sum(1)
    return out


def bpart_kernel_order(dz, splits):
    """The bias partials as f32 sums of the rounded dZ in the order include/gymrl.h documents: per row block, sixteen
    row-group sums (group g: the block's rows r = g mod 16, ascending, from 0) added in ascending g from 0.  numpy
    float32, bit-comparable with the kernel.  dz [M][N] -> [splits][N] float32."""
    z = _cpu(dz, F32).numpy()
    M, N = z.shape
    R = M // splits
    out = np.zeros((splits, N), dtype=np.float32)
    for s in range(splits):
        blk = z[s * R:(s + 1) * R].reshape(R // 16, 16, N)
        grp = np.zeros((16, N), dtype=np.float32)
        for step in blk:
            grp = (grp + step).astype(np.float32)
        t = np.zeros(N, dtype=np.float32)
        for g in range(16):
            t = (t + grp[g]).astype(np.float32)
        out[s] = t
    return out


def splitk_sum(parts, dtype=None):
    """sum_p parts[p] ([P][n] fp16 / f32) in `dtype`."""
    return _cpu(parts, dtype or F64).sum(0)


def splitk_sum_kernel_order(parts):
    """The ascending f32 sum from 0 of the partials (include/gymrl.h rl_splitk_accum), numpy float32."""
    p = _cpu(parts, F32).numpy()
    acc = np.zeros(p.shape[1:], dtype=np.float32)
    for row in p:
        acc = (acc + row).astype(np.float32)
    return acc
