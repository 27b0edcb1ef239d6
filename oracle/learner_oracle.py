"""Learner bookkeeping oracle -- TEST INFRASTRUCTURE ONLY (imported by tests/ alone).

Plain torch-on-CPU restatements of the statements include/gymrl.h names for rl_rms_normalize, rl_opt_step,
rl_policy_kl, rl_adaptive_lr, rl_act_heads / rl_policy_head and rl_colsum_accum (rl_games 1.6.x; see
oracle/ppo_oracle.py for how far rl_games itself is pinned).  Every function takes ``dtype``: float64 (the default)
is the reference, ``torch.float32`` the same statements in float32, and the pair measures what f32 rounding alone
does to each output.  Inputs are the f32 / fp16 tensors the kernel receives, widened to ``dtype``; state the ABI
holds in float64 (the running moments, the count, the learning rate) stays float64 in both.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
RMS_INIT = dict(mean=0.0, var=1.0, count=1.0)  # rl/running_mean_std.py RunningMeanStd.__init__


def _cpu(x, dt):
    return torch.as_tensor(x).detach().to("cpu").to(dt)


def _f32(x):
    """A Python float as the kernel's f32 argument sees it."""
    return float(np.float32(x))


def rms_normalize(x, mean, var, count, eps, update, dtype=None):
    """RunningMeanStd.forward of x [rows][cols] f32 on the float64 moments mean / var [cols] and count.

    update: the batch mean and unbiased variance over axis 0 are merged into the moments by
    _update_mean_var_count_from_moments, in float64, in its order of operations.  float64: the batch moments are
    taken in float64 and not rounded; float32: they are torch's float32 ``mean(0)`` / ``var(0)`` cast up, as
    rl_games computes them.  rows == 1: the batch variance is 0 in both (torch's ``var`` of one row is NaN, which
    would poison the running variance for good; the kernel's documented departure, include/gymrl.h).
    Then y = clamp((x - mean) / sqrt(var + eps), -5, 5) on the new moments: in float32 with their float32 casts, as
    the statement reads; in float64 with the moments as they are.
    Returns (mean, var: float64 tensors, count: float, y: tensor of `dtype`)."""
    dt = dtype or F64
    x32 = _cpu(x, F32)
    rows = x32.shape[0]
    mean, var, count = _cpu(mean, F64).clone(), _cpu(var, F64).clone(), float(count)
    if update:
        xb = x32.to(dt)
        bm = xb.mean(0).to(F64)
        bv = xb.var(0).to(F64) if rows > 1 else torch.zeros_like(bm)
        delta = bm - mean
        tot = count + rows
        new_mean = mean + delta * rows / tot
        m2 = var * count + bv * rows + delta ** 2 * count * rows / tot
        mean, var, count = new_mean, m2 / tot, tot
    y = (x32.to(dt) - mean.to(dt)) / torch.sqrt(var.to(dt) + torch.tensor(eps, dtype=dt))
    return mean, var, count, torch.clamp(y, -5.0, 5.0)


OPT_HYPER = dict(max_norm=1.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, backoff=0.5, growth=2.0,
                 growth_interval=2000)


def scaler_update(scale, tracker, found_inf, hyper):
    """torch._amp_update_scale_ on an f32 scale and an int32 tracker: (scale, tracker) after it."""
    if found_inf:
        return float(np.float32(scale) * np.float32(hyper["backoff"])), 0
    if tracker + 1 == hyper["growth_interval"]:
        with np.errstate(over="ignore"):
            grown = np.float32(scale) * np.float32(hyper["growth"])
        return (float(grown) if np.isfinite(grown) else float(scale)), 0
    return float(scale), tracker + 1


def opt_step(p, g, m, v, step, lr, scale, tracker, hyper, dtype=None):
    """One rl_opt_step (include/gymrl.h): scaler.unscale_, clip_grad_norm_, scaler.step(Adam), scaler.update.

    p, g, m, v [n] f32; step, lr: the f32 scalars' values; scale (None: no loss scaling; then tracker is None) and
    tracker: the GradScaler's f32 scale and int32 growth tracker; hyper: OPT_HYPER's keys (floats are taken as the
    f32 the struct holds).  The arithmetic on tensors and on the step's scalars runs in `dtype`.
    Returns (p, m, v: tensors of `dtype`, step, scale, tracker, found_inf)."""
    dt = dtype or F64
    p, g, m, v = (_cpu(t, dt).reshape(-1).clone() for t in (p, g, m, v))
    s = lambda x: torch.tensor(_f32(x), dtype=dt)  # noqa: E731
    h = {k: (s(x) if k != "growth_interval" else x) for k, x in hyper.items()}
    one = torch.tensor(1.0, dtype=dt)
    gu = g / s(scale) if scale is not None else g
    found = not bool(torch.isfinite(gu).all())
    if found and scale is not None:  # GradScaler.step skips the optimizer, Adam's step count stays
        ns, nt = scaler_update(scale, tracker, True, hyper)
        return p, m, v, float(step), ns, nt, True
    if hyper["max_norm"] > 0:
        coef = h["max_norm"] / (torch.sqrt((gu * gu).sum()) + s(1e-6))
        gu = gu * torch.clamp(coef, max=1.0)
    if hyper["weight_decay"] != 0:
        gu = gu + h["weight_decay"] * p
    t = s(step) + one
    m = m + (one - h["beta1"]) * (gu - m)
    v = h["beta2"] * v + (one - h["beta2"]) * gu * gu
    bc1, bc2 = one - torch.pow(h["beta1"], t), one - torch.pow(h["beta2"], t)
    p = p - (s(lr) / bc1) * (m / (torch.sqrt(v) / torch.sqrt(bc2) + h["eps"]))
    ns, nt = scaler_update(scale, tracker, False, hyper) if scale is not None else (None, None)
    return p, m, v, float(step) + 1.0, ns, nt, found


def policy_kl(mu_new, sigma_new, mu_old, sigma_old, sigma_is_log, dtype=None, eps_terms=True):
    """torch_ext.policy_kl: mean over the rows of sum over A of log(s1 / s0 + 1e-5) + (s0^2 + (m1 - m0)^2) /
    (2 (s1^2 + 1e-5)) - 0.5, m0 / s0 the new policy, m1 / s1 the old; sigma_new [A] or [M][A], its log when
    sigma_is_log.  eps_terms False: without the two 1e-5 (the KL of the two normals proper).  A 0-d tensor."""
    dt = dtype or F64
    m0, m1, s1 = _cpu(mu_new, dt), _cpu(mu_old, dt), _cpu(sigma_old, dt)
    s0 = _cpu(sigma_new, dt)
    if sigma_is_log:
        s0 = torch.exp(s0)
    s0 = s0.expand_as(m0)
    e = torch.tensor(1e-5 if eps_terms else 0.0, dtype=dt)
    c1 = torch.log(s1 / s0 + e)
    c2 = (s0 * s0 + (m1 - m0) ** 2) / (2.0 * (s1 * s1 + e))
    return (c1 + c2 - 0.5).sum(dim=-1).mean()


LR_MIN, LR_MAX = 1e-6, 1e-2  # schedulers.AdaptiveScheduler


def adaptive_lr(kl, inv_world, adaptive, thr, lr):
    """schedulers.AdaptiveScheduler on kl * inv_world (kl: the f32 scalar's value; lr float64): (kl, lr)."""
    k = float(np.float32(kl) * np.float32(inv_world)) if inv_world != 1.0 else float(np.float32(kl))
    lr = float(lr)
    if adaptive:
        nxt = lr
        if k > 2.0 * thr:
            nxt = max(lr / 1.5, LR_MIN)
        if k < 0.5 * thr:
            nxt = min(lr * 1.5, LR_MAX)
        lr = nxt
    return k, lr


def policy_head(mu, value, noise, logstd, vmean=None, vvar=None, veps=1e-5, dtype=None):
    """ModelA2CContinuousLogStd's eval forward after the network: sigma = exp(logstd), actions = noise sigma + mu,
    neglogp of the actions, value unnormalised by the value RunningMeanStd (vmean / vvar: its float64 moments;
    float32 uses their float32 casts, as the statement reads).  dict of mu, actions, sigmas [N][A], neglogp, value [N]."""
    dt = dtype or F64
    mu, noise, ls = _cpu(mu, dt), _cpu(noise, dt), _cpu(logstd, dt).reshape(-1)
    N, A = mu.shape
    sigma = torch.exp(ls).expand(N, A)
    actions = noise * sigma + mu
    neglogp = 0.5 * (((actions - mu) / sigma) ** 2).sum(dim=-1) + 0.5 * math.log(2.0 * math.pi) * A + ls.sum(dim=-1)
    value = _cpu(value, dt).reshape(N)
    if vmean is not None:
        vm, vv = _cpu(vmean, F64).reshape(()).to(dt), _cpu(vvar, F64).reshape(()).to(dt)
        value = torch.sqrt(vv + torch.tensor(veps, dtype=dt)) * torch.clamp(value, -5.0, 5.0) + vm
    return dict(mu=mu, actions=actions, sigmas=sigma.contiguous(), neglogp=neglogp, value=value)


def act_heads(hidden_a, hidden_c, w_mu, b_mu, w_v, b_v, noise, logstd, vmean=None, vvar=None, veps=1e-5, dtype=None):
    """The two Linear heads, mu = hidden_a w_mu^T + b_mu and value = hidden_c w_v + b_v, then policy_head."""
    dt = dtype or F64
    mu = _cpu(hidden_a, dt) @ _cpu(w_mu, dt).T + _cpu(b_mu, dt).reshape(-1)
    value = _cpu(hidden_c, dt) @ _cpu(w_v, dt).reshape(-1) + _cpu(b_v, dt).reshape(())
    return policy_head(mu, value, noise, logstd, vmean, vvar, veps, dtype=dt)


def colsum(g, grad, dtype=None):
    """grad + the column sums of g [rows][cols] (the bias gradient of a Linear layer)."""
    dt = dtype or F64
    return _cpu(grad, dt).reshape(-1) + _cpu(g, dt).sum(0)
