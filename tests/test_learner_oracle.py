"""The float64 references of the learner's bookkeeping kernels (oracle/learner_oracle.py) and the input generators of
their GPU tests (tests/helpers.py), checked on the CPU before they judge the kernels: the running moments against
the moments of the concatenated batches, Adam against torch.optim.Adam in float64, the KL against
torch.distributions, neglogp against Normal.log_prob, and what tests/test_learner_kernels_gpu.py relies on about
its inputs (how many elements sit on the clamp, where the scheduler's KL lies, that the values straddle +-5)."""
import math

import numpy as np
import pytest
import torch

from oracle import learner_oracle as O
from tests import helpers as H

F64, F32 = torch.float64, torch.float32
EPS = 1e-5
RMS_SHAPES, KL_SHAPES, HEADS_SHAPES = H.RMS_SHAPES, H.KL_SHAPES, H.ACT_HEADS_SHAPES


# ------------------------------------------------------------------------------------------------ running moments
def test_rms_reference_moments_are_the_moments_of_all_batches_plus_the_prior():
    """Three updates with different row counts from the module's initial state (mean 0, var 1, count 1): the
    running mean and variance equal the count-weighted moments of the prior and the concatenated batches.  The
    prior is one pseudo-sample at 0 whose own M2 is var * count = 1."""
    cols = 10
    mean, var, count = torch.zeros(cols, dtype=F64), torch.ones(cols, dtype=F64), 1.0
    batches = [H.rms_input(rows, cols, seed=s) for s, rows in enumerate((65, 2, 130))]
    for x in batches:
        mean, var, count, _ = O.rms_normalize(x, mean, var, count, EPS, True)
    allx = torch.cat(batches).double()
    n = allx.shape[0]
    assert count == n + 1
    want_mean = allx.sum(0) / (n + 1)  # the prior sample is 0
    # sum over batches of (unbiased var * rows) is not the pooled M2; the merge adds the between-batch terms:
    # together the pooled M2 about the pooled mean, where each batch's own M2 is var_unbiased * rows (rl_games'
    # convention: M2 = var * count with the unbiased var)
    m2, na, ma = torch.ones(cols, dtype=F64), 1.0, torch.zeros(cols, dtype=F64)
    for x in batches:
        xb = x.double()
        nb, mb = xb.shape[0], xb.mean(0)
        m2 = m2 + xb.var(0) * nb + (mb - ma) ** 2 * na * nb / (na + nb)
        ma = (ma * na + mb * nb) / (na + nb)
        na += nb
    scale = allx.abs().max(0).values + 1.0
    assert torch.allclose(mean, want_mean, rtol=0, atol=0) or float(((mean - want_mean).abs() / scale).max()) < 1e-14
    assert float(((var - m2 / (n + 1)).abs() / (m2 / (n + 1))).max()) < 1e-12
    # and against numpy's own restatement (oracle/ppo_oracle.py rms_merge)
    from oracle import ppo_oracle as P
    m, v, c = np.zeros(cols), np.ones(cols), 1.0
    for x in batches:
        m, v, c = P.rms_merge(m, v, c, x.numpy())
    assert np.allclose(mean.numpy(), m, rtol=1e-13, atol=0) and np.allclose(var.numpy(), v, rtol=1e-12, atol=0)


@pytest.mark.parametrize("update", [0, 1])
def test_rms_reference_y_is_the_clamp_formula(update):
    x = H.rms_input(130, 10, seed=3)
    mean0, var0, count0 = H.rms_state(10, 1000.0)
    mean, var, count, y = O.rms_normalize(x, mean0, var0, count0, EPS, update)
    if not update:
        assert torch.equal(mean, mean0) and torch.equal(var, var0) and count == count0
    want = ((x.double() - mean) / (var + EPS).sqrt()).clamp(-5, 5)
    assert y.dtype == F64 and torch.equal(y, want)
    y32 = O.rms_normalize(x, mean0, var0, count0, EPS, update, dtype=F32)[3]
    assert y32.dtype == F32
    want32 = ((x - mean.float()) / torch.sqrt(var.float() + EPS)).clamp(-5, 5)
    if not update:
        assert torch.equal(y32, want32)


def test_rms_reference_one_row_batch_has_variance_zero():
    """rows == 1: both references merge a batch variance of 0 (torch's var of one row is NaN), the kernel's
    documented behaviour."""
    x = H.rms_input(1, 3)
    for dt in (F64, F32):
        mean, var, count, y = O.rms_normalize(x, torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64), 1.0, EPS, True, dtype=dt)
        assert count == 2.0 and bool(torch.isfinite(var).all()) and bool(torch.isfinite(y).all())
        xd = x.double()[0]
        assert torch.allclose(mean, xd / 2, rtol=1e-15) and torch.allclose(var, (1 + xd * xd / 2) / 2, rtol=1e-15)


@pytest.mark.parametrize("rows,cols", RMS_SHAPES)
def test_rms_inputs_keep_the_clamp_decided(rows, cols):
    """Of every GPU-test input, after an update from the initial state and from the count = 100 and 1e9 states: under 1 % of
    the elements lie within RMS_CLAMP_MARGIN of the clamp (those alone are exempt from the exactness check), and
    the outlier columns reach beyond it (from 63 rows on; on both sides from 200 rows on)."""
    for seed in range(16):  # the GPU tests use seed rows % 16 and take err_f32 over all sixteen
        _rms_input_is_decided(rows, cols, seed)


def _rms_input_is_decided(rows, cols, seed):
    x = H.rms_input(rows, cols, seed=seed)
    for state in ((torch.zeros(cols, dtype=F64), torch.ones(cols, dtype=F64), 1.0), H.rms_state(cols, 100.0),
                  H.rms_state(cols, 1e9)):
        mean, var, _, _ = O.rms_normalize(x, *state, EPS, True)
        raw = (x.double() - mean) / (var + EPS).sqrt()
        near = ((raw.abs() - 5.0).abs() <= H.RMS_CLAMP_MARGIN)
        assert float(near.double().mean()) < 0.01
    if rows >= 63 and cols >= 5:  # (the state above: count 1e9, where the outliers stand out)
        out = raw[:, H.rms_kinds(cols) == 4]
        above, below = bool((out > 5.0 + H.RMS_CLAMP_MARGIN).any()), bool((out < -5.0 - H.RMS_CLAMP_MARGIN).any())
        assert (above and below) if rows >= 200 else (above or below)
    kinds = H.rms_kinds(cols)
    if cols >= 4:
        assert bool((x[:, kinds == 3] == H.RMS_CONSTANT).all())
    if cols >= 2 and rows > 1:
        off = x[:, kinds == 1].double()
        assert float((off.mean(0).abs() / off.std(0)).min()) > 5e3


# ------------------------------------------------------------------------------------------------ the optimizer
def _hyper(**over):
    return dict(O.OPT_HYPER, **over)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("max_norm", [0.0, 1e-3, 10.0])
def test_adam_reference_is_torch_adam_in_float64(weight_decay, max_norm):
    """Five steps without a scaler: clip_grad_norm_ (binding at 1e-3, not binding at 10, off at 0) and
    torch.optim.Adam in float64, with the f32-rounded hyperparameters the struct holds."""
    n, steps, lr = 257, 5, 3e-4
    h = _hyper(max_norm=max_norm, weight_decay=weight_decay)
    p, m, v = H.opt_state(n, 0)
    r = lambda x: float(np.float32(x))  # noqa: E731
    tp = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([tp], lr=r(lr), betas=(r(h["beta1"]), r(h["beta2"])), eps=r(h["eps"]),
                           weight_decay=r(weight_decay))
    step, binding = 0.0, []
    for k in range(steps):
        g = H.opt_grad(n, k)
        binding.append(float(g.double().norm()) > max_norm > 0)
        p, m, v, step, _, _, found = O.opt_step(p, g, m, v, step, lr, None, None, h)
        tp.grad = g.double().clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], r(max_norm))
        opt.step()
        assert not found and step == k + 1
        st = opt.state[tp]
        assert float((p - tp.detach()).abs().max()) <= 1e-13 * lr + 2.0 ** -51 * float(p.abs().max())  # + p's ulp
        for got, want in ((m, st["exp_avg"]), (v, st["exp_avg_sq"])):  # (the moments' elements cancel across steps)
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert all(binding) if max_norm == 1e-3 else not any(binding)


def test_adam_reference_unscales_and_skips_on_a_non_finite_gradient():
    n = 65
    p, m, v = H.opt_state(n, 1000)
    h = _hyper()
    g = H.opt_grad(n, 0)
    a = O.opt_step(p, g, m, v, 1000.0, 3e-4, None, None, h)
    b = O.opt_step(p, g * 1024.0, m, v, 1000.0, 3e-4, 1024.0, 7, h)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and b[3:] == (1001.0, 1024.0, 8, False)
    bad = (g * 1024.0).clone()
    bad[n - 1] = float("inf")
    c = O.opt_step(p, bad, m, v, 1000.0, 3e-4, 1024.0, 7, h)
    assert all(torch.equal(x, y.double()) for x, y in zip(c[:3], (p, m, v))) and c[3:] == (1000.0, 512.0, 0, True)
    d = O.opt_step(p, bad, m, v, 1000.0, 3e-4, None, None, h)  # no scaler: the step is taken
    assert d[3] == 1001.0 and d[6] and bool(torch.isnan(d[0][n - 1])) and bool(torch.isfinite(d[0][:n - 1]).all())


def test_scaler_transitions_are_the_known_answers():
    h = _hyper(growth_interval=3)
    assert O.scaler_update(65536.0, 2, True, h) == (32768.0, 0)       # backoff, whatever the tracker
    assert O.scaler_update(65536.0, 0, False, h) == (65536.0, 1)
    assert O.scaler_update(65536.0, 1, False, h) == (65536.0, 2)
    assert O.scaler_update(65536.0, 2, False, h) == (131072.0, 0)     # growth at the interval
    top = float(2.0 ** 127)
    assert O.scaler_update(top, 2, False, h) == (top, 0)              # no growth to inf; the tracker restarts
    assert O.scaler_update(top, 0, True, h) == (top / 2, 0)


# ------------------------------------------------------------------------------------------------ KL and scheduler
@pytest.mark.parametrize("sigma_mode", H.KL_SIGMA_MODES)
@pytest.mark.parametrize("kind", H.KL_KINDS)
def test_kl_reference_is_the_kl_of_the_two_normals(kind, sigma_mode):
    """Without the two 1e-5 terms: torch.distributions.kl_divergence(new || old), summed over A, mean over rows.
    With them: each element moves by at most 1e-5 / (s1 / s0) in the log and c2 1e-5 / s1^2 in the quotient."""
    M, A = 257, 12
    d = H.kl_inputs(M, A, kind, sigma_mode, seed=2)
    args = (d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], d["sigma_is_log"])
    bare = O.policy_kl(*args, eps_terms=False)
    s0 = d["sigma_new"].double().exp() if d["sigma_is_log"] else d["sigma_new"].double()
    new = torch.distributions.Normal(d["mu_new"].double(), s0.expand(M, A))
    old = torch.distributions.Normal(d["mu_old"].double(), d["sigma_old"].double())
    want = torch.distributions.kl_divergence(new, old).sum(-1).mean()
    assert abs(float(bare - want)) <= 1e-13 * max(1.0, abs(float(want)))
    full = O.policy_kl(*args)
    s1 = d["sigma_old"].double()
    c2 = (s0.expand(M, A) ** 2 + (d["mu_old"].double() - d["mu_new"].double()) ** 2) / (2 * s1 * s1)
    bound = (1e-5 / (s1 / s0.expand(M, A)) + c2 * 1e-5 / (s1 * s1)).sum(-1).mean()
    assert abs(float(full - bare)) <= float(bound) * (1 + 1e-9)
    if kind == "same":
        assert torch.equal(d["mu_new"].float(), d["mu_old"]) and abs(float(bare)) < 1e-6
    if kind == "near":
        assert 0 < float((d["mu_new"].double() - d["mu_old"].double()).abs().max()) < 1e-2
    assert O.policy_kl(*args, dtype=F32).dtype == F32


@pytest.mark.parametrize("M,A", KL_SHAPES)
def test_scheduler_inputs_keep_the_branch_decided(M, A):
    """The far inputs of the GPU tests: the float64 KL is positive, and every scheduler case keeps it at least 1 %
    (a factor of 2, in fact) from 2 thr and thr / 2, so an f32 KL takes the same branch."""
    d = H.kl_inputs(M, A, "far", "log", seed=M)
    kl = float(O.policy_kl(d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], 1))
    assert kl > 1e-4
    for thr, lr, want in H.kl_scheduler_cases(kl):
        assert abs(kl - 2 * thr) >= 0.01 * 2 * thr and abs(kl - thr / 2) >= 0.01 * thr / 2
        k, got = O.adaptive_lr(np.float32(kl), 1.0, 1, thr, lr)
        assert got == want and k == float(np.float32(kl))
    assert O.adaptive_lr(np.float32(kl), 1.0, 0, kl / 4, 3e-4)[1] == 3e-4  # not adaptive: untouched
    assert O.adaptive_lr(np.float32(kl), 0.25, 1, kl, 3e-4) == (float(np.float32(kl) * np.float32(0.25)), 3e-4 * 1.5)


# ------------------------------------------------------------------------------------------------ the act heads
@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("N,Hd,A", HEADS_SHAPES)
def test_heads_reference_neglogp_is_minus_log_prob(N, Hd, A, sharp):
    d = H.act_heads_inputs(N, Hd, A, seed=N, sharp=sharp)
    hid = d["hidden"]
    assert hid.shape == (N, 2 * Hd + 4) and bool(torch.isnan(hid[:, 2 * Hd:]).all())
    ha, hc = hid[:, :Hd], hid[:, Hd:2 * Hd]
    r = O.act_heads(ha, hc, d["w_mu"], d["b_mu"], d["w_v"], d["b_v"], d["noise"], d["logstd"])
    want = -torch.distributions.Normal(r["mu"], r["sigmas"]).log_prob(r["actions"]).sum(-1)
    assert float((r["neglogp"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(r["mu"], ha.double() @ d["w_mu"].double().T + d["b_mu"].double())
    assert torch.equal(r["value"], hc.double() @ d["w_v"].double() + d["b_v"].double()[0])
    n = O.act_heads(ha, hc, d["w_mu"], d["b_mu"], d["w_v"], d["b_v"], d["noise"], d["logstd"], d["vmean"], d["vvar"], EPS)
    assert torch.equal(n["value"], (d["vvar"][0] + EPS).sqrt() * r["value"].clamp(-5, 5) + d["vmean"][0])
    p = O.policy_head(r["mu"], r["value"], d["noise"], d["logstd"], d["vmean"], d["vvar"], EPS)
    assert all(torch.equal(p[k], n[k]) for k in p)
    if sharp:
        assert float(r["mu"].abs().min()) > 900 and float(r["sigmas"].max()) < 0.007
    assert O.act_heads(ha, hc, d["w_mu"], d["b_mu"], d["w_v"], d["b_v"], d["noise"], d["logstd"], dtype=F32)["neglogp"].dtype == F32


def test_heads_inputs_straddle_the_value_clamp():
    """Over the GPU tests' shapes with N >= 15, raw values fall on both sides of +5 and of -5 somewhere."""
    lo = hi = inside = 0
    for N, Hd, A in HEADS_SHAPES:
        d = H.act_heads_inputs(N, Hd, A, seed=N)
        v = d["hidden"][:, Hd:2 * Hd].double() @ d["w_v"].double() + d["b_v"].double()[0]
        lo, hi, inside = lo + int((v < -5).sum()), hi + int((v > 5).sum()), inside + int((v.abs() < 5).sum())
    assert lo > 0 and hi > 0 and inside > 0


# ------------------------------------------------------------------------------------------------ the column sum
@pytest.mark.parametrize("half", [False, True])
def test_colsum_reference(half):
    g, grad = H.colsum_inputs(65, 24, half)
    want = grad.double() + torch.stack([g[:, c].double().sum() for c in range(24)])
    assert torch.allclose(O.colsum(g, grad), want, rtol=1e-14, atol=1e-14) and bool((grad != 0).all())
    assert math.isfinite(float(O.colsum(g, grad, dtype=F32).sum()))
