"""PPO learner oracle -- TEST INFRASTRUCTURE ONLY (imported by tests/ alone).

numpy restatement of rl_games' ``A2CBase.discount_values`` (rl_games/common/a2c_common.py,
rl-games 1.6.x; the reference requires rl-games>=1.6.0 at setup.py:22 and calls it through
isaacgymenvs/train.py:188-218 -- rl_games is absent from /root/reference and from this image,
so this restatement is PARITY UNPINNED against rl_games itself: no reference test or fixture
covers the learner).  float32 throughout, same association order as the torch loop, so the
result is bit-comparable with the HIP kernel (libgymrl.so, built with -ffp-contract=off).

Also the RunningMeanStd moment merge (rl_games/algos_torch/running_mean_std.py) in float64.

``ppo_loss`` / ``ppo_heads_loss``: rl_games' ``calc_gradients`` loss statements for the fixed-sigma
continuous model (a2c_continuous.py, models.py ModelA2CContinuousLogStd) in float64 on the CPU, the
gradients by torch autograd -- the reference of rl_ppo_loss / rl_ppo_heads_loss (include/gymrl.h).
``dtype=torch.float32`` runs the same statements in float32: the pair measures what f32 rounding
alone does to each output.
"""
from __future__ import annotations

import numpy as np


def discount_values(rewards, values, dones, last_values, last_dones, gamma: float, tau: float):
    """rewards/values f32 [H,N], dones u8 [H,N], last_* [N] -> advantages f32 [H,N]."""
    H = rewards.shape[0]
    f32 = np.float32
    g = f32(gamma)
    gt = f32(gamma * tau)
    advs = np.zeros_like(rewards, dtype=f32)
    lastgaelam = np.zeros(rewards.shape[1], dtype=f32)
    for t in reversed(range(H)):
        if t == H - 1:
            nn = f32(1.0) - last_dones.astype(f32)
            nv = last_values.astype(f32)
        else:
            nn = f32(1.0) - dones[t + 1].astype(f32)
            nv = values[t + 1]
        delta = (rewards[t] + (g * nv) * nn) - values[t]
        lastgaelam = delta + (gt * nn) * lastgaelam
        advs[t] = lastgaelam
    return advs


def env_major(x):
    """swap_and_flatten01: [H, N, ...] -> [N*H, ...]."""
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((x.shape[0] * x.shape[1],) + x.shape[2:])


def rms_merge(mean, var, count, batch):
    """RunningMeanStd._update_mean_var_count_from_moments with torch.var (unbiased) batch moments."""
    batch = batch.astype(np.float64)
    bm = batch.mean(0)
    bv = batch.var(0, ddof=1)
    bc = batch.shape[0]
    delta = bm - mean
    tot = count + bc
    new_mean = mean + delta * bc / tot
    m2 = var * count + bv * bc + delta ** 2 * count * bc / tot
    return new_mean, m2 / tot, tot


SOFT_BOUND = 1.1  # a2c_continuous.py bound_loss


def _cpu(x, dt):
    import torch
    return torch.as_tensor(x).detach().to("cpu").to(dt)


def fp16_bound_sum(mu_half, c):
    """``mu + c`` of an fp16 tensor and a Python scalar as torch's HIP / CUDA elementwise add computes it (the scalar
    stays f32, one rounding of the f32 sum to fp16) -- what ``mu + soft_bound`` is under autocast on the device.
    torch's CPU fp16 add rounds the scalar to fp16 first (1.1 -> 1.099609375: fp16(1.5) - 1.1 gives 0.400390625
    there and 0.39990234375 on the device), so it is spelled out; tests/test_ppo_loss_gpu.py pins it to the
    device's add bit for bit."""
    import torch
    return (mu_half.to(torch.float32) + torch.tensor(c, dtype=torch.float32)).to(torch.float16)


def ppo_loss(mu, values, logstd, actions, old_neglogp, advantages, old_values, returns, e_clip, clip_value,
             critic_coef, entropy_coef, bounds_loss_coef, mu_is_f16, dtype=None):
    """The minibatch loss of calc_gradients and its gradient by autograd, in `dtype` (float64) on the CPU.

    mu [B][A], values [B], logstd [A], actions [B][A], old_neglogp / advantages / old_values / returns [B]
    (arrays or tensors of any float type; their values are taken as they are).  mu_is_f16: mu came out of an
    autocast fp16 layer, so the bound term's ``mu + 1.1`` is torch's fp16 add (its result rounded to fp16, the
    gradient passing straight through); with f32 mu nothing is rounded.
    Returns a dict of float64 numpy: loss, stats [4] (means of the actor, critic, entropy, bound terms), dmu,
    dvalues, dlogstd (d loss / d input), and per row what decides the branches: ratio [B], vdiff = v - old_v [B],
    q1, q2 [B] (the two squared errors; None without clip_value), hi = mu + 1.1, lo = mu - 1.1 [B][A]."""
    import math
    import torch
    dt = dtype or torch.float64
    mu_ = _cpu(mu, dt).clone().requires_grad_(True)
    B, A = mu_.shape
    v_ = _cpu(values, dt).reshape(B).clone().requires_grad_(True)
    ls = _cpu(logstd, dt).reshape(A).clone().requires_grad_(True)
    x = _cpu(actions, dt).reshape(B, A)
    onlp, adv = _cpu(old_neglogp, dt).reshape(B), _cpu(advantages, dt).reshape(B)
    ov, R = _cpu(old_values, dt).reshape(B), _cpu(returns, dt).reshape(B)
    e = float(e_clip)
    # models.py ModelA2CContinuousLogStd.forward (is_train)
    sigma = torch.exp(ls)
    neglogp = 0.5 * torch.sum(((x - mu_) / sigma) ** 2, dim=-1) + 0.5 * math.log(2.0 * math.pi) * A + torch.sum(ls)
    entropy = torch.distributions.Normal(mu_, sigma.expand(B, A), validate_args=False).entropy().sum(dim=-1)
    # a2c_continuous.py calc_gradients, common.actor_loss / critic_loss / bound_loss
    ratio = torch.exp(onlp - neglogp)
    surr1 = adv * ratio
    surr2 = adv * torch.clamp(ratio, 1.0 - e, 1.0 + e)
    a_loss = torch.maximum(-surr1, -surr2)
    q1 = q2 = None
    if clip_value:
        vpc = ov + (v_ - ov).clamp(-e, e)
        q1, q2 = (v_ - R) ** 2, (vpc - R) ** 2
        c_loss = torch.maximum(q1, q2)
    else:
        c_loss = (R - v_) ** 2
    if mu_is_f16:
        mh = mu_.detach().to(torch.float16)
        assert torch.equal(mh.to(dt), mu_.detach()), "mu_is_f16 needs fp16-representable mu"
        # the device's fp16 add of a Python scalar: the f32 sum with f32(1.1), rounded to fp16 once (fp16_bound_sum)
        hi = mu_ + (fp16_bound_sum(mh, SOFT_BOUND).to(dt) - mu_).detach()
        lo = mu_ + (fp16_bound_sum(mh, -SOFT_BOUND).to(dt) - mu_).detach()
    else:
        hi, lo = mu_ + SOFT_BOUND, mu_ - SOFT_BOUND
    b_loss = (torch.clamp_max(hi, 0.0) ** 2 + torch.clamp_min(lo, 0.0) ** 2).sum(dim=-1)
    a_m, c_m, e_m, b_m = a_loss.mean(), c_loss.mean(), entropy.mean(), b_loss.mean()
    loss = a_m + 0.5 * c_m * critic_coef - e_m * entropy_coef + b_m * bounds_loss_coef
    dmu, dv, dls = torch.autograd.grad(loss, [mu_, v_, ls])
    n = lambda t: None if t is None else t.detach().to(torch.float64).numpy()  # noqa: E731
    return dict(loss=float(loss.detach().to(torch.float64)), stats=n(torch.stack([a_m, c_m, e_m, b_m])), dmu=n(dmu), dvalues=n(dv), dlogstd=n(dls),
                ratio=n(ratio), vdiff=n(v_ - ov), q1=n(q1), q2=n(q2), hi=n(hi), lo=n(lo))


def ppo_branch_counts(ref, advantages, e_clip):
    """How many rows / elements of a ppo_loss result sit in each branch of the loss:
    surrogate [3][3]: ratio below / inside / above [1 - e, 1 + e] x advantage negative / zero / positive;
    value [5]: v - old_v below -e, in [-e, 0), exactly 0, in (0, e], above e (zeros without clip_value);
    critic [2]: outside +-e, the unclipped / the clipped squared error is the larger; bound [2]: mu + 1.1 < 0,
    mu - 1.1 > 0."""
    e = float(e_clip)
    adv = np.asarray(advantages, dtype=np.float64).reshape(-1)
    r = ref["ratio"]
    band = np.where(r < 1.0 - e, 0, np.where(r > 1.0 + e, 2, 1))
    sign = np.where(adv < 0, 0, np.where(adv > 0, 2, 1))
    surrogate = np.zeros((3, 3), dtype=np.int64)
    np.add.at(surrogate, (band, sign), 1)
    value, critic = np.zeros(5, dtype=np.int64), np.zeros(2, dtype=np.int64)
    if ref["q1"] is not None:
        d = ref["vdiff"]
        case = np.where(d < -e, 0, np.where(d < 0, 1, np.where(d == 0, 2, np.where(d <= e, 3, 4))))
        np.add.at(value, case, 1)
        out = np.abs(d) > e
        critic[:] = [(out & (ref["q1"] > ref["q2"])).sum(), (out & (ref["q1"] < ref["q2"])).sum()]
    bound = np.array([(ref["hi"] < 0).sum(), (ref["lo"] > 0).sum()], dtype=np.int64)
    return dict(surrogate=surrogate, value=value, critic=critic, bound=bound)


def ppo_heads_loss(hidden_a, hidden_c, w_mu, b_mu, w_v, b_v, logstd, actions, old_neglogp, advantages, old_values,
                   returns, e_clip, clip_value, critic_coef, entropy_coef, bounds_loss_coef, scale, dtype=None,
                   grads=None):
    """The mu / value heads under autocast, ppo_loss, and the heads' backward with include/gymrl.h's fp16 rounding
    points (rl_ppo_heads_loss / rl_ppo_heads_loss_backward), sums and products in `dtype` (float64).

    hidden_a, hidden_c [B][H]: the actor / critic MLP outputs; w_mu [A][H], b_mu [A], w_v [H], b_v [1] (fp16 values).
    mu = fp16(hidden_a w_mu^T + b_mu), v = fp16(hidden_c w_v + b_v); the loss on them; then with s = scale:
    d mu = fp16(f32(dmu) s), d v = fp16(f32(dvalues) s), d hidden_a = fp16(d mu w_mu), d hidden_c = fp16(d v w_v),
    grad_w_mu = d mu^T hidden_a, grad_b_mu = sum d mu, grad_w_v = d v hidden_c, grad_b_v = sum d v,
    grad_logstd = f32(dlogstd) s.  grads = (dmu, dvalues, dlogstd): the f32 loss gradients the backward starts
    from, instead of this run's own (the backward as a function of its stated inputs).
    Returns ppo_loss's dict plus mu [B][A], values [B], dhidden_a, dhidden_c [B][H] and the five grad_*."""
    import torch
    dt = dtype or torch.float64
    f16, f32 = torch.float16, torch.float32
    ha, hc = _cpu(hidden_a, dt), _cpu(hidden_c, dt)
    B, H = ha.shape
    wm, bm = _cpu(w_mu, dt), _cpu(b_mu, dt).reshape(-1)
    wv, bv = _cpu(w_v, dt).reshape(H), _cpu(b_v, dt).reshape(())
    mu = (ha @ wm.T + bm).to(f16)
    v = (hc @ wv + bv).to(f16)
    out = ppo_loss(mu, v, logstd, actions, old_neglogp, advantages, old_values, returns, e_clip, clip_value,
                   critic_coef, entropy_coef, bounds_loss_coef, True, dtype=dt)
    g = grads if grads is not None else (out["dmu"], out["dvalues"], out["dlogstd"])
    s = float(scale)
    dmu_h = (_cpu(g[0], f32) * s).to(f16).to(dt)
    dv_h = (_cpu(g[1], f32).reshape(B) * s).to(f16).to(dt)
    n = lambda t: t.to(torch.float64).numpy()  # noqa: E731
    out.update(mu=n(mu), values=n(v), dhidden_a=n((dmu_h @ wm).to(f16)), dhidden_c=n((dv_h[:, None] * wv[None, :]).to(f16)),
               grad_w_mu=n(dmu_h.T @ ha), grad_b_mu=n(dmu_h.sum(0)), grad_w_v=n(dv_h @ hc), grad_b_v=n(dv_h.sum().reshape(1)),
               grad_logstd=n(_cpu(g[2], f32).to(dt) * s))
    return out
