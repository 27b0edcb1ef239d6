"""The float64 reference of the PPO loss (oracle/ppo_oracle.py ppo_loss / ppo_heads_loss) and the minibatch
generator of its GPU tests (tests/helpers.py ppo_minibatch), checked on the CPU: the reference's autograd gradient
against central differences, the fp16 bound term, and that the generated minibatches populate every branch of the
loss and keep every row away from every branch boundary."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as O
from tests import helpers as H

E = H.PPO_E_CLIP
COEF = dict(critic_coef=2.0, entropy_coef=1e-3, bounds_loss_coef=1e-2)
NAMES = H.PPO_INPUTS
# (rows, actions) of tests/test_ppo_loss_gpu.py: rl_ppo_loss's and the heads kernels'
LOSS_SIZES = [(B, A) for B in (127, 128, 129, 385, 4357) for A in (1, 12, 32)]
HEADS_SIZES = [(200, 32, 1), (200, 32, 4), (200, 64, 8), (200, 128, 12), (200, 128, 16), (200, 256, 24),
               (200, 256, 32), (200, 64, 32), (4165, 128, 12), (4165, 256, 32)]
ONE_ROW_SEEDS = H.PPO_ONE_ROW_SEEDS


def _ref(mb, clip_value=1, mu_is_f16=None, dtype=None, **coef):
    f16 = mb["mu"].dtype == torch.float16 if mu_is_f16 is None else mu_is_f16
    return O.ppo_loss(*[mb[k] for k in NAMES], E, clip_value, *[dict(COEF, **coef)[k] for k in COEF], f16, dtype=dtype)


@pytest.mark.parametrize("clip_value", [0, 1])
def test_reference_gradient_matches_central_differences(clip_value):
    """B = 6, A = 3, bound loss off, the generator's points (away from every kink): autograd's d loss / d mu,
    d values, d logstd against (loss(x + h) - loss(x - h)) / 2h in float64.  h = 1e-6: truncation ~ h^2 |f'''| and
    cancellation ~ 1e-16 |loss| / h are both below 1e-9 here, against gradients of 1e-2 .. 1."""
    mb = {k: v.double() for k, v in H.ppo_minibatch(6, 3, seed=4).items()}
    ref = _ref(mb, clip_value, mu_is_f16=False, bounds_loss_coef=0.0)
    h = 1e-6
    for name, field in (("mu", "dmu"), ("values", "dvalues"), ("logstd", "dlogstd")):
        g = ref[field].reshape(-1)
        assert np.abs(g).max() > 1e-3, field
        fd = np.zeros_like(g)
        for k in range(g.size):
            lo_hi = []
            for sgn in (-1.0, 1.0):
                x = mb[name].clone()
                x.view(-1)[k] += sgn * h
                lo_hi.append(_ref(dict(mb, **{name: x}), clip_value, mu_is_f16=False, bounds_loss_coef=0.0)["loss"])
            fd[k] = (lo_hi[1] - lo_hi[0]) / (2 * h)
        assert np.abs(fd - g).max() <= 1e-7 * np.abs(g).max(), (field, fd, g)


def test_reference_bound_term_rounds_only_fp16_mu():
    """mu = 1.5, -3: with fp16 mu the bound term is torch's fp16 add (0.4 -> 0.39990234375, -1.9 -> -1.900390625),
    its gradient straight through; with f32 mu the plain sum."""
    mb = H.ppo_minibatch(1, 2, seed=0)
    for f16 in (True, False):
        mu = torch.tensor([[1.5, -3.0]], dtype=torch.float16 if f16 else torch.float32)
        ref = _ref(dict(mb, mu=mu), mu_is_f16=f16, bounds_loss_coef=1.0)
        zero = _ref(dict(mb, mu=mu), mu_is_f16=f16, bounds_loss_coef=0.0)
        lo, hi = (0.39990234375, -1.900390625) if f16 else (1.5 - 1.1, -3.0 + 1.1)
        assert ref["stats"][3] == pytest.approx(lo * lo + hi * hi, rel=1e-15)
        np.testing.assert_allclose(ref["dmu"] - zero["dmu"], [[2 * lo, 2 * hi]], rtol=1e-12)


def _margins(mb, ref):
    """The distance of every row from every branch boundary (all must hold for f32 and float64 to agree)."""
    r, d = ref["ratio"], ref["vdiff"]
    # the targets are 0.01 (1 % of a ratio of 1) or more from 1 -+ e; an f32 ratio is off by about 1e-5
    assert np.minimum(np.abs(r - (1 - E)), np.abs(r - (1 + E))).min() >= 0.0099
    adv = mb["advantages"].double().numpy()
    assert ((adv == 0) | (np.abs(adv) >= 0.1)).all()
    assert ((d == 0) | (np.abs(d) >= 0.09)).all() and np.abs(np.abs(d) - E).min() >= 0.09
    out = np.abs(d) > E
    assert (np.abs(ref["q1"] - ref["q2"])[out] >= 2 * 0.19 * 0.05).all()  # |q1 - q2| = 2 |v - v_clipped| |mid - R|
    mu = mb["mu"].double().numpy()
    assert np.abs(np.abs(mu) - 1.1).min() >= 0.02
    assert np.abs(mb["logstd"].numpy()).max() <= 0.5


def _assert_covered(c):
    assert (c["surrogate"] >= 1).all(), c
    assert (c["value"] >= 1).all() and (c["critic"] >= 1).all(), c
    assert (c["bound"] >= 1).all(), c


@pytest.mark.parametrize("B,A", LOSS_SIZES)
@pytest.mark.parametrize("f16", [False, True])
def test_generator_margins_and_branch_coverage(B, A, f16):
    mb = H.ppo_minibatch(B, A, seed=B + A, mu_f16=f16, values_f16=f16)
    ref = _ref(mb)
    _margins(mb, ref)
    assert 0.05 <= (mb["mu"].double().abs() > 1.1).double().mean() <= 0.15  # about a tenth beyond the soft bound
    _assert_covered(O.ppo_branch_counts(ref, mb["advantages"], E))
    # the float32 run of the reference takes the same branches
    c32 = O.ppo_branch_counts(_ref(mb, dtype=torch.float32), mb["advantages"], E)
    c64 = O.ppo_branch_counts(ref, mb["advantages"], E)
    assert all((c32[k] == c64[k]).all() for k in c64), (c32, c64)


def test_one_row_minibatches_cover_every_branch_together():
    """rows = 1 is one cell per minibatch: the union over the seeds the GPU test cycles through covers them all."""
    total = None
    for seed in ONE_ROW_SEEDS:
        mb = H.ppo_minibatch(1, 1, seed=seed)
        ref = _ref(mb)
        _margins(mb, ref)
        c = O.ppo_branch_counts(ref, mb["advantages"], E)
        total = c if total is None else {k: total[k] + c[k] for k in c}
    _assert_covered(total)


@pytest.mark.parametrize("B,Hd,A", HEADS_SIZES)
def test_heads_lattice_minibatches(B, Hd, A):
    """The lattice of the heads tests: mu and v exact in fp16, the margins, the branches (the bound's two sides
    need two far biases: A >= 8), and the reference's heads backward on given loss gradients."""
    heads, mb = H.ppo_heads_minibatch(B, Hd, A, seed=Hd + A)
    mu = heads["hidden_a"].double() @ heads["w_mu"].double().T + heads["b_mu"].double()
    assert torch.equal(mu, mb["mu"].double()) and torch.equal(mu * 256, (mu * 256).round())
    ref = _ref(mb)
    _margins(mb, ref)
    c = O.ppo_branch_counts(ref, mb["advantages"], E)
    assert (c["surrogate"] >= 1).all() and (c["value"] >= 1).all() and (c["critic"] >= 1).all(), c
    assert (c["bound"] >= 1).all() or A < 8, c
    full = O.ppo_heads_loss(*heads.values(), *[mb[k] for k in NAMES[2:]], E, 1, *COEF.values(), 1024.0)
    assert np.array_equal(full["mu"], mb["mu"].double().numpy()) and full["loss"] == ref["loss"]
    # d hidden_a without the fp16 roundings: within one fp16 rounding of d mu and one of the result
    want = (ref["dmu"] * 1024.0) @ heads["w_mu"].double().numpy()
    slack = 2.0 ** -10 * (np.abs(ref["dmu"] * 1024.0) @ np.abs(heads["w_mu"].double().numpy()) + np.abs(want)) + 2.0 ** -24
    assert (np.abs(full["dhidden_a"] - want) <= slack).all()
    np.testing.assert_allclose(full["grad_logstd"], ref["dlogstd"].astype(np.float32).astype(np.float64) * 1024.0)
