"""The policy player on the GPU: rl_policy_infer and rl_play_post at the C ABI (include/gymrl.h, csrc/rl_infer.hip),
PpoPlayerContinuous against the learner's own model, and train.launch(test=True) end to end.

rl_policy_infer is held to the rule of tests/test_linear_kernels_gpu.py (tests/helpers.py field_check), per output
field (actions, mu):
    max|kernel - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|
ref64: the header's statements in float64 on the CPU, computed here (the inputs of the statements are what the
kernel is handed: f32 observations and parameters, and float(mean), float(var), float(eps) of the float64 moments --
the header's own casts); ref32: the same statements in torch float32 on the CPU; err_f32 = max|ref32 - ref64| is the
largest over the three seeds of the shape and weight scale, and the kernel is run and judged on each of the three.
Weights are uniform in +-g / sqrt(K) with g = 1, 2, 3 (three seeds each), and the observations reach the +-5 clamp of
the normalisation.  Shapes: the smallest at which the tiling can go wrong (the four networks below x num_envs 1, 31,
32, 33, 64, 65, and 15, 16, 17 around the kernel's own 16-row tile), each with and
without normalisation, deterministic and with noise, with and without clip.  Beyond the rule: in noise mode the
actions equal f32 noise * sigma + mu bit for bit, with the kernel's own mu and sigma = the device's f32 exp(logstd)
as rl_policy_head writes it (and equal rl_policy_head's own actions); every element outside [N][A] of the over-
allocated outputs keeps its NaN sentinel; two calls give the same bits; integer-valued inputs give the exact integers;
each refusal is nonzero, names its limit and writes nothing.

MEASURED on an MI355X (58 tests in 8.8 s): the largest err_kernel / bar (<= 1 passes) over every case of a network,
as the [player] lines of test_policy_infer_matches_float64_reference print it (actions, mu):
    AnymalTerrain-like 0.36, 0.36   small 0.62, 0.62   Cartpole-like 0.33, 0.33   odd K, 18 actions 0.51, 0.50
    player against the learner's model: Cartpole 0.16   AnymalTerrain 0.16
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests.test_player_cpu import PlayPostReference, play_streams

pytestmark = pytest.mark.gpu

NETS = {"anymal": (188, [512, 256, 128], 12), "small": (60, [256, 128, 64], 8), "cartpole": (4, [32, 32], 1),
        "odd": (133, [512, 256, 128], 18)}
ENVS = [1, 15, 16, 17, 31, 32, 33, 64, 65]  # the tile is 16 rows: both sides of one and of two tiles, 4 tiles (+ 1)
EPS = 1e-5
GUARD = 64
SEEN = {}


def _draw(net, N, seed, g=1.0):
    """One draw of a network's parameters (weights uniform in +-g / sqrt(K)) and an observation batch (CPU tensors)."""
    O, hidden, A = NETS[net]
    rng = np.random.RandomState(1000 * seed + 7 * N + O + 100000 * int(g))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    d = {"W": [], "b": []}
    K = O
    for n in hidden:
        d["W"].append(f(rng.uniform(-1, 1, (n, K)) * g / math.sqrt(K)))
        d["b"].append(f(rng.uniform(-0.5, 0.5, n)))
        K = n
    d["w_mu"] = f(rng.uniform(-1, 1, (A, K)) * g / math.sqrt(K))
    d["b_mu"] = f(rng.uniform(-0.5, 0.5, A))
    d["logstd"] = f(rng.uniform(-1.5, 0.5, A))
    d["noise"] = f(rng.randn(N, A))
    d["mean"] = torch.from_numpy(rng.randn(O) * 2.0)
    d["var"] = torch.from_numpy(rng.uniform(0.05, 4.0, O))
    # observations 3 sigma wide around the mean: a few per cent of them beyond the +-5 clamp of the normalised value
    d["obs"] = f(d["mean"].numpy() + 3.0 * np.sqrt(d["var"].numpy()) * rng.randn(N, O))
    return d


def _ref(d, dtype, norm, noise, clip):
    """include/gymrl.h rl_policy_infer's statements in `dtype` on the CPU: (actions, mu)."""
    y = d["obs"].to(dtype)
    if norm:
        m, v = d["mean"].float().to(dtype), d["var"].float().to(dtype)
        eps = torch.tensor(EPS, dtype=torch.float32).to(dtype)
        y = torch.clamp((y - m) / torch.sqrt(v + eps), -5.0, 5.0)
    for W, b in zip(d["W"], d["b"]):
        y = F.elu(y @ W.to(dtype).T + b.to(dtype))
    mu = y @ d["w_mu"].to(dtype).T + d["b_mu"].to(dtype)
    a = mu
    if noise:
        a = d["noise"].to(dtype) * torch.exp(d["logstd"].to(dtype)) + mu
    if clip:
        a = torch.clamp(a, -1.0, 1.0)
    return a, mu


def _guarded(n):
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


def _call(dev, N, norm, noise, actions, mu, clip=False, **over):
    """One rl_policy_infer call on device tensors `dev`; `over` replaces arguments (the refusals)."""
    from isaacgymenv_amd.rl import gae
    O = dev["obs"].shape[1] if dev["obs"] is not None else 1
    a = dict(obs=dev["obs"], num_envs=N, obs_dim=O, mean=dev["mean"] if norm else None,
             var=dev["var"] if norm else None, eps=EPS, widths=[w.shape[0] for w in dev["W"]], weights=dev["W"],
             biases=dev["b"], w_mu=dev["w_mu"], b_mu=dev["b_mu"], num_actions=dev["w_mu"].shape[0],
             noise=dev["noise"] if noise else None, logstd=dev["logstd"], clip=clip, actions=actions, mu=mu, check=False)
    a.update(over)
    return gae.policy_infer(**a)


def _to_dev(d):
    return {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in d.items()}


def _device_sigma(dev, N):
    """exp(logstd) as the device's f32 expf gives it: rl_policy_head's sigmas row (pinned in
    tests/test_learner_kernels_gpu.py), and that kernel's actions for the same mu / noise."""
    from isaacgymenv_amd.rl import gae
    A = dev["logstd"].numel()

    def head(mu):
        actions, sigmas, _, _ = gae.policy_head(mu.contiguous(), dev["noise"], dev["logstd"],
                                                torch.zeros(N, device="cuda"))
        return actions, sigmas[0].clone()
    return head, A


@pytest.mark.parametrize("N", ENVS)
@pytest.mark.parametrize("net", sorted(NETS))
def test_policy_infer_matches_float64_reference(net, N):
    O, hidden, A = NETS[net]
    fails = []
    for g, norm in [(g, norm) for g in (1.0, 2.0, 3.0) for norm in (False, True)]:
        draws = [_draw(net, N, s, g) for s in range(3)]
        refs = [(_ref(d, torch.float64, norm, False, False), _ref(d, torch.float32, norm, False, False)) for d in draws]
        err_mu = max(float((r32[1].double() - r64[1]).abs().max()) for r64, r32 in refs)
        for s, d in enumerate(draws):
            dev = _to_dev(d)
            head, _ = _device_sigma(dev, N)
            for noise in (False, True):
                for clip in (False, True):
                    what = f"{net} N={N} g={g:g} seed={s} norm={norm} noise={noise} clip={clip}"
                    out = [(_guarded(N * A), _guarded(N * A)) for _ in range(2)]
                    for actions, mu in out:
                        assert _call(dev, N, norm, noise, actions, mu, clip) == 0, what
                    torch.cuda.synchronize()
                    (a1, m1), (a2, m2) = [(a.cpu(), m.cpu()) for a, m in out]
                    assert H.same_bits(a1, a2) and H.same_bits(m1, m2), f"{what}: two calls differ"
                    assert torch.isnan(a1[N * A:]).all() and torch.isnan(m1[N * A:]).all(), f"{what}: guard written"
                    a_k, mu_k = a1[:N * A].reshape(N, A), m1[:N * A].reshape(N, A)
                    if noise:  # bit for bit: f32 noise * sigma (rounded) + mu (rounded), from the kernel's own mu
                        h_actions, sigma = head(mu_k.cuda())
                        sigma = sigma.cpu()
                        exp = d["noise"] * sigma + mu_k
                        h_actions = h_actions.cpu()
                        if clip:
                            exp, h_actions = torch.clamp(exp, -1.0, 1.0), torch.clamp(h_actions, -1.0, 1.0)
                        assert torch.equal(a_k, exp), f"{what}: actions != f32 noise * sigma + mu"
                        assert torch.equal(a_k, h_actions), f"{what}: actions != rl_policy_head's"
                    elif not clip:
                        assert torch.equal(a_k, mu_k), f"{what}: deterministic actions != mu"
                    a64, m64 = _ref(d, torch.float64, norm, noise, clip)
                    a32, m32 = _ref(d, torch.float32, norm, noise, clip)
                    err_a = max(err_mu, float((a32.double() - a64).abs().max()))
                    H.field_check("player", SEEN.setdefault(net, {}), fails, what, "mu", mu_k, m64, m32, err_32=err_mu)
                    H.field_check("player", SEEN.setdefault(net, {}), fails, what, "actions", a_k, a64, a32, err_32=err_a)
            # without the optional mu output: the same actions, nothing else
            actions = _guarded(N * A)
            assert _call(dev, N, norm, False, actions, None) == 0
            assert torch.equal(actions[:N * A].cpu(), mu_k.reshape(-1)) and torch.isnan(actions[N * A:]).all()
    print(f"[player] {net} N={N}: largest err_kernel / bar "
          + ", ".join(f"{k} {v[1]:.3g}" for k, v in sorted(SEEN[net].items())))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", [33, 65])
def test_policy_infer_exact_on_integers(N):
    """Integer-valued inputs and parameters with every partial sum below 2^24 (non-negative up to the mu head, whose
    absolute sum is checked): the f32 result is the exact integer result, whatever the order of the sums."""
    O, hidden, A = NETS["odd"]
    rng = np.random.RandomState(5)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    d = {"obs": f(rng.randint(0, 4, (N, O))), "W": [], "b": []}
    K = O
    for n in hidden:
        d["W"].append(f(rng.rand(n, K) < 0.05))
        d["b"].append(f(rng.randint(1, 3, n)))
        K = n
    d["w_mu"] = f(rng.randint(-1, 2, (A, K)))
    d["b_mu"] = f(rng.randint(-3, 4, A))
    d["logstd"], d["noise"] = torch.zeros(A), torch.zeros(N, A)
    d["mean"], d["var"] = torch.zeros(O, dtype=torch.float64), torch.ones(O, dtype=torch.float64)
    y = d["obs"].double()
    for W, b in zip(d["W"], d["b"]):
        y = y @ W.double().T + b.double()
        assert float(y.min()) > 0 and float(y.max()) < 2 ** 24
    assert float((y @ d["w_mu"].double().abs().T).max()) + 3 < 2 ** 24
    want = y @ d["w_mu"].double().T + d["b_mu"].double()
    dev = _to_dev(d)
    actions, mu = _guarded(N * A), _guarded(N * A)
    assert _call(dev, N, False, False, actions, mu) == 0
    got = mu[:N * A].cpu().double().reshape(N, A)
    assert torch.equal(got, want) and torch.equal(actions[:N * A].cpu().double().reshape(N, A), want)
    assert float(want.abs().max()) > 1000


REFUSALS = [("obs_dim 257", dict(obs_dim=257), "obs_dim"), ("width 48", dict(widths=[48, 32]), "widths"),
            ("width 544", dict(widths=[544, 32]), "widths"), ("5 layers", "five", "layers"),
            ("num_actions 33", dict(num_actions=33), "num_actions"), ("num_envs 0", dict(num_envs=0), "num_envs"),
            ("null obs", dict(obs=None), "null"), ("null actions", "null_actions", "null"),
            ("null w_mu", dict(w_mu=None), "null"), ("null layer weight", "null_weight", "null")]


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_policy_infer_refusals_name_the_limit_and_write_nothing(what, over, word):
    from isaacgymenv_amd.rl import gae
    N = 8
    dev = _to_dev(_draw("cartpole", N, 0))
    # buffers large enough for whatever the refused call claims
    dev["obs"] = torch.zeros(N, 257, device="cuda")
    big = torch.zeros(544 * 544, device="cuda")
    actions, mu = _guarded(N * 33), _guarded(N * 33)
    base = dict(weights=[big, big], biases=[big, big], w_mu=big, b_mu=big, obs_dim=4)
    if over == "five":
        over = dict(widths=[32] * 5, weights=[big] * 5, biases=[big] * 5)
    elif over == "null_weight":
        over = dict(weights=[big, None])
    if over == "null_actions":
        rc = _call(dev, N, False, False, None, mu, **base)
    else:
        rc = _call(dev, N, False, False, actions, mu, **{**base, **over})
    msg = gae.lib().rl_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0, what
    assert "rl_policy_infer" in msg and word in msg, (what, msg)
    assert torch.isnan(actions).all() and torch.isnan(mu).all(), f"{what}: outputs written"
    # the same call within the limits goes through (the refusal is the limit's, not the harness's)
    assert _call(dev, N, False, False, actions, mu, **base) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(actions[:N]).all() and torch.isnan(actions[N:]).all()


@pytest.mark.parametrize("flag_dtype", [torch.bool, torch.int64], ids=["bool", "int64"])
@pytest.mark.parametrize("N", [1, 5, 70])
def test_play_post_matches_the_restatement(N, flag_dtype):
    from isaacgymenv_amd.rl import gae
    steps, games_num = 40, 7
    rew, done = play_streams(N, steps, seed=100 + N)
    tail_rew, tail_done = play_streams(N, 10, seed=200 + N)
    if N > 1:
        assert (done.sum(1) > 1).any(), "no step where several envs finish together"
    ref = PlayPostReference(N, games_num)
    cr, cs = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    games = torch.zeros(2, dtype=torch.int64, device="cuda")

    def step(r, d, what):
        ref.step(r, d)
        gae.play_post(torch.from_numpy(r).cuda(), torch.from_numpy(d).to(flag_dtype).cuda(), cr, cs, sums, games,
                      games_num)
        g, s = games.tolist(), sums.tolist()
        assert g == [ref.games_played, int(ref.finished)], what
        np.testing.assert_array_equal(cs.cpu().numpy(), ref.cur_steps, err_msg=what)
        np.testing.assert_array_equal(cr.cpu().numpy(), ref.cur_rewards, err_msg=what)
        assert abs(s[0] - ref.sum_rewards) <= 1e-12 * abs(ref.sum_rewards), what
        assert s[1] == ref.sum_steps, what
        return H.bits(sums).tolist(), g

    crossing = None
    for t in range(steps):
        was = ref.finished
        step(rew[t], done[t], f"step {t}")
        if ref.finished and not was:
            crossing = int(done[t].sum())
    if N > 1:
        assert ref.finished and crossing is not None
    if N == 70:
        assert crossing > 1 and ref.games_played > games_num  # every env of the crossing step counted
    extra = 0
    while not ref.finished:  # (one env at p = 0.2 may not finish 7 episodes in 40 steps: every further step ends one)
        step(np.full(N, 0.5, dtype=np.float32), np.ones(N, dtype=bool), f"extra step {extra}")
        extra += 1
    frozen = (H.bits(sums).tolist(), games.tolist())
    for t in range(10):
        assert step(tail_rew[t], tail_done[t], f"tail step {t}") == frozen, f"tail step {t}: totals moved after finished"


def test_play_post_refusals():
    from isaacgymenv_amd.rl import gae
    L = gae.lib()
    z = torch.zeros(8, device="cuda")
    p = z.data_ptr()
    assert L.rl_play_post(p, p, 1, 0, p, p, p, p, 7, None) != 0 and b"num_envs" in L.rl_last_error()
    assert L.rl_play_post(p, None, 1, 2, p, p, p, p, 7, None) != 0 and b"null" in L.rl_last_error()
    assert L.rl_play_post(p, p, 4, 2, p, p, p, p, 7, None) != 0 and b"dones" in L.rl_last_error()
    torch.cuda.synchronize()
    assert not z.any()


# ---------------------------------------------------------------- the player against the learner's own model
def _agent(task, num_envs):
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    import isaacgymenvs
    vec_task.EXISTING_SIM = None
    cfg = compose("config", [f"task={task}"])
    env = isaacgymenvs.make(seed=42, task=task, num_envs=num_envs, sim_device="cuda:0", rl_device="cuda:0",
                            headless=True, force_render=False)
    horizon = int(cfg["train"]["params"]["config"]["horizon_length"])
    pcfg = PpoConfig.from_train_cfg(cfg["train"], minibatch_size=horizon * num_envs)
    return A2CAgent(env, pcfg, device="cuda:0", seed=42)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """task -> (agent after one epoch, its checkpoint path), built once per task."""
    made = {}

    def get(task):
        if task not in made:
            agent = _agent(task, 64)
            agent.train_epoch()
            path = str(tmp_path_factory.mktemp(task) / f"{task}.pth")
            agent.save(path)
            made[task] = (agent, path)
        return made[task]
    return get


def _model_ref(sd, obs, dtype, clip):
    """The eval forward's mus from a ModelA2CContinuousLogStd state dict, in `dtype` on the CPU."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    y = obs.cpu().to(dtype)
    if "running_mean_std.running_mean" in sd:
        m, v = sd["running_mean_std.running_mean"].float().to(dtype), sd["running_mean_std.running_var"].float().to(dtype)
        y = torch.clamp((y - m) / torch.sqrt(v + torch.tensor(EPS, dtype=torch.float32).to(dtype)), -5.0, 5.0)
    i = 0
    while f"a2c_network.actor_mlp.{i}.weight" in sd:
        y = F.elu(y @ sd[f"a2c_network.actor_mlp.{i}.weight"].to(dtype).T + sd[f"a2c_network.actor_mlp.{i}.bias"].to(dtype))
        i += 2
    assert i > 0
    mu = y @ sd["a2c_network.mu.weight"].to(dtype).T + sd["a2c_network.mu.bias"].to(dtype)
    return torch.clamp(mu, -1.0, 1.0) if clip else mu


@pytest.mark.parametrize("task", ["Cartpole", "AnymalTerrain"])
def test_player_matches_the_learners_model(task, trained):
    from isaacgymenv_amd.rl import PpoPlayerContinuous
    agent, path = trained(task)
    rms = agent.model.running_mean_std
    assert float(rms.count) > 1.0 and float(rms.running_mean.abs().max()) > 0  # the moments have moved
    player = PpoPlayerContinuous(agent.env, agent.cfg, device="cuda:0", seed=1, games_num=4)
    player.restore(path)
    want, got = agent.model.state_dict(), player.model.state_dict()
    assert list(want) == list(got)
    for k in want:
        assert want[k].dtype == got[k].dtype and torch.equal(want[k], got[k]), k
    obs = agent._obs(agent.obs).clone()
    assert obs.shape == (64, agent.obs_dim)
    # err_f32 over three batches: the env's own and two drawn from the running moments, 3 sigma wide
    gen = torch.Generator().manual_seed(3)
    m, sd = rms.running_mean.cpu(), rms.running_var.cpu().sqrt()
    batches = [obs.cpu()] + [(m + 3.0 * sd * torch.randn(64, agent.obs_dim, generator=gen, dtype=torch.float64)).float()
                             for _ in range(2)]
    clip = agent.cfg.clip_actions
    refs = [(_model_ref(want, b, torch.float64, clip), _model_ref(want, b, torch.float32, clip)) for b in batches]
    err32 = max(float((r32.double() - r64).abs().max()) for r64, r32 in refs)
    fails = []
    seen = SEEN.setdefault("player " + task, {})
    for b, (r64, r32) in zip(batches, refs):
        a = player.get_action(b.cuda(), True)
        assert player.last_path == "rl_policy_infer"
        H.field_check("player", seen, fails, f"{task} player", "actions", a.cpu(), r64, r32, err_32=err32)
    print(f"[player] {task} player vs learner: largest err_kernel / bar {seen['actions'][1]:.3g}")
    assert not fails, "\n".join(fails)
    # what does not fit the kernel's input contract takes the model's own forward, and agrees with it
    a_k = player.get_action(obs, True)
    a_t = player.get_action(obs.double().float().t().contiguous().t(), True)  # not contiguous
    assert player.last_path == "torch"
    assert float((a_k - a_t).abs().max()) <= 1e-4 * max(1.0, float(a_k.abs().max()))
    # sampled play: clamped where the config clips, and not the mean
    a_s = player.get_action(obs, False)
    assert player.last_path == "rl_policy_infer" and not torch.equal(a_s, a_k)
    if clip:
        assert float(a_s.abs().max()) <= 1.0


def test_launch_test_true_plays_the_checkpoint(trained, monkeypatch, tmp_path):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    from isaacgymenv_amd.isaacgymenvs.train import launch
    from isaacgymenv_amd.rl import PpoPlayerContinuous
    agent, path = trained("Cartpole")
    before = open(path, "rb").read()
    repo_runs = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runs")
    had_runs = os.path.exists(repo_runs)
    monkeypatch.chdir(tmp_path)
    vec_task.EXISTING_SIM = None
    lines = []
    player, stats = launch(["task=Cartpole", "test=True", f"checkpoint={path}", "num_envs=64"], printer=lines.append,
                           games_num=16)
    assert isinstance(player, PpoPlayerContinuous) and player.last_path == "rl_policy_infer"
    assert stats["games_played"] >= 16 and math.isfinite(stats["av_reward"]) and math.isfinite(stats["av_steps"])
    assert stats["av_steps"] >= 1.0 and stats["steps"] % 16 == 0
    assert any(l.startswith("av reward:") for l in lines)
    assert open(path, "rb").read() == before
    assert not os.path.exists(tmp_path / "runs") and os.path.exists(repo_runs) == had_runs
    ckpt = torch.load(path, map_location="cuda:0", weights_only=True)["model"]
    got = player.model.state_dict()
    assert list(ckpt) == list(got)
    for k in ckpt:
        assert torch.equal(ckpt[k], got[k]), k
