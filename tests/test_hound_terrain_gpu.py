"""HoundTerrain on the GPU: the fused tail with gt_anymal_variant against the reference's recording, the runtime-sized
kernel on this robot with self-collision, joint limits, per-env friction and the fused PD step against the oracle, and
the task end to end.

The physics cases and their cap are those of tests/hound_terrain_cases.py; tests/test_hound_terrain_physics_cpu.py
holds the float oracle's figures on the same states (one simulate: 1 of 256 envs beyond tolerance, cap 5; PD sequence:
0 of 128, cap 2).
"""
import copy

import numpy as np
import pytest
import torch
import yaml

from tests import helpers as H
from tests import hound_terrain_cases as K
from tests.fakegym_hound import assert_fixture_conditions, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(a, b, what, rtol=1e-5, atol=2e-6):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol,
                               err_msg=what)


def _make(n, monkeypatch, **over):
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    import isaacgymenvs
    torch.manual_seed(42)
    return isaacgymenvs.make(seed=42, task="HoundTerrain", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True,
                             force_render=False, overrides=[f"{k}={v}" for k, v in over.items()])


# ---------------------------------------------------------------- 6. the fused tail against the fixture
def test_fused_tail_matches_reference_golden(monkeypatch):
    """post_a -> host count -> reset_flagged -> post_b with the variant, step by step on the reference's recorded
    post_physics_step inputs (tests/golden/hound_terrain*.npz) and its CPU random stream (tests/
    test_hound_tail_gpu.py's method): shoulder, thigh and trunk resets, time-outs, pushes and the 0.48 m base-height
    term.  Bool and int fields exact, floats within 1e-5 relative (1e-4 for the episode means); the kernels'
    time_outs and clamped observation outputs are VecTask's statements on the kernels' own buffers."""
    d = load_fixture()
    cases = assert_fixture_conditions(d)
    cfg = yaml.safe_load(str(d["cfg_yaml"]))
    cfg["sim"]["use_gpu_pipeline"] = True
    cfg["sim"]["physx"]["use_gpu"] = True
    from isaacgymenv_amd.isaacgymenvs.tasks import anymal_terrain as at
    from isaacgymenv_amd.isaacgymenvs.tasks import hound_terrain as ht
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    monkeypatch.setattr(vec_task, "EXISTING_SIM", None)
    env = ht.HoundTerrain(copy.deepcopy(cfg), DEV, DEV, -1, True, False, False)
    kern = env._kernels
    assert kern is not None and kern._v is not None and not kern.hound, "the GPU pipeline runs the variant tail"
    assert env.sim.kernel_variant == 4
    assert (kern._v.base_height_target, kern._v.knees_terminate, kern._v.num_term_links) == (np.float32(0.48), 1, 4)
    for k in ("feet_indices", "knee_indices", "base_indices"):
        np.testing.assert_array_equal(getattr(env, k).cpu().numpy(), d[k], err_msg=k)
    assert int(env.base_index) == int(d["base_index"])
    kern.inkernel_rng = False  # draws come from the replayed CPU stream below

    def cpu_rand_float(lower, upper, shape, device):
        return ((upper - lower) * torch.rand(*shape) + lower).to(device)

    real_rand_like = torch.rand_like
    monkeypatch.setattr(at, "torch_rand_float", cpu_rand_float)
    monkeypatch.setattr(at, "torch_rand_unit", lambda shape, device: torch.rand(*shape).to(device))
    monkeypatch.setattr(torch, "rand_like", lambda t: real_rand_like(t, device="cpu").to(t.device))
    # the tail's inputs are the fixture's: post_physics_step's refreshes must not overwrite them
    monkeypatch.setattr(env.gym, "refresh_actor_root_state_tensor", lambda sim: None)
    monkeypatch.setattr(env.gym, "refresh_net_contact_force_tensor", lambda sim: None)
    counts = []
    real_wait = kern.wait_reset_count
    kern.wait_reset_count = lambda: counts.append(real_wait()) or counts[-1]

    terms = [str(t) for t in d["terms"]]
    T, N = d["actions"].shape[0], env.num_envs
    assert N == d["obs"].shape[1] == 32 and env.num_obs == 188
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    for t in range(T):
        env.root_states.copy_(g(d["in_root"][t]))
        env.contact_forces.copy_(g(d["in_contact"][t]))
        env.dof_state.copy_(g(d["in_dof"][t]))
        env.torques.copy_(g(d["in_torques"][t]))
        env.actions = g(d["in_actions"][t]).clone()
        env.last_actions.copy_(g(d["in_last_actions"][t]))
        env.last_dof_vel.copy_(g(d["in_last_dof_vel"][t]))
        env.commands.copy_(g(d["in_commands"][t]))
        env.feet_air_time.copy_(g(d["in_feet_air_time"][t]))
        env.progress_buf.copy_(g(d["in_progress"][t]))
        for k, name in enumerate(terms):
            env.episode_sums[name].copy_(g(d["in_episode_sums"][t][k]))
        to = g(d["in_timeout"][t])
        env.timeout_buf = to if d["in_timeout_is_long"][t] else to.bool()
        env.common_step_counter = env.push_interval - 1 if d["in_push"][t] else 0
        env.extras.pop("episode", None)
        torch.set_rng_state(torch.from_numpy(d["in_rng_state"][t]))
        env.post_physics_step()
        torch.cuda.synchronize()
        assert env.reset_buf.dtype == torch.bool
        np.testing.assert_array_equal(env.reset_buf.cpu().numpy().astype(np.int64), d["reset"][t],
                                      err_msg=f"reset step {t}")
        np.testing.assert_array_equal(env.progress_buf.cpu().numpy(), d["progress"][t], err_msg=f"progress step {t}")
        assert counts[-1] == int(d["reset"][t].sum()), f"reset count step {t}"
        _close(env.rew_buf.cpu().numpy(), d["rew"][t], f"reward step {t}")
        _close(env.commands.cpu().numpy(), d["commands"][t], f"commands step {t}")
        _close(env.feet_air_time.cpu().numpy(), d["feet_air_time"][t], f"feet air time step {t}")
        _close(np.stack([env.episode_sums[k].cpu().numpy() for k in terms]), d["episode_sums"][t],
               f"episode sums step {t}")
        _close(env.obs_buf.cpu().numpy(), d["obs"][t], f"obs step {t}")
        _close(env.root_states.cpu().numpy(), d["out_root"][t], f"root states step {t}")
        _close(env.dof_state.cpu().numpy(), d["out_dof"][t], f"dof state step {t}")
        _close(env.last_actions.cpu().numpy(), d["out_last_actions"][t], f"last actions step {t}")
        _close(env.last_dof_vel.cpu().numpy(), d["out_last_dof_vel"][t], f"last dof vel step {t}")
        _close(env.base_lin_vel.cpu().numpy(), d["out_base_lin_vel"][t], f"base lin vel step {t}")
        _close(env.base_ang_vel.cpu().numpy(), d["out_base_ang_vel"][t], f"base ang vel step {t}")
        _close(env.projected_gravity.cpu().numpy(), d["out_projected_gravity"][t], f"projected gravity step {t}")
        time_outs, obs_out = env._fused_outputs
        env._fused_outputs = None
        assert torch.equal(obs_out, torch.clamp(env.obs_buf, -env.clip_obs, env.clip_obs))
        assert torch.equal(time_outs, (env.progress_buf >= env.max_episode_length - 1) & (env.reset_buf != 0))
        np.testing.assert_array_equal(time_outs.cpu().numpy().astype(np.int64), d["time_outs"][t])
        if d["ep_mask"][t]:
            got = np.array([float(env.extras["episode"]["rew_" + k]) for k in terms] +
                           [float(env.extras["episode"]["terrain_level"])])
            _close(got, d["ep_extras"][t], f"extras step {t}", rtol=1e-4, atol=1e-7)
        else:
            assert "episode" not in env.extras
    assert sum(counts) == int(d["reset"].sum()) and cases["shoulder_only"] > 0 and cases["push"] > 0


# ---------------------------------------------------------------- 7. single-launch and reset-observe paths
def test_post_ab_and_reset_observe_are_bit_identical_to_the_three_launches(monkeypatch):
    """With the variant, gt_anymal_post_physics_ab (post_a and the optimistic observations in one launch) and
    gt_anymal_wait_reset_observe (the reset step's sequence in one C call) against post_a -> count -> reset_flagged
    -> post_b from the same state, over 12 steps of 5-step episodes with a push step: every output bit-identical
    (tests/test_task_gpu.py::test_post_ab_launch_is_bit_identical_to_post_a_then_post_b's rule)."""
    from tests.test_task_gpu import _restore, _snapshot
    n = 256
    monkeypatch.setenv("GT_POST_AB", "1")  # (opt-in, gymtask.post_ab_applies)
    env = _make(n, monkeypatch, **{"task.env.learn.episodeLength_s": 0.1, "task.env.learn.baseHeightRewardScale": -5.0})
    kernels = env._kernels
    assert kernels._v is not None and env.sim.kernel_variant == 4
    gen = torch.Generator(device=DEV).manual_seed(21)
    acts = [2 * torch.rand((n, 12), device=DEV, generator=gen) - 1 for _ in range(12)]
    env.step(acts[0])
    env.common_step_counter = env.push_interval - 6
    snap = _snapshot(env)
    out, used = {}, {}
    real_ab, real_ro, real_rf = kernels.post_ab, kernels.wait_reset_observe, kernels.reset_flagged
    for mode in ("single", "separate"):
        _restore(env, snap)
        kernels._ab_ok = None if mode == "single" else False
        kernels._ro_ok = None if mode == "single" else False
        assert kernels.post_ab_applies() == kernels.reset_observe_applies() == (mode == "single")
        calls = used[mode] = {"ab": 0, "ro": 0, "rf": 0}
        kernels.post_ab = lambda c=calls: (c.__setitem__("ab", c["ab"] + 1), real_ab())[1]
        kernels.wait_reset_observe = lambda s, c=calls: (c.__setitem__("ro", c["ro"] + 1), real_ro(s))[1]
        kernels.reset_flagged = lambda *a, c=calls, **k: (c.__setitem__("rf", c["rf"] + 1), real_rf(*a, **k))[1]
        env.extras.pop("episode", None)
        res = []
        for a in acts:
            obs, rew, reset, extras = env.step(a)
            ep = extras.get("episode")
            res.append([obs["obs"].clone(), rew.clone(), reset.clone(), extras["time_outs"].clone(),
                        None if ep is None else torch.stack([torch.as_tensor(v, device=DEV).float()
                                                             for v in ep.values()]),
                        env.root_states.clone(), env.dof_state.clone(), env.progress_buf.clone(), env.commands.clone(),
                        env.feet_air_time.clone(), torch.stack([v.clone() for v in env.episode_sums.values()]),
                        env.last_actions.clone(), env.last_dof_vel.clone(), kernels.reset_masks.clone(),
                        kernels.reset_count.clone()])
            env.extras.pop("episode", None)
        out[mode] = res
    kernels.post_ab, kernels.wait_reset_observe, kernels.reset_flagged = real_ab, real_ro, real_rf
    kernels._ab_ok = kernels._ro_ok = None
    assert used["single"]["ab"] == len(acts) and used["single"]["ro"] == len(acts) and used["single"]["rf"] == 0
    assert used["separate"]["ab"] == 0 and used["separate"]["ro"] == 0 and used["separate"]["rf"] >= 2
    n_reset_steps = 0
    for t, (a, b) in enumerate(zip(out["single"], out["separate"])):
        n_reset_steps += int(bool(a[2].any()))
        for k, (x, y) in enumerate(zip(a, b)):
            assert (x is None) == (y is None), (t, k)
            if x is not None:
                assert torch.equal(x, y), f"step {t} output {k}"
    assert n_reset_steps >= 2


# ---------------------------------------------------------------- 8. physics, one simulate
def test_one_simulate_with_self_collision_limits_and_friction_matches_oracle():
    """hound_new with collision filter 0 on the runtime-sized kernel, TGS, one simulate from 256 states (standing,
    crossed legs with an active self-contact, tucked legs, dofs at their limits; per-env friction in [0.5, 1.25])
    against the fp64 oracle: state and per-link contact forces, every env within tolerance or explained, at most 2 %
    beyond tolerance (the float oracle alone: 1 of 256).  The kernel's own self-contact pools hold a contact in at
    least 80 envs (the oracle's: 90; hound_terrain_cases.MIN_SELF_CONTACT_ENVS)."""
    n = K.N_SIMULATE
    art, flat = K.model()
    root, dof, tau, mu = K.states(n, K.SEED_SIMULATE)
    gym, sim = H.make_gpu_sim("hound_new", n, K.PARAMS, self_collide=True)
    assert sim.kernel_variant == 4 and sim.self_collide
    H.load_state_into(sim, root, dof, mu)
    pools, cnt = H.sim_self_contacts(sim, 0)
    assert int((cnt > 0).sum()) >= K.MIN_SELF_CONTACT_ENVS, int((cnt > 0).sum())
    sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
    gym.simulate(sim)
    gym.refresh_net_contact_force_tensor(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 12)
    g_cf = sim.contact_tensor.cpu().numpy().astype(np.float64).reshape(n, K.NUM_LINKS, 3)
    ref = K.oracle_simulate(root, dof, tau, mu, 64)
    assert np.abs(ref["cf"]).sum() > 0
    H.assert_close_or_explained(H.state_fields(g_root, g_dof, g_cf), ref, K.simulate_rerun(root, dof, tau, mu),
                                max_env_frac=K.MAX_ENV_FRAC,
                                what="hound_terrain one simulate, runtime-sized kernel vs oracle (256 envs, TGS)")


# ---------------------------------------------------------------- 9. physics, the fused PD step
def test_fused_pd_step_matches_the_oracle_sequence():
    """One amd_pd_decimation_step (launch_pd_generic: decimation 4 and one extra simulate, kp 80, kd 2, scale 0.5,
    clip 80) on 128 envs in the task's regime, four of them with crossed legs in contact, against the oracle's PD
    sequence: dofs, root, torques and contact forces under the 4 x PD + 1 tolerances, at most 2 % of the envs beyond
    tolerance (the float oracle alone: 0 of 128)."""
    n = K.N_PD
    root, dof, mu, act = K.pd_states(n, K.SEED_PD)
    gym, sim = H.make_gpu_sim("hound_new", n, K.PARAMS, self_collide=True)
    assert sim.kernel_variant == 4 and sim.self_collide
    H.load_state_into(sim, root, dof, mu)
    gym.refresh_dof_state_tensor(sim)
    torch.cuda.synchronize()
    dof_tensor = sim.dof_tensor.view(n, 12, 2).double().cpu().numpy()
    torques = torch.empty((n, 12), device=DEV)
    gym.amd_pd_decimation_step(sim, torch.from_numpy(act.astype(np.float32)).to(DEV),
                               torch.from_numpy(K.DEFAULT_POS.astype(np.float32)).to(DEV), K.KP, K.KD, K.ACTION_SCALE,
                               K.TORQUE_CLIP, K.DECIMATION, K.EXTRA, torques)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 12)
    gpu = dict(q=g_dof[:, :, 0], qd=g_dof[:, :, 1], pose=g_root[:, :7], vel=g_root[:, 7:],
               tau=torques.double().cpu().numpy(),
               cf=sim.contact_tensor.double().cpu().numpy().reshape(n, K.NUM_LINKS, 3))
    ref = K.pd_sequence(root, dof, dof_tensor, mu, act, 64)
    assert np.abs(ref["cf"]).sum() > 0
    H.assert_close_or_explained(gpu, ref, K.pd_rerun(root, dof, dof_tensor, mu, act), tol=K.SEQ_TOL,
                                max_env_frac=K.MAX_ENV_FRAC,
                                what="hound_terrain fused pd step, 4 x PD + 1, runtime-sized kernel vs oracle")


# ---------------------------------------------------------------- 10. end to end
def test_make_steps_and_resets_as_the_task_says(monkeypatch):
    """make(task="HoundTerrain") on the GPU, 25 random-action steps of 64 envs: the runtime-sized kernel, finite
    188-wide observations, and every env reset in a step starts at root z 0.62 with each dof at its default times a
    factor in [0.5, 1.5] (reset_idx, Hound_terrain.py:401-416)."""
    n = 64
    env = _make(n, monkeypatch, **{"task.env.learn.episodeLength_s": 0.3})
    assert env.sim.kernel_variant == 4 and env._kernels._v is not None
    assert env.max_episode_length == 15
    default = env.default_dof_pos[0]
    gen = torch.Generator(device=DEV).manual_seed(3)
    resets = 0
    for t in range(25):
        obs, rew, reset, extras = env.step(2 * torch.rand((n, 12), device=DEV, generator=gen) - 1)
        o = obs["obs"]
        assert tuple(o.shape) == (n, 188) and torch.isfinite(o).all() and torch.isfinite(rew).all()
        assert reset.dtype == torch.bool
        if bool(reset.any()):
            resets += int(reset.sum())
            assert torch.equal(env.root_states[reset, 2], torch.full_like(env.root_states[reset, 2], 0.62))
            q = env.dof_state.view(n, 12, 2)[reset][:, :, 0]
            lo, hi = torch.minimum(0.5 * default, 1.5 * default), torch.maximum(0.5 * default, 1.5 * default)
            assert bool(((q >= lo - 1e-6) & (q <= hi + 1e-6)).all())
            assert bool((env.progress_buf[reset] == 0).all())
    assert resets >= n  # the 15-step episodes end inside the run, whatever falls before


def test_fused_step_equals_unfused_sequence(monkeypatch):
    """Three env steps of the fused path (one gs_sim_pd_step launch each) against the unfused sequence
    (GS_DISABLE_FUSED: torch PD -> set efforts -> simulate -> refresh, x 4, + 1 simulate) from the same state, under
    tests/test_task_gpu.py::test_fused_step_equals_unfused_sequence's rule and tolerances: equal done masks, every env
    within tolerance or moved as far by the unfused sequence itself under fp32-rounding noise."""
    from tests.test_task_gpu import _restore, _snapshot
    n, nd = 256, 12
    env = _make(n, monkeypatch)
    gen = torch.Generator(device=DEV).manual_seed(5)
    acts = [2 * torch.rand((n, nd), device=DEV, generator=gen) - 1 for _ in range(3)]
    for a in acts:  # leave the initial state
        env.step(a)
    snap = _snapshot(env)

    def run(mode, idx=None, rng=None):
        _restore(env, snap)
        if idx is not None:  # fp32-rounding-sized noise on the sim state of envs idx (H.perturbed's sizes)
            st = env.sim.state
            ii = torch.as_tensor(idx, device=st.device)
            for rows, sd in ((range(0, 3), 1e-6), (range(7, 13), 1e-5), (range(13, 13 + nd), 1e-6),
                             (range(13 + nd, 13 + 2 * nd), 1e-5)):
                for row in rows:
                    st[row, ii] += torch.from_numpy(rng.normal(0, sd, len(idx)).astype(np.float32)).to(st.device)
        monkeypatch.setenv("GS_DISABLE_FUSED", mode)
        res = {k: [] for k in ("q", "qd", "pose", "vel", "obs", "rew")}
        resets = []
        for a in acts:
            obs, rew, reset, _ = env.step(a)
            q = env.dof_state.view(n, nd, 2)
            res["q"].append(q[..., 0].cpu().numpy())
            res["qd"].append(q[..., 1].cpu().numpy())
            res["pose"].append(env.root_states[:, :7].cpu().numpy())
            res["vel"].append(env.root_states[:, 7:].cpu().numpy())
            res["obs"].append(obs["obs"].cpu().numpy())
            res["rew"].append(rew.cpu().numpy()[:, None])
            resets.append(reset.clone())
        return {k: np.stack(v, axis=1) for k, v in res.items()}, resets

    unfused, r_unfused = run("1")
    fused, r_fused = run("0")
    for d1, d2 in zip(r_unfused, r_fused):
        assert torch.equal(d1, d2)

    def rerun(idx, rng):
        out, _ = run("1", idx, rng)
        return {k: v[idx] for k, v in out.items()}
    tol = {"q": (2e-4, 0.0), "qd": (1e-2, 1e-2), "pose": (2e-4, 0.0), "vel": (1e-2, 1e-2), "obs": (1e-2, 1e-2),
           "rew": (1e-4, 1e-2)}
    H.assert_close_or_explained(fused, unfused, rerun, tol=tol, max_env_frac=1e-2,
                                what="fused vs unfused HoundTerrain step (3 env steps)")


def test_trimesh_is_refused_with_the_runtime_kernel_message(monkeypatch):
    """terrainType: trimesh through make(): libgymsim's own message (the runtime-sized kernel has plane contacts
    only) reaches the caller."""
    with pytest.raises(RuntimeError, match="terrain mesh: the runtime-sized kernel has plane contacts only"):
        _make(16, monkeypatch, **{"task.env.terrain.terrainType": "trimesh", "task.env.terrain.numLevels": 2,
                                  "task.env.terrain.numTerrains": 2})


# ---------------------------------------------------------------- 11. learner
def test_ppo_epochs_run_with_finite_losses():
    """Two PPO epochs of the in-repo learner on 256 envs with HoundTerrainPPO.yaml (the minibatch cut to the
    256 x 24 batch): finite losses and parameters."""
    from isaacgymenv_amd.isaacgymenvs.config import compose
    from isaacgymenv_amd.isaacgymenvs.tasks.base import vec_task
    from isaacgymenv_amd.rl import A2CAgent, PpoConfig
    import isaacgymenvs
    vec_task.EXISTING_SIM = None
    cfg = compose("config", ["task=HoundTerrain"])
    assert cfg["train"]["params"]["config"]["name"] == "UsefulHound"
    env = isaacgymenvs.make(seed=42, task="HoundTerrain", num_envs=256, sim_device=DEV, rl_device=DEV, headless=True,
                            force_render=False)
    agent = A2CAgent(env, PpoConfig.from_train_cfg(cfg["train"], minibatch_size=3072), device=DEV, seed=42)
    for _ in range(2):
        agent.train_epoch()
    s = agent.epoch_stats()
    assert np.isfinite(s["kl"]) and np.isfinite(s["a_loss"]) and np.isfinite(s["c_loss"])
    assert all(torch.isfinite(p).all() for p in agent.params)
    assert agent.frame == 2 * 24 * 256 and env.sim.kernel_variant == 4
