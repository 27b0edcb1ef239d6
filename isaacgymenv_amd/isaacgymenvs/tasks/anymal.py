"""Anymal and Hound: the flat-ground quadruped tasks (reference ``tasks/anymal.py`` and ``tasks/hound.py``).

The two reference files are one program with another robot, so ``Hound`` below is ``Anymal`` with its differences
only.  The behaviour is the reference's, step for step (checked against fixtures recorded from the reference's own
code, tests/golden/anymal_flat.npz and hound_flat.npz):

* the actuation is the simulator's joint drive: every actor's dofs are ``DOF_MODE_POS`` with the config's stiffness
  and damping (anymal.py:199-214), a step sets the targets ``actionScale * a + default_dof_pos`` with
  ``set_dof_position_target_tensor`` (:226-229) and runs one ``simulate``;
* ``self.torques`` is the DOF force tensor (``acquire_dof_force_tensor``, :113, :126): the drive's
  force is a physics output, and the torque penalty of the reward reads it every step;
* ``post_physics_step`` (:231-239): ``progress_buf += 1``, reset what the previous step flagged, the four refreshes,
  observations (48), reward.  A just-reset env's torques and contact forces are still the last simulate's;
* ``reset_idx`` (:278-304): five ``torch_rand_float`` draws in this order -- dof offsets ``(k, 12)`` in U(0.5, 1.5)
  (a factor on the default pose), dof velocities ``(k, 12)`` in U(-0.1, 0.1), then command x, y and yaw, ``(k, 1)``
  each, written through ``.squeeze()``.  It sets ``reset_buf[env_ids] = 1`` (not 0), and ``__init__`` ends with a
  reset of every env;
* reward (:312-351): velocity tracking + the torque penalty, clipped at 0 from below; reset on base contact, any knee
  ("THIGH" / "thigh") contact, or the episode limit.

On the GPU pipeline the post-reset tail (observations, reward, done mask) is one HIP kernel (libgymtask
gt_flat_post_physics) that also publishes the done count to pinned host memory, and ``reset_idx`` of the flagged envs
is one kernel too (gt_flat_reset_flagged, its five draws evaluated from torch's own Philox stream); the torch
statements below stay the CPU-pipeline path and the golden-tested specification.

``task.randomize: True`` raises ``NotImplementedError`` (domain randomisation is outside the scope, as for Ant).

Kernel forms: Anymal's sim carries drive gains, so it runs the one-env-per-lane kernel (the lane team has no drives)
and the host backend for ``sim_device=cpu``; Hound_new has no compiled topology and runs the runtime-sized kernel,
GPU only -- ``sim_device=cpu`` is refused by libgymsim with its own message, as for HoundTerrain.

The packed ANYmal model is ``anymal_minimal.urdf``'s (AnymalTerrain's, the compiled ``anymal_c`` topology); the
reference's ``anymal.urdf`` has other collision shapes, masses and joint limits and no compiled kernel, so
``anymal.urdf`` resolves to the packed minimal model unless the file itself is present under the asset root
(isaacgym/_assets.py PACKED_INDEX).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from isaacgym import gymapi, gymtorch

from ..utils.torch_jit_utils import get_axis_params, quat_rotate, quat_rotate_inverse, to_torch, torch_rand_float
from .base.vec_task import VecTask

FLAT_OBS, FLAT_ACTIONS = 48, 12


class Anymal(VecTask):
    asset_file = "urdf/anymal_c/urdf/anymal.urdf"
    actor_name = "anymal"
    base_link_name = "base"
    knee_name, foot_names = "THIGH", ("SHANK", "FOOT")  # feet: (fixed joints collapsed, kept)

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                 force_render):
        self.cfg = cfg
        env, learn = self.cfg["env"], self.cfg["env"]["learn"]
        self.lin_vel_scale = learn["linearVelocityScale"]
        self.ang_vel_scale = learn["angularVelocityScale"]
        self.dof_pos_scale = learn["dofPositionScale"]
        self.dof_vel_scale = learn["dofVelocityScale"]
        self.action_scale = env["control"]["actionScale"]
        self.rew_scales = {"lin_vel_xy": learn["linearVelocityXYRewardScale"],
                           "ang_vel_z": learn["angularVelocityZRewardScale"],
                           "torque": learn["torqueRewardScale"]}
        self.randomization_params = self.cfg["task"]["randomization_params"]
        self.randomize = self.cfg["task"]["randomize"]
        if self.randomize:
            raise NotImplementedError(f"{type(self).__name__} domain randomisation (task.randomize) is outside the "
                                      f"hot-path scope")
        ranges = env["randomCommandVelocityRanges"]
        self.command_x_range, self.command_y_range = ranges["linear_x"], ranges["linear_y"]
        self.command_yaw_range = ranges["yaw"]
        self.plane_static_friction = env["plane"]["staticFriction"]
        self.plane_dynamic_friction = env["plane"]["dynamicFriction"]
        self.plane_restitution = env["plane"]["restitution"]
        init = env["baseInitState"]
        self.base_init_state = init["pos"] + init["rot"] + init["vLinear"] + init["vAngular"]
        self.named_default_joint_angles = env["defaultJointAngles"]
        env["numObservations"] = FLAT_OBS
        env["numActions"] = FLAT_ACTIONS
        super().__init__(config=self.cfg, rl_device=rl_device, sim_device=sim_device,
                         graphics_device_id=graphics_device_id, headless=headless,
                         virtual_screen_capture=virtual_screen_capture, force_render=force_render)
        dev, n = self.device, self.num_envs
        self.dt = self.sim_params.dt
        self.max_episode_length_s = learn["episodeLength_s"]
        self.max_episode_length = int(self.max_episode_length_s / self.dt + 0.5)
        self.Kp, self.Kd = env["control"]["stiffness"], env["control"]["damping"]
        for key in self.rew_scales:
            self.rew_scales[key] *= self.dt

        root_t = self.gym.acquire_actor_root_state_tensor(self.sim)
        dof_t = self.gym.acquire_dof_state_tensor(self.sim)
        contact_t = self.gym.acquire_net_contact_force_tensor(self.sim)
        force_t = self.gym.acquire_dof_force_tensor(self.sim)
        self._refresh()
        self.root_states = gymtorch.wrap_tensor(root_t)
        self.dof_state = gymtorch.wrap_tensor(dof_t)
        per_dof = self.dof_state.view(n, self.num_dof, 2)
        self.dof_pos, self.dof_vel = per_dof[..., 0], per_dof[..., 1]
        self.contact_forces = gymtorch.wrap_tensor(contact_t).view(n, -1, 3)
        self.torques = gymtorch.wrap_tensor(force_t).view(n, self.num_dof)

        self.commands = torch.zeros(n, 3, dtype=torch.float, device=dev, requires_grad=False)
        self.commands_x, self.commands_y, self.commands_yaw = (self.commands[..., k] for k in range(3))
        self.default_dof_pos = torch.zeros_like(self.dof_pos, dtype=torch.float, device=dev, requires_grad=False)
        for i in range(FLAT_ACTIONS):
            self.default_dof_pos[:, i] = self.named_default_joint_angles[self.dof_names[i]]
        self.extras = {}
        self.initial_root_states = self.root_states.clone()
        self.initial_root_states[:] = to_torch(self.base_init_state, device=dev, requires_grad=False)
        self.gravity_vec = to_torch(get_axis_params(-1.0, self.up_axis_idx), device=dev).repeat((n, 1))
        self.actions = torch.zeros(n, self.num_actions, dtype=torch.float, device=dev, requires_grad=False)
        self.reset_idx(torch.arange(n, device=dev))
        self._tail = None
        if self.device != "cpu":
            # GPU pipeline: observations + reward + done mask are one kernel (gt_flat_post_physics), reset_idx another
            from ...gymtask import FlatTailKernel  # fails loudly when libgymtask.so is missing
            self._tail = FlatTailKernel(self)

    # ------------------------------------------------------------------ scene
    def create_sim(self):
        self.up_axis_idx = 2
        self.sim = super().create_sim(self.device_id, self.graphics_device_id, self.physics_engine, self.sim_params)
        plane = gymapi.PlaneParams()
        plane.normal = gymapi.Vec3(0.0, 0.0, 1.0)
        plane.static_friction = self.plane_static_friction
        plane.dynamic_friction = self.plane_dynamic_friction
        self.gym.add_ground(self.sim, plane)
        self._create_envs(self.num_envs, self.cfg["env"]["envSpacing"], int(np.sqrt(self.num_envs)))

    def _asset_options(self):
        opts = gymapi.AssetOptions()
        opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
        opts.collapse_fixed_joints = True
        opts.replace_cylinder_with_capsule = True
        opts.flip_visual_attachments = True
        opts.fix_base_link = self.cfg["env"]["urdfAsset"]["fixBaseLink"]
        opts.density = 0.001
        opts.angular_damping = 0.0
        opts.linear_damping = 0.0
        opts.armature = 0.0
        opts.thickness = 0.01
        opts.disable_gravity = False
        return opts

    def _create_envs(self, num_envs, spacing, num_per_row):
        here = os.path.dirname(os.path.abspath(__file__))
        asset_root = os.environ.get("ISAACGYMENVS_ASSET_ROOT", os.path.join(here, "../../assets"))
        asset_file = self.cfg["env"]["urdfAsset"].get("file", self.asset_file)
        opts = self._asset_options()
        asset = self.gym.load_asset(self.sim, asset_root, asset_file, opts)
        self.num_dof = self.gym.get_asset_dof_count(asset)
        self.num_bodies = self.gym.get_asset_rigid_body_count(asset)
        start_pose = gymapi.Transform()
        start_pose.p = gymapi.Vec3(*self.base_init_state[:3])

        self.body_names = self.gym.get_asset_rigid_body_names(asset)
        self.dof_names = self.gym.get_asset_dof_names(asset)
        foot = self.foot_names[0] if opts.collapse_fixed_joints else self.foot_names[1]
        feet = [s for s in self.body_names if foot in s]
        knees = [s for s in self.body_names if self.knee_name in s]

        props = self.gym.get_asset_dof_properties(asset)
        for i in range(self.num_dof):
            props["driveMode"][i] = gymapi.DOF_MODE_POS
            props["stiffness"][i] = self.cfg["env"]["control"]["stiffness"]
            props["damping"][i] = self.cfg["env"]["control"]["damping"]

        lower, upper = gymapi.Vec3(-spacing, -spacing, 0.0), gymapi.Vec3(spacing, spacing, spacing)
        self.envs, self.actor_handles = [], []
        for i in range(num_envs):
            env_ptr = self.gym.create_env(self.sim, lower, upper, num_per_row)
            handle = self.gym.create_actor(env_ptr, asset, start_pose, self.actor_name, i, 1, 0)
            self.gym.set_actor_dof_properties(env_ptr, handle, props)
            self.gym.enable_actor_dof_force_sensors(env_ptr, handle)
            self.envs.append(env_ptr)
            self.actor_handles.append(handle)

        find = lambda name: self.gym.find_actor_rigid_body_handle(self.envs[0], self.actor_handles[0], name)  # noqa: E731
        self.feet_indices = torch.tensor([find(s) for s in feet], dtype=torch.long, device=self.device)
        self.knee_indices = torch.tensor([find(s) for s in knees], dtype=torch.long, device=self.device)
        self.base_index = find(self.base_link_name)

    # ------------------------------------------------------------------ step
    def pre_physics_step(self, actions):
        self.actions = actions.clone().to(self.device)
        targets = self.action_scale * self.actions + self.default_dof_pos
        self.gym.set_dof_position_target_tensor(self.sim, gymtorch.unwrap_tensor(targets))

    def post_physics_step(self):
        self.progress_buf += 1
        if self._tail is not None:
            # the previous step's kernel published how many envs it flagged: look for them only then
            k = self._tail.done_count()
            if k is None:  # before the first launch: no ballots yet (every env carries reset_idx's 1)
                env_ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1)
                if len(env_ids) > 0:
                    self.reset_idx(env_ids)
            elif k > 0:  # reset_idx fused (gt_flat_reset_flagged): no nonzero() host sync
                self._tail.reset_flagged(k)
            self._refresh()
            self._tail()  # compute_observations + compute_reward
            return
        env_ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1)
        if len(env_ids) > 0:
            self.reset_idx(env_ids)
        self.compute_observations()
        self.compute_reward(self.actions)

    def _refresh(self):
        self.gym.refresh_dof_state_tensor(self.sim)
        self.gym.refresh_actor_root_state_tensor(self.sim)
        self.gym.refresh_net_contact_force_tensor(self.sim)
        self.gym.refresh_dof_force_tensor(self.sim)

    def compute_observations(self):
        self._refresh()
        self.obs_buf[:] = compute_flat_observations(
            self.root_states, self.commands, self.dof_pos, self.default_dof_pos, self.dof_vel, self.gravity_vec,
            self.actions, self.lin_vel_scale, self.ang_vel_scale, self.dof_pos_scale, self.dof_vel_scale)

    def compute_reward(self, actions):
        self.rew_buf[:], self.reset_buf[:] = compute_flat_reward(
            self.root_states, self.commands, self.torques, self.contact_forces, self.knee_indices, self.progress_buf,
            self.rew_scales, self.base_index, self.max_episode_length)

    def reset_idx(self, env_ids):
        k = len(env_ids)
        factors = torch_rand_float(0.5, 1.5, (k, self.num_dof), device=self.device)
        velocities = torch_rand_float(-0.1, 0.1, (k, self.num_dof), device=self.device)
        self.dof_pos[env_ids] = self.default_dof_pos[env_ids] * factors
        self.dof_vel[env_ids] = velocities
        ids32 = env_ids.to(dtype=torch.int32)
        self.gym.set_actor_root_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.initial_root_states),
                                                     gymtorch.unwrap_tensor(ids32), k)
        self.gym.set_dof_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.dof_state),
                                              gymtorch.unwrap_tensor(ids32), k)
        # (.squeeze() of a (1, 1) draw is 0-d: a reset of exactly one env broadcasts it)
        for column, (lo, hi) in ((self.commands_x, self.command_x_range), (self.commands_y, self.command_y_range),
                                 (self.commands_yaw, self.command_yaw_range)):
            column[env_ids] = torch_rand_float(lo, hi, (k, 1), device=self.device).squeeze()
        self.progress_buf[env_ids] = 0
        self.reset_buf[env_ids] = 1


class Hound(Anymal):
    """hound.py: Hound_new, fixed joints kept per the config, cylinders stay cylinders, ``"trunk"`` for ``"base"``."""
    asset_file = "urdf/Hound_new/Hound.urdf"
    actor_name = "hound"
    base_link_name = "trunk"
    knee_name, foot_names = "thigh", ("calf", "foot")

    def _asset_options(self):
        opts = super()._asset_options()
        opts.collapse_fixed_joints = self.cfg["env"]["urdfAsset"]["collapseFixedJoints"]
        opts.replace_cylinder_with_capsule = False
        opts.flip_visual_attachments = False
        return opts


def compute_flat_observations(root_states, commands, dof_pos, default_dof_pos, dof_vel, gravity_vec, actions,
                              lin_vel_scale: float, ang_vel_scale: float, dof_pos_scale: float, dof_vel_scale: float):
    """anymal.py:355-386: base linear and angular velocity in the base frame (scaled), projected gravity, scaled
    commands, dof positions about the default pose, scaled dof velocities, the actions."""
    quat = root_states[:, 3:7]
    lin = quat_rotate_inverse(quat, root_states[:, 7:10]) * lin_vel_scale
    ang = quat_rotate_inverse(quat, root_states[:, 10:13]) * ang_vel_scale
    gravity = quat_rotate(quat, gravity_vec)  # (quat_rotate, not its inverse: the reference's choice)
    scale = torch.tensor([lin_vel_scale, lin_vel_scale, ang_vel_scale], requires_grad=False, device=commands.device)
    return torch.cat((lin, ang, gravity, commands * scale, (dof_pos - default_dof_pos) * dof_pos_scale,
                      dof_vel * dof_vel_scale, actions), dim=-1)


def compute_flat_reward(root_states, commands, torques, contact_forces, knee_indices, episode_lengths, rew_scales,
                        base_index: int, max_episode_length: int):
    """anymal.py:312-351; returns (reward, reset)."""
    quat = root_states[:, 3:7]
    lin = quat_rotate_inverse(quat, root_states[:, 7:10])
    ang = quat_rotate_inverse(quat, root_states[:, 10:13])
    lin_err = torch.sum(torch.square(commands[:, :2] - lin[:, :2]), dim=1)
    ang_err = torch.square(commands[:, 2] - ang[:, 2])
    rew_lin = torch.exp(-lin_err / 0.25) * rew_scales["lin_vel_xy"]
    rew_ang = torch.exp(-ang_err / 0.25) * rew_scales["ang_vel_z"]
    rew_torque = torch.sum(torch.square(torques), dim=1) * rew_scales["torque"]
    total = torch.clip(rew_lin + rew_ang + rew_torque, 0.0, None)
    reset = torch.norm(contact_forces[:, base_index, :], dim=1) > 1.0
    reset = reset | torch.any(torch.norm(contact_forces[:, knee_indices, :], dim=2) > 1.0, dim=1)
    reset = reset | (episode_lengths >= max_episode_length - 1)
    return total.detach(), reset
