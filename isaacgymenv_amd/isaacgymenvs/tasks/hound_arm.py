"""Houndarm: operational-space reach on a fixed-base, zero-gravity 6-DoF arm (reference ``tasks/hound_arm.py``).

One Open Manipulator P per env (the arm UsefulHound carries on its trunk), welded to the world and loaded with
``disable_gravity = True``; the policy's six actions are a cartesian pose increment that an operational-space
controller (OSC) turns into joint torques, and the reward pulls the end-effector (the ``end_link`` body) to a
commanded point.  The behaviour is the reference's, step for step (checked against a recording of the reference's
own code, tests/golden/houndarm.npz):

* control (hound_arm.py:462-523): ``dpose = a * cmd_limit / actionScale`` with ``cmd_limit = [0.1]*3 + [0.5]*3``;
  ``u = J^T M_eef (kp dpose - kd v_eef) + (1 - J^T M_eef J M^-1) M u_null`` with ``M_eef = (J M^-1 J^T)^-1``,
  ``u_null = -kd_null qd + kp_null wrap(default - q)``, gains 150 / 2 sqrt(150) and 10 / 2 sqrt(10), clamped to the
  URDF's effort limits.  ``J`` is the ``joint6`` row of the fixed-base Jacobian, ``M`` the 6x6 mass matrix.  There is
  no gravity compensation: the task relies on the asset's gravity being off;
* ``post_physics_step`` (:525-533): ``progress_buf += 1``, reset what the previous step flagged, the five refreshes,
  the 10-wide observation (end-effector position 3, quaternion 4, command 3), the reward;
* ``reset_idx`` (:397-459): three command draws (``torch_rand_float`` of ``(k, 1)``, written through ``.squeeze()``),
  then ``torch.rand((k, 6))`` for the joint noise: ``q = clamp(default + houndarmDofNoise * 2 (r - 0.5), limits)``,
  ``qd = 0``; targets, efforts and the dof state are pushed with the three indexed sets; ``reset_buf`` is set to 0;
* reward (:551-567): ``max(0, (1 - tanh(10 d)) distRewardScale + (1 - tanh(10 |v_eef|)) [d < 0.02] velRewardScale)``,
  ``d`` the distance to the command, ``|v_eef|`` over all six velocity components; reset on the episode limit only;
* ``__init__`` ends with a reset of every env and a refresh.

On the GPU pipeline the controller, the post-reset tail and ``reset_idx`` of the flagged envs are one HIP kernel each
(libgymtask gt_arm_control, gt_arm_post_physics, gt_arm_reset_flagged); the torch statements below stay the CPU-tensor
path and the golden-tested specification.

``controlType: joint_tor`` raises ``NotImplementedError``: the reference sizes its observation to 26 for it and then
writes 10, so there is no working behaviour to match.  ``task.randomize: True`` is refused as in Anymal.

The arm has no compiled topology and runs the runtime-sized kernel, GPU only -- ``sim_device=cpu`` is refused by
libgymsim with its own message, as for Hound.  Its model is not shipped with the package: ``env.asset.assetRoot`` and
``env.asset.assetFileNamehoundarm`` name the reference's URDF, or a packed ``*.model.json`` of it
(tools/pack_assets.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from isaacgym import gymapi, gymtorch

from ..utils.torch_jit_utils import tensor_clamp, to_torch, torch_rand_float
from .base.vec_task import VecTask

ARM_OBS, ARM_ACTIONS = 10, 6
ASSET_ROOT = "../../assets"
ASSET_FILE = "urdf/open_manipulator_p_gazebo/urdf/open_manipulator_p.urdf"


class Houndarm(VecTask):
    actor_name = "houndarm"
    eef_link_name, eef_joint_name = "end_link", "joint6"
    # what a subclass on another arm overrides (tasks/manipulator.py)
    arm_dofs = 6
    default_pose = [0, 0, 0, 0, 0, 0]
    dof_noise_key, asset_file_key, asset_file = "houndarmDofNoise", "assetFileNamehoundarm", ASSET_FILE
    flip_visual_attachments = False
    kernels_class = "ArmKernels"

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                 force_render):
        self.cfg = cfg
        env = self.cfg["env"]
        self.max_episode_length = env["episodeLength"]
        self.action_scale = env["actionScale"]
        self.dof_noise = env[self.dof_noise_key]
        ranges = env["randomCommandPositionRanges"]
        self.command_x_range, self.command_y_range, self.command_z_range = ranges["x"], ranges["y"], ranges["z"]
        self.reward_settings = {"r_dist_scale": env["distRewardScale"], "r_vel_scale": env["velRewardScale"]}
        self.control_type = env["controlType"]
        if self.control_type == "joint_tor":
            raise NotImplementedError(f"{type(self).__name__} controlType joint_tor: the reference sizes its "
                                      "observation to 26 and writes 10, so it does not run there either; use osc")
        if self.control_type != "osc":
            raise ValueError("Invalid control type specified. Must be one of: {osc, joint_tor}")
        if self.cfg["task"]["randomize"]:
            raise NotImplementedError(f"{type(self).__name__} domain randomisation (task.randomize) is outside the "
                                      "hot-path scope")
        env["numObservations"] = ARM_OBS
        env["numActions"] = ARM_ACTIONS
        self.up_axis, self.up_axis_idx = "z", 2
        super().__init__(config=self.cfg, rl_device=rl_device, sim_device=sim_device,
                         graphics_device_id=graphics_device_id, headless=headless,
                         virtual_screen_capture=virtual_screen_capture, force_render=force_render)
        dev, n = self.device, self.num_envs
        nd = self.arm_dofs
        self.default_dof_pos = to_torch(self.default_pose, device=dev)
        self.kp = to_torch([150.0] * 6, device=dev)
        self.kd = 2 * torch.sqrt(self.kp)
        self.kp_null = to_torch([10.0] * nd, device=dev)
        self.kd_null = 2 * torch.sqrt(self.kp_null)
        self.cmd_limit = to_torch([0.1, 0.1, 0.1, 0.5, 0.5, 0.5], device=dev).unsqueeze(0)
        self.commands = torch.zeros(n, 3, dtype=torch.float, device=dev, requires_grad=False)
        self.commands_x, self.commands_y, self.commands_z = (self.commands[..., k] for k in range(3))
        self.actions = torch.zeros(n, self.num_actions, dtype=torch.float, device=dev, requires_grad=False)
        self.reset_idx(torch.arange(n, device=dev))
        self._refresh()
        self._kernels = None
        if self.device != "cpu":
            # GPU pipeline: the controller, observations + reward + time-out mask, and reset_idx are one kernel each
            from ... import gymtask  # fails loudly when libgymtask.so is missing
            self._kernels = getattr(gymtask, self.kernels_class)(self)

    # ------------------------------------------------------------------ scene
    def create_sim(self):
        self.sim_params.up_axis = gymapi.UP_AXIS_Z
        self.sim_params.gravity.x, self.sim_params.gravity.y, self.sim_params.gravity.z = 0, 0, -9.81
        self.sim = super().create_sim(self.device_id, self.graphics_device_id, self.physics_engine, self.sim_params)
        plane = gymapi.PlaneParams()
        plane.normal = gymapi.Vec3(0.0, 0.0, 1.0)
        self.gym.add_ground(self.sim, plane)
        self._create_envs(self.num_envs, self.cfg["env"]["envSpacing"], int(np.sqrt(self.num_envs)))

    def _asset_options(self):
        opts = gymapi.AssetOptions()
        opts.replace_cylinder_with_capsule = False
        opts.flip_visual_attachments = self.flip_visual_attachments
        opts.fix_base_link = True
        opts.collapse_fixed_joints = False
        opts.disable_gravity = True  # (the OSC has no gravity compensation)
        opts.thickness = 0.001
        opts.default_dof_drive_mode = gymapi.DOF_MODE_EFFORT
        opts.use_mesh_materials = True
        return opts

    def _asset_path(self):
        """(root, file) from env.asset, as the reference resolves them; a missing file names the two keys."""
        here = os.path.dirname(os.path.abspath(__file__))
        asset = self.cfg["env"].get("asset", {})
        root = os.path.join(here, asset.get("assetRoot", ASSET_ROOT))
        file = asset.get(self.asset_file_key, self.asset_file)
        if not os.path.isfile(os.path.join(root, file)):
            raise FileNotFoundError(
                f"{type(self).__name__} asset not found: {os.path.join(root, file)}.  The arm's model is not shipped "
                f"with the package: point env.asset.assetRoot and env.asset.{self.asset_file_key} at the reference's "
                f"{self.asset_file} or at a packed *.model.json of it (tools/pack_assets.py)")
        return root, file

    def _create_envs(self, num_envs, spacing, num_per_row):
        root, file = self._asset_path()
        asset = self.gym.load_asset(self.sim, root, file, self._asset_options())
        self.num_bodies = self.gym.get_asset_rigid_body_count(asset)
        self.num_dof = self.gym.get_asset_dof_count(asset)

        props = self.gym.get_asset_dof_properties(asset)
        lower, upper, effort = [], [], []
        for i in range(self.num_dof):
            props["driveMode"][i] = gymapi.DOF_MODE_EFFORT
            props["stiffness"][i] = 0.0
            props["damping"][i] = 0.0
            lower.append(props["lower"][i])
            upper.append(props["upper"][i])
            effort.append(props["effort"][i])
        self.dof_lower_limits = to_torch(lower, device=self.device)
        self.dof_upper_limits = to_torch(upper, device=self.device)
        self.effort_limits = to_torch(effort, device=self.device)

        start_pose = gymapi.Transform()
        start_pose.p = gymapi.Vec3(-0.45, 0.0, 0.0)
        start_pose.r = gymapi.Quat(0.0, 0.0, 0.0, 1.0)
        lo, hi = gymapi.Vec3(-spacing, -spacing, 0.0), gymapi.Vec3(spacing, spacing, spacing)
        self.envs, self.actor_handles = [], []
        for i in range(num_envs):
            env_ptr = self.gym.create_env(self.sim, lo, hi, num_per_row)
            # (collision filter 0: the reference's; self-collision of a fixed base is not simulated)
            handle = self.gym.create_actor(env_ptr, asset, start_pose, self.actor_name, i, 0, 0)
            self.gym.set_actor_dof_properties(env_ptr, handle, props)
            self.envs.append(env_ptr)
            self.actor_handles.append(handle)
        self._init_data()

    def _init_data(self):
        n, env0, actor0 = self.num_envs, self.envs[0], self.actor_handles[0]
        self.eef_index = self.gym.find_actor_rigid_body_handle(env0, actor0, self.eef_link_name)
        self.hand_joint_index = self.gym.get_actor_joint_dict(env0, actor0)[self.eef_joint_name]
        self.num_dofs = self.gym.get_sim_dof_count(self.sim) // n
        self.root_states = gymtorch.wrap_tensor(self.gym.acquire_actor_root_state_tensor(self.sim)).view(n, -1, 13)
        self.dof_state = gymtorch.wrap_tensor(self.gym.acquire_dof_state_tensor(self.sim))
        per_dof = self.dof_state.view(n, -1, 2)
        self.dof_pos, self.dof_vel = per_dof[..., 0], per_dof[..., 1]
        self.rigid_body_state = gymtorch.wrap_tensor(self.gym.acquire_rigid_body_state_tensor(self.sim)).view(n, -1, 13)
        self.eef_state = self.rigid_body_state[:, self.eef_index, :]
        # fixed base: [n, links - 1, 6, 6], the welded root's row dropped; the joint6 row is the end link's
        self.jacobian_full = gymtorch.wrap_tensor(self.gym.acquire_jacobian_tensor(self.sim, self.actor_name))
        nd = self.arm_dofs
        self.j_eef = self.jacobian_full[:, self.hand_joint_index, :, :nd]
        self.mass_matrix = gymtorch.wrap_tensor(self.gym.acquire_mass_matrix_tensor(self.sim, self.actor_name))
        self.mm = self.mass_matrix[:, :nd, :nd]
        self.pos_control = torch.zeros((n, self.num_dofs), dtype=torch.float, device=self.device)
        self.effort_control = torch.zeros_like(self.pos_control)
        self.global_indices = torch.arange(n, dtype=torch.int32, device=self.device).view(n, -1)

    # ------------------------------------------------------------------ step
    def compute_osc_torques(self, dpose):
        """hound_arm.py:462-493 (Khatib's operational-space formulation with a null-space posture term)."""
        nd = self.arm_dofs
        q, qd = self.dof_pos[:, :nd], self.dof_vel[:, :nd]
        j_eef_t = torch.transpose(self.j_eef, 1, 2)
        mm_inv = torch.inverse(self.mm)
        m_eef_inv = self.j_eef @ mm_inv @ j_eef_t
        m_eef = torch.inverse(m_eef_inv)
        u = j_eef_t @ m_eef @ (self.kp * dpose - self.kd * self.eef_state[:, 7:]).unsqueeze(-1)
        j_eef_inv = m_eef @ self.j_eef @ mm_inv
        u_null = self.kd_null * -qd + self.kp_null * ((self.default_dof_pos[:nd] - q + np.pi) % (2 * np.pi) - np.pi)
        u_null = self.mm @ u_null.unsqueeze(-1)
        u += (torch.eye(nd, device=self.device).unsqueeze(0) - j_eef_t @ j_eef_inv) @ u_null
        return tensor_clamp(u.squeeze(-1), -self.effort_limits[:nd].unsqueeze(0), self.effort_limits[:nd].unsqueeze(0))

    def pre_physics_step(self, actions):
        self.actions = actions.clone().to(self.device)
        if self._kernels is not None:
            # the torques go into effort_control and straight into the tensor the sim reads its forces from
            self._kernels.control(self.actions, self.sim.dof_force)
            return
        dpose = self.actions * self.cmd_limit / self.action_scale
        self.effort_control[:, :self.arm_dofs] = self.compute_osc_torques(dpose)
        self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(self.effort_control))

    def post_physics_step(self):
        self.progress_buf += 1
        if self._kernels is not None:
            # the previous step's kernel published how many envs it flagged: look for them only then
            k = self._kernels.done_count()
            if k is None:  # before the first launch: no ballots yet
                env_ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1)
                if len(env_ids) > 0:
                    self.reset_idx(env_ids)
            elif k > 0:  # reset_idx fused (gt_arm_reset_flagged): no nonzero() host sync
                self._kernels.reset_flagged(k)
            self._refresh()
            self._kernels()  # compute_observations + compute_reward
            return
        env_ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1)
        if len(env_ids) > 0:
            self.reset_idx(env_ids)
        self.compute_observations()
        self.compute_reward(self.actions)

    def _refresh(self):
        self.gym.refresh_actor_root_state_tensor(self.sim)
        self.gym.refresh_dof_state_tensor(self.sim)
        self.gym.refresh_rigid_body_state_tensor(self.sim)
        self.gym.refresh_jacobian_tensors(self.sim)
        self.gym.refresh_mass_matrix_tensors(self.sim)

    def compute_observations(self):
        self._refresh()
        self.obs_buf[:] = torch.cat((self.eef_state[:, :3], self.eef_state[:, 3:7], self.commands), dim=-1)
        return self.obs_buf

    def compute_reward(self, actions):
        self.rew_buf[:], self.reset_buf[:] = compute_houndarm_reward(
            self.reset_buf, self.progress_buf, self.eef_state, self.commands, self.reward_settings["r_dist_scale"],
            self.reward_settings["r_vel_scale"], self.max_episode_length)

    def _after_reset_clamp(self, pos):
        """What a subclass does to the clamped reset positions before they are written (Houndarm: nothing)."""
        return pos

    def reset_idx(self, env_ids):
        k = len(env_ids)
        # (.squeeze() of a (1, 1) draw is 0-d: a reset of exactly one env broadcasts it)
        for column, (lo, hi) in ((self.commands_x, self.command_x_range), (self.commands_y, self.command_y_range),
                                 (self.commands_z, self.command_z_range)):
            column[env_ids] = torch_rand_float(lo, hi, (k, 1), device=self.device).squeeze()
        noise = torch.rand((k, self.arm_dofs), device=self.device)
        pos = tensor_clamp(self.default_dof_pos.unsqueeze(0) + self.dof_noise * 2.0 * (noise - 0.5),
                           self.dof_lower_limits.unsqueeze(0), self.dof_upper_limits)
        pos = self._after_reset_clamp(pos)
        self.dof_pos[env_ids, :] = pos
        self.dof_vel[env_ids, :] = torch.zeros_like(self.dof_vel[env_ids])
        self.pos_control[env_ids, :] = pos
        self.effort_control[env_ids, :] = torch.zeros_like(pos)
        ids32 = self.global_indices[env_ids].flatten()
        self.gym.set_dof_position_target_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.pos_control),
                                                        gymtorch.unwrap_tensor(ids32), len(ids32))
        self.gym.set_dof_actuation_force_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.effort_control),
                                                        gymtorch.unwrap_tensor(ids32), len(ids32))
        self.gym.set_dof_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.dof_state),
                                              gymtorch.unwrap_tensor(ids32), len(ids32))
        self.progress_buf[env_ids] = 0
        self.reset_buf[env_ids] = 0


def compute_houndarm_reward(reset_buf, progress_buf, eef_state, commands, r_dist_scale: float, r_vel_scale: float,
                            max_episode_length: float):
    """hound_arm.py:551-567; returns (reward, reset)."""
    distance = torch.norm(eef_state[:, :3] - commands, dim=-1)
    distance_rewards = 1 - torch.tanh(10.0 * distance)
    in_reach = distance < 0.02
    velocity_rewards = 1 - torch.tanh(10.0 * torch.norm(eef_state[:, 7:], dim=-1))
    rewards = torch.clip(distance_rewards * r_dist_scale + velocity_rewards * in_reach * r_vel_scale, 0.0, None)
    reset = torch.where(progress_buf >= max_episode_length - 1, torch.ones_like(reset_buf), reset_buf)
    return rewards.detach(), reset
