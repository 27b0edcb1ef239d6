"""Humanoid locomotion (reference ``tasks/humanoid.py``), the third of the upstream locomotion trio.

The behaviour is the reference's, step for step (checked against a recording of the reference's own code,
tests/golden/humanoid.npz):

* actions are torques: ``a * motor_efforts * powerScale`` with the efforts the MJCF motors declare, gear x control
  limit, listed in the file's ``<actuator>`` order and multiplied onto actions in DOF order as they are
  (humanoid.py:160-163, 281-285); written with ``set_dof_actuation_force_tensor``;
* one ``simulate`` per control step (dt 1/60, 2 substeps), the actor created with collision filter 0 (its own
  shapes collide), joint limits enforced by the solver, force sensors on both feet, the DOF force tensor enabled
  (humanoid.py:164-168, 194-196);
* start height 1.34; the start pose of a joint is 0 unless 0 lies outside its range (humanoid.py:99-102);
* ``post_physics_step`` resets the envs flagged in the previous step, then rebuilds the 108-wide observation and the
  reward (humanoid.py:287-296);
* reset draws: dof offsets U(-0.2, 0.2) then dof velocities U(-0.1, 0.1), both [k, 21], in that order, positions
  clamped into the limits (humanoid.py:253-279); the reset buffer is int64.

On the GPU pipeline the post-reset tail (observations, reward, done mask) is one HIP kernel (libgymtask
gt_humanoid_post_physics) that also publishes the done count to pinned host memory, and reset_idx of the flagged envs
is another (gt_humanoid_reset_flagged); the torch statements below stay the CPU-tensor path and the golden-tested
specification.

Observation layout (humanoid.py:407-411): torso height, local linear velocity (3), local angular velocity *
angularVelocityScale (3), yaw, roll, angle to target, up projection, heading projection, scaled dof positions (21),
dof velocities * dofVelocityScale (21), DOF forces * contactForceScale (21), the two foot sensors' wrenches *
contactForceScale (12), actions (21).

Two deviations from the reference, on purpose.  One: every actor's dofs are switched to ``DOF_MODE_POS`` with
the position targets left at 0, so the stiffness and damping the MJCF declares per joint act as MuJoCo means them --
a passive spring toward 0 and a passive damper, integrated implicitly by the simulator's joint drive.
The body is built around them (a hip's damping of 5 against an inertia of 0.02 about its axis): under
``DOF_MODE_NONE`` saturated torques spin such joints past what the solver's explicit step integrates at the task's 2
substeps and the state diverges within a few steps ("Stability").  The DOF force tensor, and
with it observation columns 54-74, then holds the motor's effort plus that spring-damper force.

A second one: an env whose observation or reward is not finite (a diverged simulation; about one env in 10^5
env-steps under an untrained policy) ends as a fallen one does -- a zero observation, the death
cost, the done flag -- in the kernel and in ``end_nonfinite_envs`` below.  The reference's height test is false for
NaN and would leave such an env non-finite until its time-out.

The body is not shipped with the package: ``env.asset.assetFileName`` (under ``env.asset.assetRoot``, the reference's
``../../assets`` by default, or ``ISAACGYMENVS_ASSET_ROOT``) names the reference's ``mjcf/nv_humanoid.xml`` or a
packed ``*.model.json`` of it (tools/pack_assets.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from isaacgym import gymapi, gymtorch

from ..utils.torch_jit_utils import (compute_heading_and_up, compute_rot, get_axis_params, normalize_angle,
                                     quat_conjugate, tensor_clamp, to_torch, torch_rand_float, unscale)
from .base.vec_task import VecTask

HUMANOID_OBS, HUMANOID_ACTIONS, HUMANOID_SENSORS = 108, 21, 2
ASSET_ROOT, ASSET_FILE = "../../assets", "mjcf/nv_humanoid.xml"

# column ranges inside the observation (humanoid.py:407-411)
OBS_HEIGHT, OBS_UP, OBS_HEADING = 0, 10, 11
OBS_DOF_POS = slice(12, 33)
OBS_DOF_VEL = slice(33, 54)
OBS_DOF_FORCE = slice(54, 75)
OBS_SENSORS = slice(75, 87)
OBS_ACTIONS = slice(87, 108)


class Humanoid(VecTask):
    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                 force_render):
        self.cfg = cfg
        env = self.cfg["env"]
        self.randomization_params = self.cfg["task"]["randomization_params"]
        self.randomize = self.cfg["task"]["randomize"]
        if self.randomize:
            raise NotImplementedError("Humanoid domain randomisation (task.randomize) is outside the hot-path scope")
        self.dof_vel_scale = env["dofVelocityScale"]
        self.angular_velocity_scale = env.get("angularVelocityScale", 0.1)
        self.contact_force_scale = env["contactForceScale"]
        self.power_scale = env["powerScale"]
        self.heading_weight = env["headingWeight"]
        self.up_weight = env["upWeight"]
        self.actions_cost_scale = env["actionsCost"]
        self.energy_cost_scale = env["energyCost"]
        self.joints_at_limit_cost_scale = env["jointsAtLimitCost"]
        self.death_cost = env["deathCost"]
        self.termination_height = env["terminationHeight"]
        self.debug_viz = env["enableDebugVis"]
        self.plane_static_friction = env["plane"]["staticFriction"]
        self.plane_dynamic_friction = env["plane"]["dynamicFriction"]
        self.plane_restitution = env["plane"]["restitution"]
        self.max_episode_length = env["episodeLength"]
        env["numObservations"] = HUMANOID_OBS
        env["numActions"] = HUMANOID_ACTIONS
        super().__init__(config=self.cfg, rl_device=rl_device, sim_device=sim_device,
                         graphics_device_id=graphics_device_id, headless=headless,
                         virtual_screen_capture=virtual_screen_capture, force_render=force_render)
        dev, n = self.device, self.num_envs

        root_t = self.gym.acquire_actor_root_state_tensor(self.sim)
        dof_t = self.gym.acquire_dof_state_tensor(self.sim)
        sensor_t = self.gym.acquire_force_sensor_tensor(self.sim)
        self.vec_sensor_tensor = gymtorch.wrap_tensor(sensor_t).view(n, HUMANOID_SENSORS * 6)
        force_t = self.gym.acquire_dof_force_tensor(self.sim)
        self.dof_force_tensor = gymtorch.wrap_tensor(force_t).view(n, self.num_dof)
        self.gym.refresh_dof_state_tensor(self.sim)
        self.gym.refresh_actor_root_state_tensor(self.sim)

        self.root_states = gymtorch.wrap_tensor(root_t)
        self.initial_root_states = self.root_states.clone()
        self.initial_root_states[:, 7:13] = 0.0
        self.dof_state = gymtorch.wrap_tensor(dof_t)
        per_dof = self.dof_state.view(n, self.num_dof, 2)
        self.dof_pos, self.dof_vel = per_dof[..., 0], per_dof[..., 1]
        # the start pose is 0 unless 0 lies outside a joint's range (humanoid.py:99-102)
        lo, hi = self.dof_limits_lower, self.dof_limits_upper
        start = torch.where(lo > 0.0, lo, torch.where(hi < 0.0, hi, torch.zeros_like(lo)))
        self.initial_dof_pos = start.expand(n, -1).clone()
        self.initial_dof_vel = torch.zeros_like(self.dof_vel)

        self.up_vec = to_torch(get_axis_params(1.0, self.up_axis_idx), device=dev).repeat((n, 1))
        self.heading_vec = to_torch([1, 0, 0], device=dev).repeat((n, 1))
        self.inv_start_rot = quat_conjugate(self.start_rotation).repeat((n, 1))
        self.basis_vec0 = self.heading_vec.clone()
        self.basis_vec1 = self.up_vec.clone()
        self.targets = to_torch([1000, 0, 0], device=dev).repeat((n, 1))
        self.target_dirs = to_torch([1, 0, 0], device=dev).repeat((n, 1))
        self.dt = self.cfg["sim"]["dt"]
        self.potentials = to_torch([-1000.0 / self.dt], device=dev).repeat(n)
        self.prev_potentials = self.potentials.clone()
        self._tail = None
        if self.device != "cpu":
            # GPU pipeline: observations + reward + done mask are one kernel (gt_humanoid_post_physics)
            from ...gymtask import HumanoidTailKernel  # fails loudly when libgymtask.so is missing
            self._tail = HumanoidTailKernel(self)

    # ------------------------------------------------------------------ scene
    def create_sim(self):
        self.up_axis_idx = 2
        self.sim = super().create_sim(self.device_id, self.graphics_device_id, self.physics_engine, self.sim_params)
        plane = gymapi.PlaneParams()
        plane.normal = gymapi.Vec3(0.0, 0.0, 1.0)
        plane.static_friction = self.plane_static_friction
        plane.dynamic_friction = self.plane_dynamic_friction
        plane.restitution = self.plane_restitution
        self.gym.add_ground(self.sim, plane)
        spacing = self.cfg["env"]["envSpacing"]
        self._create_envs(self.num_envs, spacing, int(np.sqrt(self.num_envs)))

    def _asset_path(self):
        """(root, file) as the reference resolves them (humanoid.py:142-150); a missing file names the two keys."""
        here = os.path.dirname(os.path.abspath(__file__))
        asset = self.cfg["env"].get("asset", {})
        root = os.path.join(here, asset.get("assetRoot", os.environ.get("ISAACGYMENVS_ASSET_ROOT", ASSET_ROOT)))
        path = os.path.join(root, asset.get("assetFileName", ASSET_FILE))
        if not os.path.isfile(path):
            raise FileNotFoundError(
                f"Humanoid asset not found: {path}.  The body's model is not shipped with the package: point "
                f"env.asset.assetRoot and env.asset.assetFileName at the reference's {ASSET_FILE} or at a packed "
                f"*.model.json of it (tools/pack_assets.py)")
        return os.path.dirname(path), os.path.basename(path)

    def _create_envs(self, num_envs, spacing, num_per_row):
        root, file = self._asset_path()
        opts = gymapi.AssetOptions()
        opts.angular_damping = 0.01
        opts.max_angular_velocity = 100.0
        opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE  # (humanoid.py:156; the actors switch to POS below)
        asset = self.gym.load_asset(self.sim, root, file, opts)
        # the motors in the MJCF's <actuator> order, multiplied onto actions in DOF order as they are
        motor_efforts = [p.motor_effort for p in self.gym.get_asset_actuator_properties(asset)]
        right_foot = self.gym.find_asset_rigid_body_index(asset, "right_foot")
        left_foot = self.gym.find_asset_rigid_body_index(asset, "left_foot")
        self.gym.create_asset_force_sensor(asset, right_foot, gymapi.Transform())
        self.gym.create_asset_force_sensor(asset, left_foot, gymapi.Transform())
        self.max_motor_effort = max(motor_efforts)
        self.motor_efforts = to_torch(motor_efforts, device=self.device)
        self.torso_index = 0
        self.num_bodies = self.gym.get_asset_rigid_body_count(asset)
        self.num_dof = self.gym.get_asset_dof_count(asset)
        self.num_joints = self.gym.get_asset_joint_count(asset)

        start_pose = gymapi.Transform()
        start_pose.p = gymapi.Vec3(*get_axis_params(1.34, self.up_axis_idx))
        start_pose.r = gymapi.Quat(0.0, 0.0, 0.0, 1.0)
        r = start_pose.r
        self.start_rotation = torch.tensor([r.x, r.y, r.z, r.w], device=self.device)

        lower, upper = gymapi.Vec3(-spacing, -spacing, 0.0), gymapi.Vec3(spacing, spacing, spacing)
        self.envs, self.humanoid_handles = [], []
        for i in range(num_envs):
            env_ptr = self.gym.create_env(self.sim, lower, upper, num_per_row)
            handle = self.gym.create_actor(env_ptr, asset, start_pose, "humanoid", i, 0, 0)  # filter 0: self-collision
            self.gym.enable_actor_dof_force_sensors(env_ptr, handle)
            # the body's passive joint springs and dampers (module docstring): the MJCF's stiffness / damping are in
            # the dof properties already, the drive toward the targets' initial 0 applies them
            props = self.gym.get_actor_dof_properties(env_ptr, handle)
            props["driveMode"][:] = gymapi.DOF_MODE_POS
            self.gym.set_actor_dof_properties(env_ptr, handle, props)
            self.envs.append(env_ptr)
            self.humanoid_handles.append(handle)

        # limits of the last actor, each pair ordered (humanoid.py:205-215)
        props = self.gym.get_actor_dof_properties(self.envs[-1], self.humanoid_handles[-1])
        a, b = np.asarray(props["lower"], np.float64), np.asarray(props["upper"], np.float64)
        self.dof_limits_lower = to_torch(np.minimum(a, b).tolist(), device=self.device)
        self.dof_limits_upper = to_torch(np.maximum(a, b).tolist(), device=self.device)
        self.extremities = to_torch([5, 8], device=self.device, dtype=torch.long)

    # ------------------------------------------------------------------ step
    def pre_physics_step(self, actions):
        self.actions = actions.to(self.device).clone()
        forces = self.actions * self.motor_efforts.unsqueeze(0) * self.power_scale
        self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(forces))

    def post_physics_step(self):
        self.progress_buf += 1
        self.randomize_buf += 1
        if self._tail is not None:
            # the previous step's kernel published how many envs it flagged: look for them only then
            k = self._tail.done_count()
            if k is None:  # before the first launch: no ballots yet
                env_ids = self.reset_buf.nonzero(as_tuple=False).flatten()
                if len(env_ids) > 0:
                    self.reset_idx(env_ids)
            elif k > 0:  # reset_idx fused (gt_humanoid_reset_flagged): no nonzero() host sync
                self._tail.reset_flagged(k)
            self.gym.refresh_dof_state_tensor(self.sim)
            self.gym.refresh_actor_root_state_tensor(self.sim)
            self.gym.refresh_force_sensor_tensor(self.sim)
            self.gym.refresh_dof_force_tensor(self.sim)
            self._tail()  # compute_observations + compute_reward
            return
        env_ids = self.reset_buf.nonzero(as_tuple=False).flatten()
        if len(env_ids) > 0:
            self.reset_idx(env_ids)
        self.compute_observations()
        self.compute_reward(self.actions)

    def reset_idx(self, env_ids):
        k = len(env_ids)
        positions = torch_rand_float(-0.2, 0.2, (k, self.num_dof), device=self.device)
        velocities = torch_rand_float(-0.1, 0.1, (k, self.num_dof), device=self.device)
        self.dof_pos[env_ids] = tensor_clamp(self.initial_dof_pos[env_ids] + positions, self.dof_limits_lower,
                                             self.dof_limits_upper)
        self.dof_vel[env_ids] = velocities
        ids32 = env_ids.to(dtype=torch.int32)
        self.gym.set_actor_root_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.initial_root_states),
                                                     gymtorch.unwrap_tensor(ids32), k)
        self.gym.set_dof_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.dof_state),
                                              gymtorch.unwrap_tensor(ids32), k)
        to_target = self.targets[env_ids] - self.initial_root_states[env_ids, 0:3]
        to_target[:, self.up_axis_idx] = 0.0
        self.prev_potentials[env_ids] = -torch.norm(to_target, p=2, dim=-1) / self.dt
        self.potentials[env_ids] = self.prev_potentials[env_ids].clone()
        self.progress_buf[env_ids] = 0
        self.reset_buf[env_ids] = 0

    def compute_observations(self):
        self.gym.refresh_dof_state_tensor(self.sim)
        self.gym.refresh_actor_root_state_tensor(self.sim)
        self.gym.refresh_force_sensor_tensor(self.sim)
        self.gym.refresh_dof_force_tensor(self.sim)
        obs, pot, prev, up, heading = compute_humanoid_observations(
            self.root_states, self.targets, self.potentials, self.inv_start_rot, self.dof_pos, self.dof_vel,
            self.dof_force_tensor, self.dof_limits_lower, self.dof_limits_upper, self.dof_vel_scale,
            self.vec_sensor_tensor, self.actions, self.dt, self.contact_force_scale, self.angular_velocity_scale,
            self.basis_vec0, self.basis_vec1)
        self.obs_buf[:] = obs
        self.potentials[:] = pot
        self.prev_potentials[:] = prev
        self.up_vec[:] = up
        self.heading_vec[:] = heading

    def compute_reward(self, actions):
        self.rew_buf[:], self.reset_buf[:] = compute_humanoid_reward(
            self.obs_buf, self.reset_buf, self.progress_buf, self.actions, self.up_weight, self.heading_weight,
            self.potentials, self.prev_potentials, self.actions_cost_scale, self.energy_cost_scale,
            self.joints_at_limit_cost_scale, self.max_motor_effort, self.motor_efforts, self.termination_height,
            self.death_cost, self.max_episode_length)
        end_nonfinite_envs(self.obs_buf, self.rew_buf, self.reset_buf, self.death_cost)


def end_nonfinite_envs(obs_buf, rew_buf, reset_buf, death_cost: float):
    """Not the reference's: an env whose observation or reward is not finite (a diverged simulation) ends as a fallen
    one does -- a zero observation, the death cost, the done flag -- so that reset_idx restores it at the next step
    and nothing non-finite reaches the learner (the reference's height test is false for NaN).  In place."""
    bad = ~(torch.isfinite(obs_buf).all(dim=-1) & torch.isfinite(rew_buf))
    obs_buf[bad] = 0.0
    rew_buf[bad] = death_cost
    reset_buf[bad] = 1


def compute_humanoid_observations(root_states, targets, potentials, inv_start_rot, dof_pos, dof_vel, dof_force,
                                  lower, upper, dof_vel_scale: float, sensors, actions, dt: float,
                                  contact_force_scale: float, angular_velocity_scale: float, basis_vec0, basis_vec1):
    """humanoid.py:378-413; returns (obs, potentials, previous potentials, up vector, heading vector)."""
    pos, rot = root_states[:, 0:3], root_states[:, 3:7]
    to_target = targets - pos
    to_target[:, 2] = 0.0
    prev = potentials.clone()
    pot = -torch.norm(to_target, p=2, dim=-1) / dt
    torso_quat, up_proj, heading_proj, up_vec, heading_vec = compute_heading_and_up(
        rot, inv_start_rot, to_target, basis_vec0, basis_vec1, 2)
    vel_loc, angvel_loc, roll, _pitch, yaw, angle_to_target = compute_rot(
        torso_quat, root_states[:, 7:10], root_states[:, 10:13], targets, pos)
    n = root_states.shape[0]
    obs = torch.empty((n, HUMANOID_OBS), dtype=root_states.dtype, device=root_states.device)
    obs[:, OBS_HEIGHT] = pos[:, 2]
    obs[:, 1:4] = vel_loc
    obs[:, 4:7] = angvel_loc * angular_velocity_scale
    obs[:, 7] = normalize_angle(yaw)
    obs[:, 8] = normalize_angle(roll)
    obs[:, 9] = normalize_angle(angle_to_target)
    obs[:, OBS_UP] = up_proj
    obs[:, OBS_HEADING] = heading_proj
    obs[:, OBS_DOF_POS] = unscale(dof_pos, lower, upper)
    obs[:, OBS_DOF_VEL] = dof_vel * dof_vel_scale
    obs[:, OBS_DOF_FORCE] = dof_force * contact_force_scale
    obs[:, OBS_SENSORS] = sensors.view(-1, HUMANOID_SENSORS * 6) * contact_force_scale
    obs[:, OBS_ACTIONS] = actions
    return obs, pot, prev, up_vec, heading_vec


def compute_humanoid_reward(obs, reset_buf, progress_buf, actions, up_weight: float, heading_weight: float,
                            potentials, prev_potentials, actions_cost_scale: float, energy_cost_scale: float,
                            joints_at_limit_cost_scale: float, max_motor_effort: float, motor_efforts,
                            termination_height: float, death_cost: float, max_episode_length: float):
    """humanoid.py:324-375: progress + alive + upright + heading - action, energy and joint-limit costs, the last two
    weighted per dof by motor_efforts / max_motor_effort; a fallen torso (height below terminationHeight) pays
    deathCost and resets, as does the episode end."""
    heading = obs[:, OBS_HEADING]
    heading_reward = torch.where(heading > 0.8, torch.ones_like(heading) * heading_weight,
                                 heading_weight * heading / 0.8)
    up_reward = torch.zeros_like(heading_reward)
    up_reward = torch.where(obs[:, OBS_UP] > 0.93, up_reward + up_weight, up_reward)
    actions_cost = torch.sum(actions ** 2, dim=-1)
    ratio = motor_efforts / max_motor_effort
    scaled_cost = joints_at_limit_cost_scale * (torch.abs(obs[:, OBS_DOF_POS]) - 0.98) / 0.02
    dof_at_limit_cost = torch.sum((torch.abs(obs[:, OBS_DOF_POS]) > 0.98) * scaled_cost * ratio.unsqueeze(0), dim=-1)
    electricity_cost = torch.sum(torch.abs(actions * obs[:, OBS_DOF_VEL]) * ratio.unsqueeze(0), dim=-1)
    alive_reward = torch.ones_like(potentials) * 2.0
    progress_reward = potentials - prev_potentials
    total = (progress_reward + alive_reward + up_reward + heading_reward - actions_cost_scale * actions_cost
             - energy_cost_scale * electricity_cost - dof_at_limit_cost)
    fallen = obs[:, OBS_HEIGHT] < termination_height
    total = torch.where(fallen, torch.ones_like(total) * death_cost, total)
    reset = torch.where(fallen, torch.ones_like(reset_buf), reset_buf)
    reset = torch.where(progress_buf >= max_episode_length - 1, torch.ones_like(reset_buf), reset)
    return total, reset
