"""HoundTerrain: the Hound quadruped on AnymalTerrain's task (reference ``tasks/Hound_terrain.py``).

The reference file is ``anymal_terrain.py`` with another robot, so this class is AnymalTerrain with its differences
only (line numbers are Hound_terrain.py's):

* asset options (:218-229): ``collapse_fixed_joints`` from the config (false: the four ``*_foot`` links stay behind
  their fixed joints), cylinders stay cylinders, visual attachments are not flipped;
* link names (:247-258, :293-302): ``base_indices`` = every link whose name contains ``baseName`` (the four
  shoulders), ``base_index`` = ``"trunk"``, actor ``"houndterrain"`` with collision filter 0 (self-collision on);
* ``check_termination`` (:304-310): trunk, any thigh, any shoulder contact, or the episode limit --
  ``allowKneeContacts`` is read from the config and never used;
* ``compute_reward`` (:347): the base-height term targets 0.48; the collision term still counts thighs only.

The observations (188), friction buckets, push, commands, noise, ``reset_idx`` with its draws and the terrain
classes are AnymalTerrain's, and so are the fused hooks of the GPU pipeline: the physics step is one
``gs_sim_pd_step`` launch (the runtime-sized kernel, kernel_variant 4: no topology is compiled for this robot) and
the tail runs libgymtask's AnymalTerrain kernels with ``gt_anymal_variant`` (``tail_variant`` below).

Limits, both refused by libgymsim with its own message when the sim is built: ``terrainType: trimesh`` (the
runtime-sized kernel has plane contacts only) and ``sim_device=cpu`` (no host solver for this topology).
"""
from __future__ import annotations

import torch

from .anymal_terrain import AnymalTerrain


class HoundTerrain(AnymalTerrain):
    actor_name = "houndterrain"
    base_link_name = "trunk"
    base_height_target = 0.48

    def _asset_options(self):
        opts = super()._asset_options()
        opts.collapse_fixed_joints = self.cfg["env"]["urdfAsset"]["collapseFixedJoints"]
        opts.replace_cylinder_with_capsule = False
        opts.flip_visual_attachments = False
        return opts

    def _create_envs(self, num_envs, spacing, num_per_row):
        super()._create_envs(num_envs, spacing, num_per_row)
        base = self.cfg["env"]["urdfAsset"]["baseName"]
        base_names = [s for s in self.body_names if base in s]
        self.base_indices = torch.zeros(len(base_names), dtype=torch.long, device=self.device, requires_grad=False)
        for i, n in enumerate(base_names):
            self.base_indices[i] = self.gym.find_actor_rigid_body_handle(self.envs[0], self.anymal_handles[0], n)

    @property
    def tail_variant(self):
        """gt_anymal_variant (include/gymtask.h) for the fused tail: (base height target, thigh contacts terminate
        whatever allowKneeContacts says, the extra terminating links)."""
        return self.base_height_target, True, self.base_indices.tolist()

    def check_termination(self):
        cf = self.contact_forces
        self.reset_buf = torch.norm(cf[:, self.base_index, :], dim=1) > 1.0
        self.reset_buf = self.reset_buf | torch.any(torch.norm(cf[:, self.knee_indices, :], dim=2) > 1.0, dim=1)
        self.reset_buf = self.reset_buf | torch.any(torch.norm(cf[:, self.base_indices, :], dim=2) > 1.0, dim=1)
        time_out = self.progress_buf >= self.max_episode_length - 1
        self.reset_buf = self.reset_buf | time_out
