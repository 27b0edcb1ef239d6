"""Manipulator: operational-space reach on a fixed-base, zero-gravity 7-DoF Franka Panda (reference
``tasks/manipulator.py``), the task Houndarm was derived from.

The step logic is Houndarm's (tasks/hound_arm.py: the same 10-wide observation, reward, time-out reset and draw order),
checked against a recording of the reference's own code (tests/golden/manipulator.npz).  What differs:

* seven revolute dofs: ``J = jacobian[:, joint_dict['panda_joint7'], :, :7]`` (6 x 7), ``M = mass_matrix[:, :7, :7]``,
  so ``1 - J^T M_eef J M^-1`` is a real null-space projector and the posture term acts; ``kp_null`` has 7 entries;
* the end-effector is the body ``panda_link7``; the actor is ``"franka"``; ``flip_visual_attachments = True``;
* the default pose ``[0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854]``; the URDF's ``damping="10.0"`` is overwritten with 0
  like the stiffness (manipulator.py:231-234); effort limits 87 x 4 and 12 x 3 from the URDF;
* ``reset_idx`` (:390-452) draws ``torch.rand((k, 7))`` and, after the clamp, sets the last two joints to their
  defaults exactly (:413); their draws are consumed all the same.

On the GPU pipeline the controller is libgymtask's gt_osc_control (an env spread over 8 lanes: the 7-dof matrices do
not fit one lane's registers), the tail gt_arm_post_physics, the reset gt_manip_reset_flagged.

``controlType: joint_tor`` and ``task.randomize: True`` are refused as in Houndarm.  The arm runs the runtime-sized
kernel, GPU only.  Its model is not shipped with the package: ``env.asset.assetRoot`` and
``env.asset.assetFileNameFranka`` name the reference's URDF or a packed ``*.model.json`` of it (tools/pack_assets.py).
"""
from __future__ import annotations

from .hound_arm import Houndarm

ASSET_FILE = "urdf/franka_description/robots/franka_panda_manipulator.urdf"


class Manipulator(Houndarm):
    actor_name = "franka"
    eef_link_name, eef_joint_name = "panda_link7", "panda_joint7"
    arm_dofs = 7
    default_pose = [0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854]
    dof_noise_key, asset_file_key, asset_file = "frankaDofNoise", "assetFileNameFranka", ASSET_FILE
    flip_visual_attachments = True
    kernels_class = "ManipulatorKernels"

    def _after_reset_clamp(self, pos):
        pos[:, -2:] = self.default_dof_pos[-2:]  # manipulator.py:413
        return pos
