#!/usr/bin/env python3
"""Pack the reference's in-scope robot descriptions into our own JSON form.

The reference ships its robots as URDF/MJCF under ``/root/reference/assets``
(``anymal_terrain.py:212``, ``cartpole.py:76``), which is not present on the GPU
box.  This script runs *our* importer (``isaacgymenv_amd/isaacgym/_assets.py``)
over those files and stores the parsed, pre-collapse description
(links, inertials, collision geometry, joints, limits) as
``isaacgymenv_amd/assets/<name>.model.json``.  ``gym.load_asset`` parses the URDF
itself when the file exists and falls back to the packed form otherwise.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaacgymenv_amd.isaacgym._assets import parse_urdf, PACKED_DIR  # noqa: E402
from isaacgymenv_amd.isaacgym._mjcf import parse_mjcf  # noqa: E402

REF = "/root/reference/assets"
SOURCES = {
    "anymal_c.model.json": "urdf/anymal_c/urdf/anymal_minimal.urdf",
    "cartpole.model.json": "urdf/cartpole.urdf",
    "hound.model.json": "urdf/UsefulHound/urdf/Hound.urdf",
    "nv_ant.model.json": "mjcf/nv_ant.xml",
    # the fork's own quadruped (hound.py:168-183): no compiled topology, the runtime-sized kernel runs it
    "hound_new.model.json": "urdf/Hound_new/Hound.urdf",
}
# models that are test fixtures only (tests/golden/), not shipped with the package: the Houndarm task's fixed-base
# Open Manipulator P (hound_arm.py:201) and the Manipulator task's Franka Panda (manipulator.py:199; .obj collision
# meshes and no inertials: the masses come from the hulls at load time), which a user loads from the reference's own URDF
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN_SOURCES = {
    "open_manipulator_p.model.json": "urdf/open_manipulator_p_gazebo/urdf/open_manipulator_p.urdf",
    "franka_panda_manipulator.model.json": "urdf/franka_description/robots/franka_panda_manipulator.urdf",
    # the Humanoid task's body (humanoid.py:143): multi-joint bodies as hidden links, nested default classes
    "nv_humanoid.model.json": "mjcf/nv_humanoid.xml",
}


def main():
    os.makedirs(PACKED_DIR, exist_ok=True)
    for folder, sources in ((PACKED_DIR, SOURCES), (GOLDEN_DIR, GOLDEN_SOURCES)):
        for out, src in sources.items():
            path = os.path.join(REF, src)
            raw = parse_mjcf(path) if src.endswith(".xml") else parse_urdf(path)
            with open(os.path.join(folder, out), "w") as f:
                json.dump(raw.to_json(), f, indent=1)
            print("packed", src, "->", os.path.join(os.path.relpath(folder, ROOT), out))


if __name__ == "__main__":
    main()
