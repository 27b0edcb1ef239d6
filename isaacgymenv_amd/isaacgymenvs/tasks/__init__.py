"""Task registry (reference ``tasks/__init__.py:90-119``), in-scope tasks only."""
from .ant import Ant
from .anymal import Anymal, Hound
from .anymal_terrain import AnymalTerrain
from .cartpole import Cartpole
from .hound_arm import Houndarm
from .humanoid import Humanoid
from .manipulator import Manipulator
from .hound_terrain import HoundTerrain
from .useful_hound import UsefulHound

isaacgym_task_map = {
    "Ant": Ant,
    "Anymal": Anymal,
    "AnymalTerrain": AnymalTerrain,
    "Cartpole": Cartpole,
    "Hound": Hound,
    "HoundTerrain": HoundTerrain,
    "Houndarm": Houndarm,
    "Humanoid": Humanoid,
    "Manipulator": Manipulator,
    "UsefulHound": UsefulHound,
}
