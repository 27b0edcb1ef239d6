"""Set-up refusals around the runtime-sized kernel (gs_generic.hip, kernel_variant 4): what it still does not run
is refused where it is set up, with a message that names the reason or the table limit (no silent fallback).

The host backend and the table limits are checked without a GPU (gs_sim_set_model refuses before any device call);
a terrain mesh under the runtime-sized kernel needs a GPU sim to be asked for at all, so that test is marked gpu.
"""
import numpy as np
import pytest

from tests import helpers as H


def _chain_urdf(links):
    """A chain of `links` links on hinges, a sphere on each."""
    out = ['<robot name="chain">']
    for i in range(links):
        out.append(f'<link name="l{i}"><inertial><mass value="0.5"/>'
                   '<inertia ixx="0.001" iyy="0.001" izz="0.001" ixy="0" ixz="0" iyz="0"/></inertial>'
                   '<collision><geometry><sphere radius="0.02"/></geometry></collision></link>')
    for i in range(1, links):
        out.append(f'<joint name="j{i}" type="revolute"><parent link="l{i - 1}"/><child link="l{i}"/>'
                   '<origin xyz="0.05 0 0"/><axis xyz="0 1 0"/>'
                   '<limit lower="-1" upper="1" effort="10" velocity="10"/></joint>')
    out.append("</robot>")
    return "".join(out)


def _prepare(tmp_path, urdf, host, terrain=None):
    from isaacgymenv_amd.isaacgym import gymapi
    (tmp_path / "robot.urdf").write_text(urdf)
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.dt, sp.substeps, sp.up_axis = 0.005, 1, gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -9.81)
    sp.use_gpu_pipeline = sp.physx.use_gpu = not host
    sp.physx.solver_type = 0
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    gym.add_ground(sim, gymapi.PlaneParams())
    if terrain is not None:
        tm = gymapi.TriangleMeshParams()
        tm.nb_vertices = terrain["vertices"].shape[0]
        tm.nb_triangles = terrain["triangles"].shape[0]
        tm.transform.p = gymapi.Vec3(*terrain["shift"])
        gym.add_triangle_mesh(sim, terrain["vertices"].flatten(), terrain["triangles"].flatten(), tm)
    asset = gym.load_asset(sim, str(tmp_path), "robot.urdf", gymapi.AssetOptions())
    env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 1)
    gym.create_actor(env, asset, gymapi.Transform(), "robot", 0, 1, 0)
    gym.prepare_sim(sim)
    return sim


def test_host_backend_refuses_a_robot_without_a_compiled_topology(tmp_path):
    """A 5-link chain matches no compiled topology; the sim_device=cpu pipeline says that the runtime-sized kernel is
    a GPU kernel."""
    with pytest.raises(RuntimeError, match="runtime-sized kernel is a GPU kernel"):
        _prepare(tmp_path, _chain_urdf(5), host=True)


def test_a_model_beyond_a_table_limit_is_refused_naming_the_limit(tmp_path):
    """33 bodies: one more than the 32-bit ancestor masks hold.  The refusal names the count, the table and its
    limit."""
    with pytest.raises(RuntimeError, match=r"33 bodies \(32-bit ancestor masks\) exceed the limit of 32"):
        _prepare(tmp_path, _chain_urdf(33), host=True)


@pytest.mark.gpu
def test_terrain_mesh_on_the_runtime_kernel_is_refused(tmp_path):
    """A heightfield mesh under a robot without a compiled topology: the runtime-sized kernel has plane contacts
    only and says so."""
    hf = np.zeros((20, 20), dtype=np.int16)
    with pytest.raises(RuntimeError, match="terrain mesh: the runtime-sized kernel has plane contacts only"):
        _prepare(tmp_path, _chain_urdf(5), host=False, terrain=H.terrain_from_heights(hf, shift=(-1.0, -1.0, 0.0)))


@pytest.mark.gpu
def test_a_chain_of_32_bodies_runs_on_the_runtime_kernel(tmp_path):
    """The limit itself is usable: 32 bodies (31 dofs, 37 velocity components) simulate and stay finite."""
    import torch
    from isaacgymenv_amd.isaacgym import gymapi
    sim = _prepare(tmp_path, _chain_urdf(32), host=False)
    assert sim.kernel_variant == 4
    gym = gymapi.acquire_gym()
    for _ in range(5):
        gym.simulate(sim)
    torch.cuda.synchronize()
    assert torch.isfinite(sim.state).all()
