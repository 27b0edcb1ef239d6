"""The MJCF loader on the Humanoid's body (isaacgym/_mjcf.py, _assets.py, _model.py), on the packed fixture
tests/golden/nv_humanoid.model.json; where the reference's own nv_humanoid.xml is on the machine, the fresh parse must
equal the fixture.  Nested default classes, several joints on one body as hidden massless links, jointless bodies as
fixed children, document order, the actuator order, the pair table across hidden-link chains, and what stays
unchanged: nv_ant.xml's RawModel and every shipped packed model."""
import json
import math
import os

import numpy as np
import pytest

from isaacgymenv_amd.isaacgym import _assets, _mjcf, gymapi
from isaacgymenv_amd.isaacgym._model import flatten
from tests import helpers as H
from tests import humanoid_cases as HC


def _reference_assets():
    """Where tools/pack_assets.py reads the reference's assets from (absent on most machines)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pack_assets.py")
    spec = importlib.util.spec_from_file_location("pack_assets", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REF


REF_ASSETS = _reference_assets()
BODIES = ["torso", "head", "lower_waist", "pelvis", "right_thigh", "right_shin", "right_foot", "left_thigh", "left_shin",
          "left_foot", "right_upper_arm", "right_lower_arm", "right_hand", "left_upper_arm", "left_lower_arm",
          "left_hand"]
DOFS = ["abdomen_z", "abdomen_y", "abdomen_x", "right_hip_x", "right_hip_z", "right_hip_y", "right_knee",
        "right_ankle_y", "right_ankle_x", "left_hip_x", "left_hip_z", "left_hip_y", "left_knee", "left_ankle_y",
        "left_ankle_x", "right_shoulder1", "right_shoulder2", "right_elbow", "left_shoulder1", "left_shoulder2",
        "left_elbow"]
# <actuator> order: abdomen_y, abdomen_z, abdomen_x, hip x z y, knee, ankle x y (twice), shoulders, elbow (twice)
EFFORTS = [67.5, 67.5, 67.5, 45, 45, 135, 90, 22.5, 22.5, 45, 45, 135, 90, 22.5, 22.5, 67.5, 67.5, 45, 67.5, 67.5, 45]
# (radius, cylinder length) of every capsule and the radius of every sphere, at MuJoCo's default density 1000
CAPSULES = [(.07, .14), (.06, .12), (.06, .12), (.09, .14), (.06, math.sqrt(.01 ** 2 + .34 ** 2)),
            (.06, math.sqrt(.01 ** 2 + .34 ** 2)), (.049, .3), (.049, .3),
            (.027, math.sqrt(.21 ** 2 + .02 ** 2)), (.027, math.sqrt(.21 ** 2 + .02 ** 2)),
            (.027, math.sqrt(.21 ** 2 + .02 ** 2)), (.027, math.sqrt(.21 ** 2 + .02 ** 2)),
            (.04, .16 * math.sqrt(3)), (.04, .16 * math.sqrt(3)), (.031, .16 * math.sqrt(3)),
            (.031, .16 * math.sqrt(3))]
SPHERES = [.09, .04, .04]


def test_fresh_parse_equals_the_fixture():
    path = os.path.join(REF_ASSETS, "mjcf", "nv_humanoid.xml")
    if not os.path.isfile(path):
        pytest.skip("the reference's nv_humanoid.xml is not on this machine")
    with open(os.path.join(HC.GOLDEN, HC.MODEL)) as f:
        assert _mjcf.parse_mjcf(path).to_json() == json.load(f)


def test_public_bodies_and_dofs_in_document_order():
    art, flat = HC.load_humanoid()
    assert art.link_names() == BODIES and art.num_public_links == 16
    assert art.dof_names() == DOFS and art.num_dofs == 21
    assert art.num_bodies == 22 and flat["nb"] == 22 and flat["nr"] == 25 and art.num_links == 25
    hidden = [l for l in art.links if l.hidden]
    assert len(hidden) == 9 and all(l.hidden for l in art.links[16:]) and not any(l.hidden for l in art.links[:16])
    for l in hidden:
        b = art.bodies[l.body]
        assert b.mass == 0.0 and not np.any(b.inertia) and not b.shapes and l.mass == 0.0, l.name
    # the head and the hands are welded into their parents and reported as links
    by = {l.name: l for l in art.links}
    assert by["head"].body == by["torso"].body and by["right_hand"].body == by["right_lower_arm"].body
    assert by["left_hand"].body == by["left_lower_arm"].body
    np.testing.assert_allclose(by["head"].pose.t, [0, 0, 0.19])
    # the API's view (gymapi on a plain asset: no sim needed)
    asset = gymapi.Asset(art, gymapi.AssetOptions())
    gym = gymapi.Gym()
    assert gym.get_asset_rigid_body_count(asset) == 16 and gym.get_asset_dof_count(asset) == 21
    assert gym.find_asset_rigid_body_index(asset, "right_foot") == 6
    assert gym.find_asset_rigid_body_index(asset, "left_foot") == 9
    assert gym.get_asset_rigid_body_names(asset) == BODIES and gym.get_asset_dof_names(asset) == DOFS
    assert gym.find_asset_rigid_body_index(asset, "right_foot/right_ankle_y") == gymapi.INVALID_HANDLE
    assert [p.motor_effort for p in gym.get_asset_actuator_properties(asset)] == EFFORTS
    # within GS_MAXL / GS_MAXB / GS_MAXD / GS_MAXP and the pool of 8
    assert flat["nr"] <= 40 and flat["nb"] <= 32 and flat["nd"] <= 32 and 100 <= flat["npair"] <= 512
    assert flat["npool"] == 8


def test_total_mass_is_the_sum_over_the_geoms():
    art, _ = HC.load_humanoid()
    want = sum(_mjcf.capsule_mass_props(r, l, 1000.0)[0] for r, l in CAPSULES)
    want += sum(_mjcf.sphere_mass_props(r, 1000.0)[0] for r in SPHERES)
    assert art.num_shapes == len(CAPSULES) + len(SPHERES) == 19
    np.testing.assert_allclose(sum(b.mass for b in art.bodies), want, rtol=1e-12)
    assert 35.0 < want < 45.0


def test_joint_settings_come_from_the_right_class():
    art, flat = HC.load_humanoid()
    d = {x.name: x for x in art.dofs}
    np.testing.assert_allclose([d["right_knee"].lower, d["right_knee"].upper], np.radians([-160.0, 2.0]))
    assert all(x.has_limits for x in art.dofs)  # limited="true" of class body
    arm = dict(zip(DOFS, flat["armature"]))
    assert arm["abdomen_z"] == 0.02 and arm["abdomen_y"] == 0.01 and arm["abdomen_x"] == 0.01  # big_stiff, bigger_stiff, big
    assert arm["right_knee"] == 0.007 and arm["left_knee"] == 0.007                              # class body itself
    for j in ("right_ankle_y", "right_ankle_x", "left_ankle_y", "left_ankle_x", "right_elbow", "left_elbow"):
        assert arm[j] == 0.006, j                                                                 # small_joint
    assert min(arm.values()) >= 0.006
    assert (d["abdomen_z"].stiffness, d["abdomen_z"].damping) == (20.0, 5.0)
    assert (d["abdomen_x"].stiffness, d["abdomen_x"].damping) == (10.0, 5.0)
    assert (d["right_knee"].stiffness, d["right_knee"].damping) == (5.0, 0.1)
    assert (d["left_elbow"].stiffness, d["left_elbow"].damping) == (2.0, 1.0)
    # they reach the DOF properties' fields (and act in DOF_MODE_POS only)
    props = gymapi.Asset(art, gymapi.AssetOptions()).dof_props
    assert props["stiffness"][0] == 20.0 and props["damping"][6] == np.float32(0.1)
    # motors: ctrllimited / ctrlrange +-1 from the unnamed default, so effort = gear x 1
    np.testing.assert_array_equal([x.effort for x in art.dofs], [x.motor_gear for x in art.dofs])
    assert d["right_hip_y"].effort == 135.0 and art.default_friction == 1.0


def _eff_parent(links):
    par = [l.parent for l in links]
    for i in range(len(par)):
        while par[i] >= 0 and links[par[i]].hidden:
            par[i] = links[par[i]].parent
    return par


def test_no_pair_across_a_hidden_link_chain():
    art, flat = HC.load_humanoid()
    names = [l.name for l in art.links]
    tab = art.shape_table()
    pairs = {frozenset((names[tab[a]["link"]], names[tab[b]["link"]])) for a, b, _, _ in art.self_collision_pairs()}
    for a, b in (("torso", "lower_waist"), ("pelvis", "right_thigh"), ("pelvis", "left_thigh"),
                 ("right_shin", "right_foot"), ("left_shin", "left_foot"), ("torso", "right_upper_arm"),
                 ("torso", "left_upper_arm"), ("lower_waist", "pelvis"), ("right_thigh", "right_shin")):
        assert frozenset((a, b)) not in pairs, (a, b)
    par = _eff_parent(art.links)
    idx = {n: i for i, n in enumerate(names)}
    for p in pairs:
        a, b = (idx[n] for n in p)
        assert par[a] != b and par[b] != a and art.links[a].body != art.links[b].body
        assert not art.links[a].hidden and not art.links[b].hidden
    assert frozenset(("right_foot", "left_foot")) in pairs and frozenset(("right_hand", "torso")) in pairs
    # nothing else names a hidden link: no shape, no contact candidate, no sensor-able name
    assert all(l < 16 for l in flat["shlink"]) and all(l < 16 for l in flat["clink"])
    assert flat["npair"] == len(art.self_collision_pairs()) == 147


TWO_JOINTS = """<mujoco model="toy">
  <default><joint armature="0.01" damping="0" limited="true"/><geom density="800"/></default>
  <worldbody><body name="base" pos="0 0 1">
    <freejoint name="root"/>
    <geom type="box" size="0.1 0.1 0.1"/>
    <body name="arm" pos="0.2 0 0" {arm_attrs}>
      {joints}
      <geom type="capsule" fromto="0 0 0 0.3 0 -0.1" size="0.03"/>
      {tail}
    </body>
  </body></worldbody>
  <actuator><motor joint="b" gear="30" ctrllimited="true" ctrlrange="-2 2"/><motor joint="a" gear="10"/></actuator>
</mujoco>"""


def _toy(tmp_path, name, joints, arm_attrs="", tail=""):
    path = tmp_path / name
    path.write_text(TWO_JOINTS.format(joints=joints, arm_attrs=arm_attrs, tail=tail))
    return _mjcf.parse_mjcf(str(path))


def test_two_joints_on_one_body_equal_two_bodies_with_a_massless_link(tmp_path):
    """The same mechanism written both ways gives the same fp64 oracle trajectory: joints a then b on one body, at
    their own positions, against body `mid` (joint a, no geom) carrying body `arm` (joint b)."""
    from oracle.oracle import OracleSim
    two = _toy(tmp_path, "two.xml", '<joint name="a" axis="0 0 1" pos="0 0 0.05" range="-90 90"/>'
                                    '<joint name="b" axis="0 1 0" pos="0.02 0 0" range="-60 60"/>')
    chain = tmp_path / "chain.xml"
    chain.write_text(TWO_JOINTS.format(arm_attrs="", joints="", tail="").replace(
        '<body name="arm" pos="0.2 0 0" >', '<body name="mid" pos="0.2 0 0.05"><joint name="a" axis="0 0 1" '
        'range="-90 90"/><body name="arm" pos="0 0 -0.05"><joint name="b" axis="0 1 0" pos="0.02 0 0" range="-60 60"/>'
    ).replace("</body>\n  </body></worldbody>", "</body></body>\n  </body></worldbody>"))
    assert [l for l in two.link_order] == ["base", "arm/a", "arm"] and two.links["arm/a"].hidden
    one = _mjcf.parse_mjcf(str(chain))
    assert one.link_order == ["base", "mid", "arm"] and not one.links["mid"].hidden
    opts = dict(angular_damping=0.0)
    art2 = _assets.build_articulation(two, opts)
    art1 = _assets.build_articulation(one, opts)
    assert art2.dof_names() == art1.dof_names() == ["a", "b"] and art2.link_names() == ["base", "arm"]
    assert art2.bodies[1].mass == 0.0 and art1.bodies[1].mass == 1e-3  # hidden: exactly massless; named: the 1 g rule
    art1.bodies[1].mass, art1.bodies[1].inertia = 0.0, np.zeros((3, 3))  # the massless middle link of the comparison
    f2, f1 = flatten(art2), flatten(art1)
    params = dict(H.ANT_PARAMS)
    n = 4
    rng = np.random.RandomState(0)
    root = np.zeros((n, 13)); root[:, 2] = 1.0; root[:, 6] = 1.0; root[:, 10:13] = rng.uniform(-1, 1, (n, 3))
    dof = np.zeros((n, 2, 2)); dof[:, :, 0] = rng.uniform(-0.5, 0.5, (n, 2)); dof[:, :, 1] = rng.uniform(-2, 2, (n, 2))
    tau = rng.uniform(-1, 1, (n, 2))
    out = []
    for flat in (f2, f1):
        sim = OracleSim(flat, params)
        r, d = root.copy(), dof.copy()
        for _ in range(30):
            sim.simulate(r, d, np.ascontiguousarray(tau), np.ones((n, flat["ns"])))
        out.append((r, d))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-9, atol=1e-9)
    assert np.abs(out[0][1][:, :, 0] - dof[:, :, 0]).max() > 0.1  # it moved
    # the motors come in <actuator> order where that shows: b (30 x 2) before a (gear 10, control not limited)
    asset = gymapi.Asset(art2, gymapi.AssetOptions())
    assert two.actuator_order == ["b", "a"]
    assert [p.motor_effort for p in gymapi.Gym().get_asset_actuator_properties(asset)] == [60.0, 10.0]


def test_zero_armature_on_a_hidden_joint_is_refused(tmp_path):
    raw = _toy(tmp_path, "zero.xml", '<joint name="a" axis="0 0 1" armature="0" range="-90 90"/>'
                                     '<joint name="b" axis="0 1 0" range="-60 60"/>')
    with pytest.raises(ValueError, match="joint a .*zero armature"):
        _assets.build_articulation(raw, {})
    # the body's last joint carries the body itself: no armature needed there
    ok = _toy(tmp_path, "ok.xml", '<joint name="a" axis="0 0 1" range="-90 90"/>'
                                  '<joint name="b" axis="0 1 0" armature="0" range="-60 60"/>')
    assert _assets.build_articulation(ok, {}).num_dofs == 2


def test_childclass_and_own_class(tmp_path):
    text = TWO_JOINTS.replace('<default><joint', '<default><default class="limb"><joint damping="3" stiffness="7"/>'
                              '<default class="stiff"><joint stiffness="9" armature="0.5"/></default></default><joint')
    path = tmp_path / "cls.xml"
    path.write_text(text.format(arm_attrs='childclass="limb"', tail="",
                                joints='<joint name="a" axis="0 0 1" range="-90 90"/>'
                                       '<joint name="b" axis="0 1 0" class="stiff" range="-60 60"/>'))
    j = {x.name: x for x in _mjcf.parse_mjcf(str(path)).joints}
    assert (j["a"].damping, j["a"].stiffness, j["a"].armature) == (3.0, 7.0, 0.01)   # limb over the unnamed default
    assert (j["b"].damping, j["b"].stiffness, j["b"].armature) == (3.0, 9.0, 0.5)    # stiff over limb
    assert j["a"].has_limits and j["b"].has_limits                                  # limited from the unnamed default


def test_rigid_body_tensors_are_refused_with_the_reason():
    art, _ = HC.load_humanoid()

    class S:
        asset = gymapi.Asset(art, gymapi.AssetOptions())
    gym = gymapi.Gym()
    for fn in (gym.acquire_rigid_body_state_tensor, gym.acquire_net_contact_force_tensor):
        with pytest.raises(NotImplementedError, match="9 hidden links"):
            fn(S())


def test_ant_and_the_shipped_packed_models_are_unchanged():
    # every packed model reads and writes back to the text it has (no new key appears in a model without the
    # new features)
    shipped = [os.path.join(_assets.PACKED_DIR, f) for f in sorted(os.listdir(_assets.PACKED_DIR))
               if f.endswith(".model.json")]
    shipped += [os.path.join(HC.GOLDEN, f) for f in sorted(os.listdir(HC.GOLDEN)) if f.endswith(".model.json")]
    assert len(shipped) >= 8
    for path in shipped:
        with open(path) as f:
            d = json.load(f)
        raw = _assets.RawModel.from_json(d)
        assert raw.to_json() == d, path
        if "nv_humanoid" not in path:
            assert not raw.document_order and raw.actuator_order is None and not any(l.hidden for l in raw.links.values())
    # Ant: 9 bodies, 8 dofs, the gears, as before
    art, flat = H.ant()
    assert art.num_bodies == art.num_links == art.num_public_links == 9 and art.links is None and flat["nr"] == 9
    assert art.dof_names() == ["hip_1", "ankle_1", "hip_2", "ankle_2", "hip_3", "ankle_3", "hip_4", "ankle_4"]
    asset = gymapi.Asset(art, gymapi.AssetOptions())
    assert [p.motor_effort for p in gymapi.Gym().get_asset_actuator_properties(asset)] == [15.0] * 8
    path = os.path.join(REF_ASSETS, "mjcf", "nv_ant.xml")
    if os.path.isfile(path):  # the fresh parse is the RawModel it was
        with open(os.path.join(_assets.PACKED_DIR, "nv_ant.model.json")) as f:
            assert _mjcf.parse_mjcf(path).to_json() == json.load(f)


def test_actuator_order_compares_the_listed_efforts(tmp_path):
    """Equal gears, different control ranges, listed out of DOF order: the efforts differ, so the order is kept."""
    text = TWO_JOINTS.replace('<motor joint="b" gear="30" ctrllimited="true" ctrlrange="-2 2"/><motor joint="a" gear="10"/>',
                              '<motor joint="b" gear="10" ctrllimited="true" ctrlrange="-3 3"/>'
                              '<motor joint="a" gear="10" ctrllimited="true" ctrlrange="-1 1"/>')
    path = tmp_path / "ctrl.xml"
    path.write_text(text.format(arm_attrs="", tail="", joints='<joint name="a" axis="0 0 1" range="-90 90"/>'
                                                               '<joint name="b" axis="0 1 0" range="-60 60"/>'))
    raw = _mjcf.parse_mjcf(str(path))
    assert raw.actuator_order == ["b", "a"]
    asset = gymapi.Asset(_assets.build_articulation(raw, {}), gymapi.AssetOptions())
    assert [p.motor_effort for p in gymapi.Gym().get_asset_actuator_properties(asset)] == [30.0, 10.0]
    # the same motors in DOF order: nothing to record
    path.write_text(text.format(arm_attrs="", tail="", joints='<joint name="b" axis="0 0 1" range="-90 90"/>'
                                                               '<joint name="a" axis="0 1 0" range="-60 60"/>'))
    assert _mjcf.parse_mjcf(str(path)).actuator_order is None


FIXED_LINKS_URDF = """<robot name="fixed_links">
  <link name="base"><inertial><mass value="2"/><inertia ixx="0.1" iyy="0.1" izz="0.1" ixy="0" ixz="0" iyz="0"/></inertial></link>
  <link name="aplate"><inertial><mass value="0.5"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
  <link name="arm"><inertial><mass value="1"/><inertia ixx="0.02" iyy="0.02" izz="0.02" ixy="0" ixz="0" iyz="0"/></inertial></link>
  <link name="tip"><inertial><mass value="0.2"/><inertia ixx="0.001" iyy="0.001" izz="0.001" ixy="0" ixz="0" iyz="0"/></inertial></link>
  <joint name="plate_weld" type="fixed"><parent link="base"/><child link="aplate"/><origin xyz="0 0 0.1"/></joint>
  <joint name="shoulder" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0.2 0 0"/><axis xyz="0 1 0"/>
    <limit lower="-1" upper="1" effort="10" velocity="5"/></joint>
  <joint name="tip_weld" type="fixed"><parent link="arm"/><child link="tip"/><origin xyz="0.3 0 0"/></joint>
</robot>"""


def test_force_sensor_index_is_a_reported_link_on_an_asset_with_fixed_links(tmp_path):
    """A URDF that keeps its fixed links (collapse_fixed_joints=False): create_asset_force_sensor takes the reported
    rigid-body index, the solver the dynamic body it belongs to; a welded link has no joint reaction of its own."""
    path = tmp_path / "fixed_links.urdf"
    path.write_text(FIXED_LINKS_URDF)
    art = _assets.build_articulation(_assets.parse_urdf(str(path)), dict(collapse_fixed_joints=False))
    assert art.link_names() == ["base", "aplate", "arm", "tip"] and art.body_names() == ["base", "arm"]

    class S:
        asset = gymapi.Asset(art, gymapi.AssetOptions())
    assert gymapi.Sim._sensor_body(S(), 2) == 1  # link "arm" is body 1: passed through as a body index it would be out of range
    with pytest.raises(NotImplementedError, match="tip"):
        gymapi.Sim._sensor_body(S(), 3)
    # an asset without kept links: the index is the body's
    ant, _ = H.ant()

    class A:
        asset = gymapi.Asset(ant, gymapi.AssetOptions())
    assert [gymapi.Sim._sensor_body(A(), b) for b in H.ANT_FEET] == H.ANT_FEET
