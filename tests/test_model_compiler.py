"""G3: the model compiler against known answers derived from the reference URDFs,
plus a synthetic URDF exercising collapse_fixed_joints / dont_collapse / capsule conversion."""
import json
import os
import textwrap

import numpy as np
import pytest

from legged_games_gym_amd.envs import configs
from legged_games_gym_amd.utils.model_compiler import compile_urdf, load_model, rpy_to_matrix

REF = "/root/reference"


def test_shipped_anymal_table_known_answers(golden_dir):
    m = load_model("anymal_c.urdf")
    g = json.load(open(os.path.join(golden_dir, "models.json")))["anymal_c"]
    assert (m.num_bodies, m.num_dof, m.num_shapes) == (17, 12, 13) == (g["num_bodies"], g["num_dof"], g["num_shapes"])
    assert abs(m.total_mass - 52.13485) < 1e-4
    assert m.body_names[:5] == ["base", "LF_HIP", "LF_THIGH", "LF_SHANK", "LF_FOOT"]
    assert m.dof_names == ["LF_HAA", "LF_HFE", "LF_KFE", "LH_HAA", "LH_HFE", "LH_KFE", "RF_HAA", "RF_HFE", "RF_KFE", "RH_HAA", "RH_HFE", "RH_KFE"]
    np.testing.assert_allclose(m.report_mass[:5], [26.373, 2.781, 3.071, 0.33842, 0.25], atol=2e-3)
    q0 = np.array([configs.AnymalCRoughCfg.init_state.default_joint_angles[n] for n in m.dof_names])
    feet = m.report_body_positions(q0)[m.bodies_matching("FOOT")]
    expect = np.array([[0.46143, 0.30116, -0.53954], [-0.46143, 0.30116, -0.53954], [0.46143, -0.30116, -0.53954], [-0.46143, -0.30116, -0.53954]])
    np.testing.assert_allclose(feet, expect, atol=2e-5)
    np.testing.assert_allclose(m.report_body_positions(np.zeros(12))[4], [0.44775, 0.30116, -0.62297], atol=2e-5)
    np.testing.assert_allclose(m.center_of_mass(q0), [-0.0090, -0.0001, -0.0633], atol=2e-4)
    np.testing.assert_allclose(feet, g["feet_default_pose"], atol=1e-9)
    # lowest point of the foot sphere: z = -0.54882 in the base frame (5.1 cm drop from the 0.6 m spawn)
    Rs, ps = m.forward_kinematics(q0)
    foot_pt = [c for c in m.limb_points[0] if c.report_body == 4][0]
    assert abs((ps[2] + Rs[2] @ foot_pt.pos)[2] - foot_pt.radius + 0.54882) < 2e-5
    assert m.bodies_matching("SHANK") + m.bodies_matching("THIGH") == [3, 7, 11, 15, 2, 6, 10, 14] and m.bodies_matching("base") == [0]


def test_shipped_cassie_table_known_answers():
    m = load_model("cassie.urdf")
    assert (m.num_bodies, m.num_dof, m.num_shapes, m.num_limbs, m.chain_len) == (13, 12, 3, 2, 6)
    assert abs(m.total_mass - 30.468) < 1e-4 and m.body_names[0] == "pelvis"
    q0 = np.array([configs.CassieRoughCfg.init_state.default_joint_angles[n] for n in m.dof_names])
    toes = m.report_body_positions(q0)[m.bodies_matching("toe")]
    np.testing.assert_allclose(toes, [[0.00931, 0.20968, -0.78935], [0.00931, -0.20968, -0.78935]], atol=2e-5)
    np.testing.assert_allclose(m.center_of_mass(q0), [-0.0011, 0.0, -0.0818], atol=2e-4)
    assert m.dof_has_limits.all() and abs(m.dof_lower[3] + 2.8623) < 1e-6 and abs(m.dof_effort[5] - 45) < 1e-6


def test_shipped_a1_table_known_answers(golden_dir):
    """A1 (12.454 kg; a1.urdf boxes -> sphere-swept points, model_compiler._box_points)."""
    m = load_model("a1.urdf")
    g = json.load(open(os.path.join(golden_dir, "models.json")))["a1"]
    assert (m.num_bodies, m.num_dof, m.num_shapes, m.num_limbs, m.chain_len) == (17, 12, 13, 4, 3)
    assert (g["num_bodies"], g["num_dof"], g["num_shapes"]) == (17, 12, 13)
    assert abs(m.total_mass - 12.454) < 1e-4 and m.body_names[0] == "base"
    assert m.body_names[1:5] == ["FL_hip", "FL_thigh", "FL_calf", "FL_foot"]
    assert m.dof_names[:3] == ["FL_hip_joint", "FL_thigh_joint", "FL_calf_joint"] and m.dof_names[9:] == ["RR_hip_joint", "RR_thigh_joint", "RR_calf_joint"]
    assert m.bodies_matching("foot") == [4, 8, 12, 16] and m.bodies_matching("base") == [0]
    # trunk box 0.267 x 0.194 x 0.114 -> four spheres of radius 0.057 at the inset corners: bottom face preserved
    assert len(m.base_points) == 4
    for c in m.base_points:
        assert abs(c.radius - 0.057) < 1e-9 and abs(abs(c.pos[0]) - (0.1335 - 0.057)) < 1e-9 and abs(abs(c.pos[1]) - (0.097 - 0.057)) < 1e-9
    # per leg: thigh rod (2), calf rod (2), foot sphere r=0.02
    for k in range(4):
        pts = m.limb_points[k]
        assert list(m.limb_point_joint[k]) == [1, 1, 2, 2, 2] and abs(pts[4].radius - 0.02) < 1e-12
        assert abs(pts[0].radius - 0.25 * (0.0245 + 0.034)) < 1e-9 and abs(pts[2].radius - 0.008) < 1e-9
    # standing height: feet 0.2 m links, default pose (0.8 / -1.5) -> foot centre below the hip
    q0 = np.array([configs.A1RoughCfg.init_state.default_joint_angles[n] for n in m.dof_names])
    feet = m.report_body_positions(q0)[m.bodies_matching("foot")]
    np.testing.assert_allclose(feet, g["feet_default_pose"], atol=1e-9)
    z = -0.2 * np.cos(0.8) - 0.2 * np.cos(0.8 - 1.5)      # hip roll 0.1 rad scales z by cos(0.1) up to the 8.5 cm lateral offset
    assert abs(feet[0][2] - (z * np.cos(0.1) + 0.08505 * np.sin(0.1))) < 1e-4     # FL: +y offset rolled by +0.1 rad lifts the foot


def test_shipped_anymal_b_table_known_answers(golden_dir):
    m = load_model("anymal_b.urdf")
    g = json.load(open(os.path.join(golden_dir, "models.json")))["anymal_b"]
    assert (m.num_bodies, m.num_dof, m.num_shapes) == (17, 12, 13) == (g["num_bodies"], g["num_dof"], g["num_shapes"])
    assert abs(m.total_mass - g["total_mass"]) < 1e-9 and abs(m.total_mass - 30.6214) < 1e-3
    assert m.body_names[:5] == ["base", "LF_HIP", "LF_THIGH", "LF_SHANK", "LF_FOOT"]
    assert len(m.base_points) == 4 and all(abs(c.radius - 0.12) < 1e-9 and abs(c.pos[2] - 0.08) < 1e-9 for c in m.base_points)
    assert list(m.limb_point_joint[0]) == [1, 1, 2, 2, 2] and abs(m.limb_points[0][4].radius - 0.031) < 1e-12
    q0 = np.array([configs.AnymalBRoughCfg.init_state.default_joint_angles[n] for n in m.dof_names])
    np.testing.assert_allclose(m.report_body_positions(q0)[m.bodies_matching("FOOT")], g["feet_default_pose"], atol=1e-9)


def test_box_points_rules():
    from legged_games_gym_amd.utils.model_compiler import _box_points
    R = rpy_to_matrix([0, np.pi / 2, 0])                      # A1 thigh: long axis x -> -z after the pitch
    rod = _box_points([0.2, 0.0245, 0.034], R, np.array([0, 0, -0.1]), 2, 0)
    assert len(rod) == 2 and abs(rod[0].radius - 0.014625) < 1e-12
    zs = sorted(c.pos[2] for c in rod)
    np.testing.assert_allclose(zs, [-0.2 + 0.014625, -0.014625], atol=1e-12)      # capsule spans exactly the box length
    slab = _box_points([0.4, 0.2, 0.1], np.eye(3), np.zeros(3), 0, 0)
    assert len(slab) == 4 and all(abs(c.radius - 0.05) < 1e-12 for c in slab)
    assert sorted((round(c.pos[0], 6), round(c.pos[1], 6)) for c in slab) == [(-0.15, -0.05), (-0.15, 0.05), (0.15, -0.05), (0.15, 0.05)]


@pytest.mark.parametrize("stem,rel", [("anymal_c", "resources/robots/anymal_c/urdf/anymal_c.urdf"), ("cassie", "resources/robots/cassie/urdf/cassie.urdf"),
                                      ("anymal_b", "resources/robots/anymal_b/urdf/anymal_b.urdf"), ("a1", "resources/robots/a1/urdf/a1.urdf")])
def test_compiled_table_is_fresh(stem, rel, golden_dir):
    """The shipped tables against the reference URDFs, stored as fixtures (tests/golden/urdf/); where the reference tree is present the
    fixtures must still be byte-identical to it."""
    urdf = os.path.join(golden_dir, "urdf", stem + ".urdf")
    if os.path.isfile(os.path.join(REF, rel)):
        assert open(os.path.join(REF, rel), "rb").read() == open(urdf, "rb").read(), f"{rel} changed: refresh tests/golden/urdf/{stem}.urdf"
    a, b = compile_urdf(urdf, name=stem), load_model(stem + ".urdf")
    for f in ("joint_pos", "joint_rot", "joint_axis", "body_mass", "body_com", "body_inertia", "base_inertia", "base_com"):
        np.testing.assert_allclose(getattr(a, f), getattr(b, f), atol=1e-12)
    assert a.body_names == b.body_names and a.dof_names == b.dof_names


URDF = textwrap.dedent("""\
    <robot name="toy">
      <link name="trunk"><inertial><origin xyz="0 0 0"/><mass value="2"/><inertia ixx="0.1" iyy="0.2" izz="0.3" ixy="0" ixz="0" iyz="0"/></inertial>
        <collision><origin xyz="0 0 0" rpy="0 1.5707963 0"/><geometry><cylinder length="0.4" radius="0.05"/></geometry></collision></link>
      <link name="lump"><inertial><origin xyz="0 0 0"/><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
      <joint name="weld" type="fixed"><parent link="trunk"/><child link="lump"/><origin xyz="0.3 0 0"/></joint>
      %s
    </robot>""")
LEG = """
      <link name="{p}_upper"><inertial><origin xyz="0 0 -0.1"/><mass value="0.5"/><inertia ixx="0.002" iyy="0.002" izz="0.001" ixy="0" ixz="0" iyz="0"/></inertial></link>
      <joint name="{p}_j0" type="revolute"><parent link="trunk"/><child link="{p}_upper"/><origin xyz="{x} 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/><limit effort="10" velocity="5" lower="-1" upper="1"/></joint>
      <link name="{p}_lower"><inertial><origin xyz="0 0 -0.1"/><mass value="0.25"/><inertia ixx="0.001" iyy="0.001" izz="0.0005" ixy="0" ixz="0" iyz="0"/></inertial></link>
      <joint name="{p}_j1" type="revolute"><parent link="{p}_upper"/><child link="{p}_lower"/><origin xyz="0 0 -0.2"/><axis xyz="0 1 0"/><limit effort="10" velocity="5"/></joint>
      <link name="{p}_pad"><inertial><origin xyz="0 0 0"/><mass value="0.05"/><inertia ixx="1e-5" iyy="1e-5" izz="1e-5" ixy="0" ixz="0" iyz="0"/></inertial>
        <collision><origin xyz="0 0 0"/><geometry><sphere radius="0.02"/></geometry></collision></link>
      <joint name="{p}_pad_fix" type="fixed" dont_collapse="true"><parent link="{p}_lower"/><child link="{p}_pad"/><origin xyz="0 0 -0.2"/></joint>
"""


def test_synthetic_urdf_collapse_and_order(tmp_path):
    f = tmp_path / "toy.urdf"
    f.write_text(URDF % (LEG.format(p="b", x=-0.2) + LEG.format(p="a", x=0.2)))
    m = compile_urdf(str(f))
    # siblings alphabetical: limb "a" first although "b" is first in the file; feet kept as report bodies
    assert m.body_names == ["trunk", "a_upper", "a_lower", "a_pad", "b_upper", "b_lower", "b_pad"]
    assert m.dof_names == ["a_j0", "a_j1", "b_j0", "b_j1"] and (m.num_limbs, m.chain_len) == (2, 2)
    # weld: 2 kg at 0 + 1 kg at x=0.3 -> com 0.1, Ixx unchanged, Iyy += parallel axis
    assert abs(m.base_mass - 3.0) < 1e-12 and abs(m.base_com[0] - 0.1) < 1e-12
    assert abs(m.base_inertia[1, 1] - (0.2 + 0.01 + 2 * 0.01 + 1 * 0.04)) < 1e-12
    # the pad is welded dynamically into the lower leg but reports separately
    assert abs(m.body_mass[1] - 0.30) < 1e-12 and abs(m.report_mass[3] - 0.05) < 1e-12
    assert m.limb_points[0][0].report_body == 3 and m.limb_point_joint[0] == [1]
    np.testing.assert_allclose(m.limb_points[0][0].pos, [0, 0, -0.2])
    # cylinder (axis z rotated onto x) -> capsule = two end spheres
    ends = sorted(p.pos[0] for p in m.base_points)
    np.testing.assert_allclose(ends, [-0.2, 0.2], atol=1e-6)
    assert m.dof_has_limits.tolist() == [True, False, True, False]
    np.testing.assert_allclose(rpy_to_matrix([0, 0, np.pi / 2]) @ [1, 0, 0], [0, 1, 0], atol=1e-12)
    j = m.to_json()
    m2 = type(m).from_json(j)
    np.testing.assert_allclose(m2.joint_pos, m.joint_pos)
