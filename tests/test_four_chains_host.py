"""A biped with arms (tests/assets/biped_arms.xml): a floating base with FOUR serial chains below it (legs 6 / 6, arms 2 / 2), 22 dofs,
16 actuators, 20 bodies.  The kernel tables, the loader (host-only `odk_model_load`), the compiled shape it matches, and the refusal of a
fifth chain.  No GPU."""
import os
import re
import tempfile

import numpy as np
import pytest

from conftest import ROOT

ARMS = ("biped_arms.xml", "biped_arms_between.xml")
LEGS = ["left_hip_yaw", "left_hip_roll", "left_hip_pitch", "left_knee", "left_ankle_pitch", "left_ankle_roll",
        "right_hip_yaw", "right_hip_roll", "right_hip_pitch", "right_knee", "right_ankle_pitch", "right_ankle_roll"]


def _model(name):
    from open_duck_playground_amd.model import Model
    return Model.from_xml(os.path.join(ROOT, "tests", "assets", name), sim_dt=0.002)


def _five_chains(tail_on):
    """biped_arms.xml with one-joint arms (forearms dropped) and a one-joint tail on `tail_on`: 19 bodies, 21 dofs, five chains"""
    from open_duck_playground_amd.model import Model
    src = open(os.path.join(ROOT, "tests", "assets", "biped_arms.xml")).read()
    src = re.sub(r'\s*<body name="(left|right)_forearm".*?</body>', "", src, flags=re.S)
    src = re.sub(r'\s*<position name="(left|right)_elbow"[^>]*/>', "", src)
    tail = ('<body name="tail" pos="-0.06 0 0.02"><inertial pos="-0.03 0 0" mass="0.05" fullinertia="1e-5 2e-5 2e-5 0 0 0"/>'
            '<joint name="tail_yaw" axis="0 0 1" range="-0.6 0.6"/></body>')
    anchor = {"trunk": '<body name="left_hip_yaw_link"', "base": '<body name="trunk"'}[tail_on]
    src = src.replace(anchor, tail + anchor, 1)
    # home pose: the tail's hinge is the first (its body is declared first), the arms keep their shoulders; no tail actuator
    src = src.replace('qpos="0 0 0.34 1 0 0 0  ', 'qpos="0 0 0.34 1 0 0 0  0 ').replace("0.2 -0.4  0.2 -0.4\"", "0.2 0.2\"").replace("0.2 -0.4 0.2 -0.4\"", "0.2 0.2\"")
    with tempfile.NamedTemporaryFile("w", suffix=".xml", delete=False) as f:
        f.write(src)
    try:
        return Model.from_xml(f.name, sim_dt=0.002)
    finally:
        os.unlink(f.name)


@pytest.mark.parametrize("xml,chains", [("biped_arms.xml", [6, 6, 2, 2]), ("biped_arms_between.xml", [6, 2, 2, 6])])
def test_kernel_tables_hold_four_chains(xml, chains):
    from open_duck_playground_amd.tables import build_kernel_tables
    m = _model(xml)
    assert (m.nq, m.nv, m.nu, m.nbody, m.njnt) == (23, 22, 16, 20, 17)
    t = build_kernel_tables(m.a)
    assert int(t["k_nchain"][0]) == 4 and list(t["k_chain_len"]) == chains
    assert list(t["k_chain_first"]) == list(6 + np.concatenate([[0], np.cumsum(chains)[:-1]]))
    trunk = list(map(str, m.a["names_body"])).index("trunk")
    assert t["k_body_children"].shape == (20, 4) and int(t["k_body_nchild"][trunk]) == 4 and (t["k_body_children"][trunk] > trunk).all()


def test_second_leg_hangs_below_the_first_foot_with_the_arms_between():
    """The virtual (Hessian) tree of foot-foot contact: the right leg's first dof hangs below the left foot's last dof, also when the
    arms' dofs lie between the two legs in dof order."""
    from open_duck_playground_amd.tables import build_kernel_tables
    for xml, r_first in (("biped_arms.xml", 12), ("biped_arms_between.xml", 16)):
        t = build_kernel_tables(_model(xml).a)
        depth, anc = t["k_vdof_depth"], t["k_vdof_anc"]
        assert int(depth[r_first]) == 12 and int(anc[r_first, 1]) == 11      # parent (anc[d, 1]): the left ankle roll
        arm = 18 if xml == "biped_arms.xml" else 12
        assert int(t["k_dof_depth"][arm]) == 6 and int(depth[arm]) == 6       # the arms stay on the base
        assert int(t["k_nH"][0]) == 201 and int(t["k_nM"][0]) == 165


@pytest.mark.parametrize("xml", ARMS)
def test_the_loader_takes_a_biped_with_arms(xml):
    from open_duck_playground_amd import engine
    m = _model(xml)
    red = engine.model_reduction(m)
    assert red["paired"] == 0 and (red["nvr"], red["nMr"], red["nHr"]) == (22, 165, 201)
    assert engine.model_obs_sizes(m, 0) == (113, 230)
    # every serial body chain in one 16-lane row, in order (the DPP chain scans)
    lanes = engine.model_body_lanes(m, 32)
    assert sorted(b for b in lanes if b >= 0) == list(range(20))
    for names in (["left_hip_yaw_link", "left_hip_roll_link", "left_thigh", "left_shank", "left_ankle_link", "left_foot_link"],
                  ["right_shoulder_link", "right_forearm"]):
        ids = [list(map(str, m.a["names_body"])).index(n) for n in names]
        at = [lanes.index(b) for b in ids]
        assert at == list(range(at[0], at[0] + len(at))) and at[0] // 16 == at[-1] // 16


def test_five_chains_are_refused_by_name():
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.tables import build_kernel_tables
    m = _five_chains("base")          # the tail on the base body: no body has more than four children
    assert (m.nbody, m.nv) == (19, 21)
    with pytest.raises(ValueError, match="5 serial chains below the floating base: the kernels take at most four"):
        build_kernel_tables(m.a)
    with pytest.raises((ValueError, engine.OdkError), match="at most four"):
        engine.model_reduction(m)
    with pytest.raises(ValueError, match="more than four child bodies"):      # the tail on the trunk: five children
        build_kernel_tables(_five_chains("trunk").a)


def test_arm_joints_are_not_leg_joints():
    from open_duck_playground_amd import constants
    for xml in ARMS:
        robot = constants.robot_of(_model(xml))
        assert not robot.is_open_duck and list(robot.joints_order_no_head) == LEGS


def test_new_shape_emits_the_chain_count_of_the_compiled_shape():
    import importlib.util
    spec = importlib.util.spec_from_file_location("new_shape", os.path.join(ROOT, "tools", "new_shape.py"))
    ns = importlib.util.module_from_spec(spec); spec.loader.exec_module(ns)
    line, dims, chains = ns.shape_line(_model("biped_arms.xml"))
    assert chains == [6, 6, 2, 2] and line.endswith(", false, 6, true, 4>;"), line
    args = re.search(r"Shape<([^>]*)>", line).group(1)
    src = open(os.path.join(ROOT, "open_duck_playground_amd", "csrc", "odk_shapes.h")).read()
    assert f"using ShapeE = Shape<{args}>;" in src and "X(16, ShapeE)" in src
    assert ns.shape_line(_model("biped_arms_between.xml"))[0] == line
    # three chains: the default, not spelled out
    assert ns.shape_line(_model("biped12.xml"))[0].endswith(", false, 6, true>;")
