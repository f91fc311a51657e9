"""The Standing task's head-joint map on the host (standing.head_joint_map, the `head_joints` config key, runner / track --head_joints):
name resolution and its refusals, the posture-command ranges of unmapped slots, the exported symbol; no GPU."""
import os

import numpy as np
import pytest

from open_duck_playground_amd import constants, engine, joystick, runner, standing, track
from open_duck_playground_amd.model import Model, load_task_model

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")


def _robot(name):
    return Model.from_xml(os.path.join(ASSETS, name))


def test_the_duck_resolves_to_its_actuators_5_to_8():
    m = load_task_model("flat_terrain")
    assert standing.head_joint_map(m, {s: s for s in constants.HEAD_SLOTS}) == [5, 6, 7, 8]
    assert standing.head_joint_map(m, {"head_yaw": "head_yaw"}) == [-1, -1, 7, -1]
    assert standing.head_joint_map(m, {}) == [-1] * 4


def test_biped12_neck_resolves_to_its_neck_actuators():
    m = _robot("biped12_neck.xml")
    assert standing.head_joint_map(m, {"neck_pitch": "neck_a", "head_yaw": "neck_b"}) == [12, -1, 13, -1]
    assert standing.head_joint_map(m, {"head_roll": "neck_a"}) == [-1, -1, -1, 12]
    assert standing.head_joint_map(m, {}) == [-1] * 4
    line = standing.describe_head_joint_map(m, [12, -1, 13, -1])
    assert "neck_pitch=neck_a (actuator 12" in line and "head_pitch=-" in line and "head_yaw=neck_b (actuator 13" in line


def test_other_robots_resolve_their_non_leg_joints():
    assert standing.head_joint_map(_robot("tail_biped.xml"), {"neck_pitch": "tail_pitch_1", "head_roll": "tail_roll"}) == [6, -1, -1, 9]
    assert standing.head_joint_map(_robot("biped_arms.xml"), {"head_pitch": "left_elbow", "head_yaw": "right_shoulder_pitch"}) == [-1, 13, 14, -1]
    assert standing.head_joint_map(_robot("biped12.xml"), {}) == [-1] * 4


@pytest.mark.parametrize("spec, match", [
    ({"neck_yaw": "neck_a"}, "unknown slot 'neck_yaw'"),
    ({"neck_pitch": "neck_c"}, "no joint 'neck_c'"),
    ({"neck_pitch": "floating_base"}, "no actuator drives joint 'floating_base'"),
    ({"neck_pitch": "neck_a", "head_pitch": "neck_a"}, "'neck_a' is used twice"),
    ({"neck_pitch": "left_knee"}, "'left_knee' is a leg joint"),
    (["neck_a"], "a dict from head slot"),
])
def test_bad_maps_are_refused_by_name(spec, match):
    with pytest.raises(ValueError, match=match):
        standing.head_joint_map(_robot("biped12_neck.xml"), spec)


def test_a_joint_that_two_actuators_drive_is_refused():
    m = _robot("biped12_neck.xml")
    trn = np.array(m.a["actuator_trnid"]).copy()
    trn.reshape(m.nu, -1)[13, 0] = trn.reshape(m.nu, -1)[12, 0]      # actuator 13 drives neck_a as well
    twice = Model({**m.a, "actuator_trnid": trn}, xml_path=m.xml_path)
    with pytest.raises(ValueError, match="'neck_a' is driven by 2 actuators"):
        standing.head_joint_map(twice, {"neck_pitch": "neck_a"})


def test_a_leg_of_the_duck_is_refused():
    with pytest.raises(ValueError, match="'right_knee' is a leg joint"):
        standing.head_joint_map(load_task_model("flat_terrain"), {"head_pitch": "right_knee"})


def _ranges(c):
    return [tuple(c.cmd_range[k]) for k in range(7)]


def test_unmapped_slots_sample_a_zero_range_and_mapped_slots_keep_theirs():
    cfg = joystick._merge(standing.default_config(), {"head_range_factor": 0.5})
    default = _ranges(standing.to_standing_engine_config(cfg))
    f = 0.5
    assert default[:3] == [(0.0, 0.0)] * 3
    expect = [[x * f for x in cfg[k + "_range"]] for k in constants.HEAD_SLOTS]
    np.testing.assert_allclose(default[3:], expect, rtol=1e-6)
    assert _ranges(standing.to_standing_engine_config(cfg, head_map=[5, 6, 7, 8])) == default
    partial = _ranges(standing.to_standing_engine_config(cfg, head_map=[12, -1, 13, -1]))
    assert partial[:3] == default[:3] and partial[3] == default[3] and partial[5] == default[5]
    assert partial[4] == (0.0, 0.0) and partial[6] == (0.0, 0.0)
    assert _ranges(standing.to_standing_engine_config(cfg, head_map=[-1] * 4))[3:] == [(0.0, 0.0)] * 4
    # everything else of the config is what the task without a map gets
    a, b = standing.to_standing_engine_config(cfg), standing.to_standing_engine_config(cfg, head_map=[-1] * 4)
    for name, _ in engine.EnvConfig._fields_:
        if name != "cmd_range":
            va, vb = getattr(a, name), getattr(b, name)
            assert (list(va) if hasattr(va, "__len__") else va) == (list(vb) if hasattr(vb, "__len__") else vb), name


def test_head_joints_is_not_a_default_config_key():
    assert "head_joints" not in standing.default_config() and "head_joints" not in joystick.default_config()


def test_the_joystick_task_refuses_head_joints():
    with pytest.raises(ValueError, match="head_joints"):
        joystick.Joystick(xml_path=os.path.join(ASSETS, "biped12.xml"), num_envs=8, config_overrides={"head_joints": {}})


def test_runner_flag():
    p = runner.build_parser()
    args = p.parse_args(["--env", "standing", "--xml", "tests/assets/biped12_neck.xml", "--head_joints", "neck_pitch=neck_a,head_yaw=neck_b"])
    assert runner.config_overrides(args)["head_joints"] == {"neck_pitch": "neck_a", "head_yaw": "neck_b"}
    args = p.parse_args(["--env", "standing", "--head_joints", "none"])
    assert runner.config_overrides(args)["head_joints"] == {}
    args = p.parse_args(["--env", "standing"])
    assert "head_joints" not in (runner.config_overrides(args) or {})
    args = p.parse_args(["--env", "joystick", "--head_joints", "none"])
    with pytest.raises(ValueError, match="--head_joints is a flag of --env standing"):
        runner.config_overrides(args)
    for bad in ("neck_a", "neck_pitch=neck_a,neck_pitch=neck_b", ","):
        with pytest.raises(ValueError, match="--head_joints"):
            runner.parse_head_joints(bad)


def test_track_flag():
    p = track.build_parser()
    args = p.parse_args(["--checkpoint", "x.pt", "--env", "standing", "--xml", "tests/assets/biped12_neck.xml",
                         "--head_joints", "neck_pitch=neck_a", "--command", "0", "0", "0"])
    assert track.config_overrides(args)["head_joints"] == {"neck_pitch": "neck_a"}
    args = p.parse_args(["--checkpoint", "x.pt", "--env", "standing", "--head_joints", "NONE", "--command", "0", "0", "0"])
    assert track.config_overrides(args)["head_joints"] == {}
    args = p.parse_args(["--checkpoint", "x.pt", "--head_joints", "neck_pitch=neck_a", "--command", "0", "0", "0"])
    with pytest.raises(ValueError, match="--env standing"):
        track.config_overrides(args)


def test_a_flag_of_the_other_env_is_refused_before_any_gpu_work(monkeypatch, capsys):
    def no_gpu(*a, **k):
        raise AssertionError("reached GPU set-up")
    monkeypatch.setattr(runner, "OpenDuckMiniV2Runner", no_gpu)
    monkeypatch.setattr(track, "run", no_gpu)
    with pytest.raises(SystemExit) as e:
        runner.main(["--env", "joystick", "--head_joints", "none"])
    assert e.value.code == 2 and "--head_joints is a flag of --env standing" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        track.main(["--checkpoint", "x.pt", "--head_joints", "neck_pitch=neck_a", "--command", "0", "0", "0"])
    assert e.value.code == 2 and "--head_joints is a flag of --env standing" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        runner.main(["--env", "standing", "--head_joints", "neck_a"])
    assert e.value.code == 2 and "expected KEY=VALUE" in capsys.readouterr().err


def test_the_setter_is_exported():
    assert "odk_batch_set_head_joints" in engine.EXPORTED_SYMBOLS
    L = engine.load_library()
    assert hasattr(L, "odk_batch_set_head_joints")
    hdr = open(os.path.join(os.path.dirname(ASSETS), "..", "include", "odk.h")).read()
    assert "int odk_batch_set_head_joints(odk_batch* b, const int32_t* actuator, int n);" in hdr
