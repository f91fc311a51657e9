"""Reward-library terms, host side (no GPU): the numpy restatement of each term against the reference's own outputs
(tests/golden/reward_library.npz, tools/make_reward_library_golden.py), the config -> odk_reward_terms mapping, the
runner's --reward_scale / --reward_param flags and the C-ABI symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from open_duck_playground_amd import engine, joystick, runner, standing

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reward_library.npz")
f32 = np.float32


def nan_to_num(x):
    return np.nan_to_num(np.asarray(x, f32))


# ---- numpy restatement of the twelve terms, float32, one row per call: what the step kernel computes (include/odk.h odk_xterm)
def lin_vel_z(global_linvel):
    return nan_to_num(np.square(global_linvel[2]))


def ang_vel_xy(global_angvel):
    return nan_to_num(np.sum(np.square(global_angvel[:2])))


def orientation(upvector):
    return nan_to_num(np.sum(np.square(upvector[:2])))


def base_height(base_height, base_height_target):
    return nan_to_num(np.square(base_height - base_height_target))


def energy(qvel, qfrc_actuator):
    return nan_to_num(np.sum(np.abs(qvel) * np.abs(qfrc_actuator)))


def joint_pos_limits(qpos, soft_lowers, soft_uppers):
    return nan_to_num(np.sum(-np.minimum(qpos - soft_lowers, 0.0) + np.maximum(qpos - soft_uppers, 0.0)))


def termination(done):
    return f32(done)


def pose(qpos, default_pose, weights):
    return nan_to_num(np.sum(np.square(qpos - default_pose) * weights))


def feet_slip(contact, feet_vel):
    return nan_to_num(np.sum(np.sqrt(np.sum(np.square(feet_vel), axis=-1)) * contact))


def feet_clearance(feet_vel, foot_pos, max_foot_height):
    vn = np.sqrt(np.sqrt(np.sum(np.square(feet_vel[:, :2]), axis=-1)))
    return nan_to_num(np.sum(np.abs(foot_pos[:, 2] - max_foot_height) * vn))


def feet_height(swing_peak, first_contact, max_foot_height):
    return nan_to_num(np.sum(np.square(swing_peak / max_foot_height - 1.0) * first_contact))


def feet_air_time(air_time, first_contact, commands, threshold_min, threshold_max):
    a = np.minimum((air_time - threshold_min) * first_contact, threshold_max - threshold_min)
    return nan_to_num(np.sum(a) * (np.sqrt(np.sum(np.square(commands[:3]))) > 0.01))


TERMS = dict(lin_vel_z=lin_vel_z, ang_vel_xy=ang_vel_xy, orientation=orientation, base_height=base_height, energy=energy,
             joint_pos_limits=joint_pos_limits, termination=termination, pose=pose, feet_slip=feet_slip, feet_clearance=feet_clearance,
             feet_height=feet_height, feet_air_time=feet_air_time)


def golden_args(g, key):
    names = [k.split("/", 1)[1] for k in g.files if k.startswith(key + "/") and not k.endswith("/out")]
    return names


@pytest.mark.parametrize("key", list(engine.XTERM_NAMES))
def test_restatement_matches_reference_library(key):
    g = np.load(GOLDEN)
    names = golden_args(g, key)
    assert names, key
    want = g[f"{key}/out"]
    got = np.array([TERMS[key](*[g[f"{key}/{n}"][i] for n in names]) for i in range(len(want))], f32)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7)


def test_fixture_covers_edge_cases():
    g = np.load(GOLDEN)
    cmd, fc, air = g["feet_air_time/commands"], g["feet_air_time/first_contact"], g["feet_air_time/air_time"]
    zero_cmd = np.linalg.norm(cmd[:, :3], axis=1) <= 0.01
    assert zero_cmd.any() and (g["feet_air_time/out"][zero_cmd] == 0).all()
    assert (fc == 0).any() and (fc == 1).any()
    assert ((air - 0.1) * fc > 0.4).any()                                  # clipped rows
    assert (g["base_height/base_height"] == g["base_height/base_height_target"]).any()
    assert (g["joint_pos_limits/qpos"] == g["joint_pos_limits/soft_lowers"]).any()


def test_term_table_matches_header():
    hdr = engine.header_constants()
    assert hdr["NXTERM"] == 12
    for i, k in enumerate(engine.XTERM_NAMES):
        assert hdr[f"XTERM_{k.upper()}"] == i, k
    assert C.sizeof(engine.RewardTerms) == 4 * (12 + 1 + 1 + 2 + 1 + 16)


# ---- config mapping
def cfg_with(scales=None, params=None, base=joystick.default_config):
    cfg = base()
    cfg.reward_config.scales.update(scales or {})
    cfg.reward_config.update(params or {})
    return cfg


def test_no_library_term_maps_to_none():
    assert joystick.to_reward_terms(joystick.default_config(), 14) is None
    assert joystick.to_reward_terms(standing.default_config(), 14, standing.REWARD_SLOTS) is None
    # zero scales and unknown keys stay off / ignored, as in the reference
    assert joystick.to_reward_terms(cfg_with({"feet_air_time": 0.0, "no_such_term": 3.0}), 14) is None


def test_mapping_of_every_term():
    w = [0.1 * (i + 1) for i in range(14)]
    scales = {k: (i + 1) * (-1) ** i * 0.5 for i, k in enumerate(engine.XTERM_NAMES)}
    cfg = cfg_with(scales, dict(base_height_target=0.18, max_foot_height=0.03, air_time_range=[0.2, 0.6], pose_weights=w))
    t = joystick.to_reward_terms(cfg, 14)
    for i, k in enumerate(engine.XTERM_NAMES):
        assert t.scale[i] == pytest.approx(scales[k]), k
    assert t.base_height_target == pytest.approx(0.18) and t.max_foot_height == pytest.approx(0.03)
    assert list(t.air_time_range) == pytest.approx([0.2, 0.6])
    assert t.soft_joint_pos_limit_factor == pytest.approx(0.95)      # the config's own top-level key
    assert list(t.pose_weight)[:14] == pytest.approx(w) and list(t.pose_weight)[14:] == [0.0, 0.0]
    assert joystick.active_reward_terms(cfg) == list(engine.XTERM_NAMES)


def test_air_time_range_default_is_the_functions():
    t = joystick.to_reward_terms(cfg_with({"feet_air_time": 1.0}), 14)
    assert list(t.air_time_range) == pytest.approx([0.1, 0.5])


def test_native_slots_keep_their_meaning():
    # Standing: orientation is native slot 0, not the library term
    cfg = cfg_with({"orientation": -3.0, "lin_vel_z": -1.0}, base=standing.default_config)
    assert joystick.active_reward_terms(cfg, standing.REWARD_SLOTS) == ["lin_vel_z"]
    t = joystick.to_reward_terms(cfg, 14, standing.REWARD_SLOTS)
    assert t.scale[engine.XTERM_NAMES.index("orientation")] == 0.0
    ec = joystick.to_engine_config(cfg, standing=True, reward_slots=standing.REWARD_SLOTS)
    assert ec.reward_scales[0] == pytest.approx(-3.0)
    # Joystick: orientation is a library term
    cfg = cfg_with({"orientation": -3.0})
    assert joystick.active_reward_terms(cfg) == ["orientation"]
    ec = joystick.to_engine_config(cfg)
    assert list(ec.reward_scales) == pytest.approx([2.5, 6.0, -1e-3, -0.5, -0.2, 20.0, 1.0])


@pytest.mark.parametrize("term,param", [("base_height", "base_height_target"), ("feet_clearance", "max_foot_height"),
                                        ("feet_height", "max_foot_height"), ("pose", "pose_weights")])
def test_missing_parameter_is_named(term, param):
    with pytest.raises(ValueError, match=param):
        joystick.to_reward_terms(cfg_with({term: -1.0}), 14)


def test_missing_soft_limit_factor_is_named():
    cfg = cfg_with({"joint_pos_limits": -1.0})
    del cfg["soft_joint_pos_limit_factor"]
    with pytest.raises(ValueError, match="soft_joint_pos_limit_factor"):
        joystick.to_reward_terms(cfg, 14)


def test_pose_weights_of_the_wrong_length():
    with pytest.raises(ValueError, match="pose_weights"):
        joystick.to_reward_terms(cfg_with({"pose": -1.0}, {"pose_weights": [1.0] * 13}), 14)
    assert joystick.to_reward_terms(cfg_with({"pose": -1.0}, {"pose_weights": [1.0] * 12}), 12) is not None


def test_metric_names_follow_the_sign():
    assert joystick.reward_metric_name("feet_air_time", 2.0) == "reward/feet_air_time"
    assert joystick.reward_metric_name("base_height", -10.0) == "cost/base_height"


# ---- runner flags
def test_runner_flags_parse():
    args = runner.build_parser().parse_args(["--reward_scale", "feet_air_time=2.0", "--reward_scale", "base_height=-10",
                                             "--reward_param", "base_height_target=0.15", "--reward_param", "air_time_range=0.2,0.4"])
    ov = runner.reward_overrides(args.env, args.reward_scale, args.reward_param)
    assert ov == {"reward_config.scales.feet_air_time": 2.0, "reward_config.scales.base_height": -10.0,
                  "reward_config.base_height_target": 0.15, "reward_config.air_time_range": [0.2, 0.4]}
    cfg = joystick._merge(joystick.default_config(), ov)
    t = joystick.to_reward_terms(cfg, 14)
    assert t.scale[engine.XTERM_NAMES.index("feet_air_time")] == 2.0 and t.base_height_target == pytest.approx(0.15)
    # native keys are accepted too, and the soft limit factor is a top-level key
    assert runner.reward_overrides("joystick", ["alive=10"], ["soft_joint_pos_limit_factor=0.9"]) == {
        "reward_config.scales.alive": 10.0, "soft_joint_pos_limit_factor": 0.9}
    assert runner.build_parser().parse_args([]).reward_scale == []


@pytest.mark.parametrize("scales,params,match", [(["feet_airtime=1"], [], "feet_airtime"), (["imitation=1"], [], "imitation"),
                                                 ([], ["max_height=0.1"], "max_height"), (["feet_air_time"], [], "KEY=VALUE"),
                                                 ([], ["air_time_range=0.1"], "two numbers")])
def test_runner_rejects_unknown_keys(scales, params, match):
    env = "standing" if scales == ["imitation=1"] else "joystick"     # Standing has no imitation slot
    with pytest.raises(ValueError, match=match):
        runner.reward_overrides(env, scales, params)


def test_new_symbols_exported():
    if not os.path.exists(engine.LIB_PATH):
        pytest.fail(f"{engine.LIB_PATH} missing: build() first")
    lib = C.CDLL(engine.LIB_PATH)
    for name in ("odk_batch_set_reward_terms", "odk_batch_bind_reward_metrics"):
        assert hasattr(lib, name), name
        assert name in engine.EXPORTED_SYMBOLS


def test_blob_carries_the_global_linvel_address():
    from open_duck_playground_amd.model import load_task_model
    from open_duck_playground_amd.tables import build_kernel_tables
    m = load_task_model("flat_terrain")
    tabs = build_kernel_tables(m.a)
    sid = m.sensor_id("global_linvel")
    assert sid >= 0 and int(tabs["k_adr_global_linvel"][0]) == int(m.a["sensor_adr"][sid])
