"""CPU checks of the posture and stillness report of `track --posture`: the C-ABI export and the slot names, the report's reduction of a
hand-written posture accumulator (an env that never leaves the tolerance, one that enters and stays, one still outside at its last sample,
an unmapped slot, an empty block), the command-line flags, the head-joint map the report names its joints from and the tensor checks of
`Batch.posture_accumulate`."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = dict(SAMPLES=0, DRIFT_SPEED_SUM=1, YAW_RATE_SQ_SUM=2, ROLLPITCH_RATE_SQ_SUM=3, TILT_SUM=4, TILT_PEAK=5, HEIGHT_SUM=6, LEG_POSE_SUM=7,
               LEG_VEL_SUM=8, HEAD_SQERR_SUM=9)
ARRAYS = dict(ANGLE_SUM=16, ERR_SQ_SUM=20, ERR_PEAK=24, LAST_OFF=28)
NACC = 32


def test_libodk_exports_the_posture_accumulator_and_the_header_names_its_slots():
    from open_duck_playground_amd import engine, track
    engine.build_library()
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "odk_posture_accumulate")
    assert "odk_posture_accumulate" in engine.EXPORTED_SYMBOLS
    names = {k[8:]: v for k, v in engine.header_constants().items() if k.startswith("POSTURE_")}
    assert names.pop("NACC") == NACC
    assert engine.POSTURE_NACC == track.POSTURE_NACC == NACC
    assert names == {**SCALARS, **ARRAYS}          # the header names these slots and no others
    for name, slot in {**SCALARS, **ARRAYS}.items():
        assert getattr(engine, "POSTURE_" + name) == slot, name
    # the four-entry arrays follow the scalars, do not overlap and end the row
    assert max(SCALARS.values()) < ARRAYS["ANGLE_SUM"] and sorted(ARRAYS.values()) == list(range(16, NACC, 4))
    assert track.HEAD_SLOTS == ("neck_pitch", "head_pitch", "head_yaw", "head_roll")
    from open_duck_playground_amd import constants
    assert tuple(constants.HEAD_SLOTS) == track.HEAD_SLOTS


def _row(**kw):
    """one accumulator row: scalars by name, arrays by name as four values"""
    r = np.zeros(NACC, np.float32)
    for k, v in kw.items():
        if k in SCALARS:
            r[SCALARS[k]] = np.float32(v)
        else:
            r[ARRAYS[k]:ARRAYS[k] + 4] = np.float32(v)
    return r


def test_posture_report_reduction():
    """Two blocks of three envs and the map [7, -1, 2, -1] (neck_pitch on actuator 7, head_yaw on actuator 2, two slots unmapped).  Block 0:
    env 0 never leaves the tolerance on either slot (LAST_OFF 0), env 1 enters it after 12 (neck_pitch) / 30 (head_yaw) samples and stays,
    env 2 is still outside on head_yaw at its last sample (LAST_OFF == SAMPLES) and ended its first episode early.  Block 1: nobody has a
    sample.  Every figure at its closed form."""
    from open_duck_playground_amd import track
    dt = 0.02
    hmap = [7, -1, 2, -1]
    joints = [f"joint_{u}" for u in range(9)]
    acc = np.stack([
        _row(SAMPLES=50, DRIFT_SPEED_SUM=1.0, YAW_RATE_SQ_SUM=2.0, ROLLPITCH_RATE_SQ_SUM=0.5, TILT_SUM=5.0, TILT_PEAK=0.25, HEIGHT_SUM=7.5, LEG_POSE_SUM=10.0,
             LEG_VEL_SUM=20.0, HEAD_SQERR_SUM=0.5, ANGLE_SUM=(25.0, 0, -10.0, 0), ERR_SQ_SUM=(0.125, 0, 0.375, 0), ERR_PEAK=(0.0625, 0, 0.09375, 0),
             LAST_OFF=(0, 0, 0, 0)),
        _row(SAMPLES=50, DRIFT_SPEED_SUM=3.0, YAW_RATE_SQ_SUM=6.0, ROLLPITCH_RATE_SQ_SUM=1.5, TILT_SUM=10.0, TILT_PEAK=0.5, HEIGHT_SUM=7.5, LEG_POSE_SUM=30.0,
             LEG_VEL_SUM=40.0, HEAD_SQERR_SUM=4.0, ANGLE_SUM=(20.0, 0, -15.0, 0), ERR_SQ_SUM=(1.0, 0, 3.0, 0), ERR_PEAK=(0.5, 0, 0.75, 0),
             LAST_OFF=(12, 0, 30, 0)),
        _row(SAMPLES=20, DRIFT_SPEED_SUM=2.0, YAW_RATE_SQ_SUM=4.0, ROLLPITCH_RATE_SQ_SUM=1.0, TILT_SUM=9.0, TILT_PEAK=0.75, HEIGHT_SUM=3.0, LEG_POSE_SUM=20.0,
             LEG_VEL_SUM=60.0, HEAD_SQERR_SUM=7.5, ANGLE_SUM=(15.0, 0, 5.0, 0), ERR_SQ_SUM=(0.5, 0, 7.0, 0), ERR_PEAK=(0.25, 0, 1.0, 0),
             LAST_OFF=(6, 0, 20, 0)),
        _row(), _row(), _row(),
    ])
    cmds = [[0, 0, 0, 0.5, 0.1, -0.25, 0.2], [0, 0, 0, 1.0, 0, 0.5, 0]]
    out = track.reduce_posture(acc, cmds, 3, dt, hmap, joints)
    assert len(out) == 2 and json.loads(json.dumps(out)) == out
    ap = pytest.approx
    g = out[0]
    # an unmapped slot is absent; the mapped ones sit under their names, in slot order
    assert tuple(g) == ("samples", "neck_pitch", "head_yaw", "head_cost_mean", "stillness")
    assert g["samples"] == 120
    np_, hy = g["neck_pitch"], g["head_yaw"]
    assert tuple(np_) == tuple(hy) == track.POSTURE_SLOT_KEYS
    assert np_["joint"] == "joint_7" and hy["joint"] == "joint_2" and np_["command"] == 0.5 and hy["command"] == -0.25
    assert np_["mean_angle"] == ap(60.0 / 120) and hy["mean_angle"] == ap(-20.0 / 120)
    assert np_["rms_error"] == ap(np.sqrt(1.625 / 120)) and hy["rms_error"] == ap(np.sqrt(10.375 / 120))
    assert np_["peak_error"] == 0.5 and hy["peak_error"] == 1.0
    # neck_pitch: all three settled, after 0, 12 and 6 samples; head_yaw: env 2 is still outside at its last sample and has no settle time
    assert np_["settled_fraction"] == 1.0 and np_["settle_time_s"] == ap((0 + 12 + 6) / 3 * dt)
    assert hy["settled_fraction"] == ap(2 / 3) and hy["settle_time_s"] == ap((0 + 30) / 2 * dt)
    assert g["head_cost_mean"] == ap(12.0 / 120)
    s = g["stillness"]
    assert tuple(s) == track.STILLNESS_KEYS
    assert s["drift_speed_mps"] == ap(6.0 / 120) and s["yaw_rate_rms"] == ap(np.sqrt(12.0 / 120)) and s["roll_pitch_rate_rms"] == ap(np.sqrt(3.0 / 120))
    assert s["tilt_mean"] == ap(24.0 / 120) and s["tilt_peak"] == 0.75 and s["root_height_mean"] == ap(18.0 / 120)
    assert s["leg_pose_deviation_mean"] == ap(60.0 / 120) and s["leg_joint_speed_mean"] == ap(120.0 / 120)

    # the empty block: nothing to average, nothing divides by zero
    e = out[1]
    assert tuple(e) == tuple(g) and e["samples"] == 0 and e["head_cost_mean"] is None
    assert e["neck_pitch"] == dict(joint="joint_7", command=1.0, mean_angle=None, rms_error=None, peak_error=None, settle_time_s=None, settled_fraction=None)
    assert e["head_yaw"]["command"] == 0.5 and all(v is None for v in e["stillness"].values())

    # nobody settled: a fraction of 0 and no time; an env without a sample counts on neither side
    late = np.stack([_row(SAMPLES=10, ERR_PEAK=(1, 0, 1, 0), LAST_OFF=(10, 0, 10, 0)), _row()])
    (h,) = track.reduce_posture(late, cmds[:1], 2, dt, hmap, joints)
    assert h["neck_pitch"]["settled_fraction"] == 0.0 and h["neck_pitch"]["settle_time_s"] is None
    # a map without any joint: the stillness part alone
    (bare,) = track.reduce_posture(acc[:3], cmds[:1], 3, dt, [-1] * 4, joints)
    assert tuple(bare) == ("samples", "head_cost_mean", "stillness") and bare["stillness"] == s


def test_posture_command_line_flags(capsys):
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt", "--command", "0", "0", "0"]
    args = track.build_parser().parse_args(base)
    assert args.posture is False and args.posture_tolerance == track.DEFAULT_POSTURE_TOLERANCE == 0.1
    args = track.build_parser().parse_args(base + ["--posture"])
    assert args.posture is True and args.posture_tolerance == 0.1
    # the tolerance alone is accepted and inert: nothing but --posture reads it
    args = track.build_parser().parse_args(base + ["--posture_tolerance", "0.25"])
    assert args.posture is False and args.posture_tolerance == 0.25
    assert track.build_parser().parse_args(base + ["--posture", "--posture_tolerance", "0"]).posture_tolerance == 0.0
    for bad in ("-0.1", "nan", "inf", "wide"):
        with pytest.raises(SystemExit):
            track.build_parser().parse_args(base + ["--posture", f"--posture_tolerance={bad}"])
        assert "--posture_tolerance" in capsys.readouterr().err
    help_text = " ".join(track.build_parser().format_help().split())
    for word in ("settle time", "cost_head_pos", "--head_joints", "read by --posture only"):
        assert word in help_text, word


def test_posture_head_map_names_the_joints(model_a):
    """The duck's default map and joint names; a Standing env's own map; the Joystick task on another robot has none and says where to get one."""
    from open_duck_playground_amd import track
    from open_duck_playground_amd.model import Model
    hmap, joints = track.posture_head_map(types.SimpleNamespace(mj_model=model_a, head_joints=None))
    assert hmap == [5, 6, 7, 8] and len(joints) == 14
    assert [joints[u] for u in hmap] == ["neck_pitch", "head_pitch", "head_yaw", "head_roll"]
    biped = Model.from_xml(os.path.join(ROOT, "tests", "assets", "biped12_neck.xml"))
    hmap, joints = track.posture_head_map(types.SimpleNamespace(mj_model=biped, head_joints=[13, -1, -1, 12]))
    assert hmap == [13, -1, -1, 12] and len(joints) == biped.nu
    jn = [str(n) for n in biped.a["names_jnt"]]
    trn = np.asarray(biped.a["actuator_trnid"]).reshape(biped.nu, -1)[:, 0]
    assert joints == [jn[int(j)] for j in trn]
    with pytest.raises(ValueError, match="no head-joint map.*--env standing --head_joints"):
        track.posture_head_map(types.SimpleNamespace(mj_model=biped, head_joints=None))


def test_posture_accumulate_rejects_bad_tensors():
    """The tensor checks run before the library is touched, so a stand-in batch (no GPU) reaches them through the real method."""
    import torch
    from open_duck_playground_amd import engine
    n = 8
    stub = types.SimpleNamespace(nenv=n, device=0, model=types.SimpleNamespace(nu=14))
    G, T = engine.POSTURE_NACC, engine.TRACK_NACC
    bad = [
        (np.zeros((n, G), np.float32), "torch tensor"),
        (torch.zeros(n, G - 1), "shape"),
        (torch.zeros(n + 1, G), "shape"),
        (torch.zeros(n, G, dtype=torch.float64), "dtype"),
        (torch.zeros(G, n).t(), "contiguous"),
        (torch.zeros(n, G), "cuda:0"),            # a host tensor: the kernel writes device memory
    ]
    for t, what in bad:
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.posture_accumulate(stub, t, torch.zeros(n, T), 0.1)
        assert "posture_accumulate: acc" in str(ei.value)
