"""CPU checks of the imitation-fidelity report of `track --imitation_report`: the C-ABI export and the slot names, the report's reduction
of a hand-written imitation accumulator (sample-weighted means, an empty block, a reference joint that does not move, a foot without a
touchdown, the sign of the lag, per-cell rows with pushes), the two refusals made on the host before any batch exists, the command-line
flag and the tensor checks of `Batch.imitation_accumulate`."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = dict(SAMPLES=0, GATED=1, SPEED_ERR_SQ_SUM=2, REF_SPEED_SUM=3, JOINT_POS_SQ_SUM=4, JOINT_VEL_SQ_SUM=5)
PAIRS = dict(BOTH=6, ROBOT_ONLY=8, REF_ONLY=10, REF_TOUCHDOWNS=12, TOUCHDOWNS=14, LAG_SUM=16, LAG_ABS_SUM=18, PREV_CONTACT=20, PREV_REF=22, REF_AGE=24)
ARRAYS = dict(POS_ERR_SUM=32, POS_ERR_SQ=48, POS_ERR_PEAK=64, VEL_ERR_SQ=80, RANGE_MIN=96, RANGE_MAX=112, REF_RANGE_MIN=128, REF_RANGE_MAX=144)
NACC, STRIDE = 160, 16


def test_libodk_exports_the_imitation_accumulator_and_the_header_names_its_slots():
    from open_duck_playground_amd import engine, track
    engine.build_library()
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "odk_imitation_accumulate")
    assert "odk_imitation_accumulate" in engine.EXPORTED_SYMBOLS
    names = {k[5:]: v for k, v in engine.header_constants().items() if k.startswith("IMIT_")}
    assert names.pop("NACC") == NACC and names.pop("STRIDE") == STRIDE
    assert engine.IMIT_NACC == track.IMIT_NACC == NACC and engine.IMIT_STRIDE == STRIDE
    every = {**SCALARS, **PAIRS, **ARRAYS}
    assert names == every          # the header names these slots and no others
    for name, slot in every.items():
        assert getattr(engine, "IMIT_" + name) == slot, name
    # scalars, then pairs (left, right), then the 16-entry arrays: nothing overlaps and the arrays end the row
    assert sorted(SCALARS.values()) == list(range(6)) and sorted(PAIRS.values()) == list(range(6, 26, 2))
    assert max(PAIRS.values()) + 2 <= ARRAYS["POS_ERR_SUM"] and sorted(ARRAYS.values()) == list(range(32, NACC, STRIDE))


def _row(**kw):
    """one accumulator row: scalars by name, pairs by name as (left, right), arrays by name as {actuator: value}"""
    r = np.zeros(NACC, np.float32)
    for k, v in kw.items():
        if k in SCALARS:
            r[SCALARS[k]] = np.float32(v)
        elif k in PAIRS:
            r[PAIRS[k]:PAIRS[k] + 2] = np.float32(v)
        else:
            for u, x in v.items():
                r[ARRAYS[k] + u] = np.float32(x)
    return r


IMAP = [4, -1, 0]                     # actuator 0 against frame joint 4, actuator 1 not compared, actuator 2 against frame joint 0
JOINTS = ["hip", "neck", "knee"]


def _block():
    """Three envs.  Env 0: 30 samples; env 1: 10 samples (its first episode ended early); env 2: none.  Actuator 2's reference never moves.
    The left foot touches down 3 + 1 times, late by 2 + 2 + 1 and early by 3 (lags 2, 2, 1, -3); the right foot never touches down."""
    return np.stack([
        _row(SAMPLES=30, GATED=30, SPEED_ERR_SQ_SUM=1.5, REF_SPEED_SUM=3.0, JOINT_POS_SQ_SUM=6.0, JOINT_VEL_SQ_SUM=300.0,
             BOTH=(12, 10), ROBOT_ONLY=(3, 0), REF_ONLY=(6, 5), REF_TOUCHDOWNS=(3, 2), TOUCHDOWNS=(3, 0), LAG_SUM=(5, 0), LAG_ABS_SUM=(5, 0),
             PREV_CONTACT=(1, 0), PREV_REF=(1, 1), REF_AGE=(4, 7),
             POS_ERR_SUM={0: 3.0, 2: -6.0}, POS_ERR_SQ={0: 1.2, 2: 4.8}, POS_ERR_PEAK={0: 0.5, 2: 0.75}, VEL_ERR_SQ={0: 120.0, 2: 180.0},
             RANGE_MIN={0: -0.25, 2: 0.125}, RANGE_MAX={0: 0.5, 2: 0.25}, REF_RANGE_MIN={0: -0.5, 2: 0.375}, REF_RANGE_MAX={0: 0.25, 2: 0.375}),
        _row(SAMPLES=10, GATED=0, SPEED_ERR_SQ_SUM=0.1, REF_SPEED_SUM=1.0, JOINT_POS_SQ_SUM=2.0, JOINT_VEL_SQ_SUM=100.0,
             BOTH=(2, 5), ROBOT_ONLY=(1, 5), REF_ONLY=(0, 0), REF_TOUCHDOWNS=(1, 0), TOUCHDOWNS=(1, 0), LAG_SUM=(-3, 0), LAG_ABS_SUM=(3, 0),
             POS_ERR_SUM={0: 1.0, 2: -2.0}, POS_ERR_SQ={0: 0.4, 2: 1.6}, POS_ERR_PEAK={0: 0.625, 2: 0.5}, VEL_ERR_SQ={0: 40.0, 2: 60.0},
             RANGE_MIN={0: -0.5, 2: 0.0}, RANGE_MAX={0: 0.25, 2: 0.125}, REF_RANGE_MIN={0: -0.25, 2: 0.375}, REF_RANGE_MAX={0: 0.5, 2: 0.375}),
        _row(),
    ])


def test_imitation_report_reduction():
    """Two blocks of three envs: the one above, and one where nobody has a sample.  Every figure at its closed form."""
    from open_duck_playground_amd import track
    dt, period = 0.02, 27
    acc = np.concatenate([_block(), np.zeros((3, NACC), np.float32)])
    out = track.reduce_imitation(acc, [[0.1, 0, 0, 0, 0, 0, 0], [0, 0, 0.5, 0, 0, 0, 0]], 3, dt, IMAP, JOINTS, period)
    assert len(out) == 2 and json.loads(json.dumps(out)) == out
    ap = pytest.approx
    g = out[0]
    assert tuple(g) == track.IMITATION_KEYS
    # pooled over samples: the env with 30 samples weighs three times the one with 10, the env without any not at all
    assert g["samples"] == 40 and g["gated_share"] == ap(30 / 40) and g["period_steps"] == period
    assert g["speed_rms_error"] == ap(np.sqrt(1.6 / 40)) and g["reference_speed_mean"] == ap(4.0 / 40)
    assert g["joint_pos_term"] == ap(15.0 * 8.0 / 40) and g["joint_vel_term"] == ap(1e-3 * 400.0 / 40)
    # one entry per compared actuator, in actuator order; the uncompared one is absent
    assert [j["joint"] for j in g["joints"]] == ["hip", "knee"] and [j["frame_joint"] for j in g["joints"]] == [4, 0]
    hip, knee = g["joints"]
    assert tuple(hip) == tuple(knee) == track.IMITATION_JOINT_KEYS
    assert hip["bias"] == ap(4.0 / 40) and knee["bias"] == ap(-8.0 / 40)
    assert hip["rms_error"] == ap(np.sqrt(1.6 / 40)) and knee["rms_error"] == ap(np.sqrt(6.4 / 40))
    assert hip["peak_error"] == 0.625 and knee["peak_error"] == 0.75                       # the block's maximum
    assert hip["vel_rms_error"] == ap(np.sqrt(160.0 / 40)) and knee["vel_rms_error"] == ap(np.sqrt(240.0 / 40))
    assert hip["range"] == [-0.5, 0.5] and hip["reference_range"] == [-0.5, 0.5] and hip["amplitude_ratio"] == 1.0
    # a reference joint that does not move has no amplitude to compare with; the env without a sample does not pull the range to 0
    assert knee["range"] == [0.0, 0.25] and knee["reference_range"] == [0.375, 0.375] and knee["amplitude_ratio"] is None
    left, right = g["feet"]
    assert tuple(left) == tuple(right) == track.IMITATION_FOOT_KEYS and (left["foot"], right["foot"]) == ("left", "right")
    assert left["contact_agreement"] == ap(1 - (4 + 6) / 40) and right["contact_agreement"] == ap(1 - (5 + 5) / 40)
    assert left["stance_share"] == ap(18 / 40) and left["reference_stance_share"] == ap(20 / 40)
    assert right["stance_share"] == ap(20 / 40) and right["reference_stance_share"] == ap(20 / 40)
    assert left["touchdowns"] == 4 and left["reference_touchdowns"] == 4 and right["touchdowns"] == 0 and right["reference_touchdowns"] == 2
    # the lag's sign survives the mean: (2 + 2 + 1 - 3) / 4 late, |lag| 2 on average
    assert left["touchdown_lag_steps"] == ap(0.5) and left["touchdown_lag_s"] == ap(0.5 * dt) and left["touchdown_lag_abs_steps"] == ap(2.0)
    assert right["touchdown_lag_steps"] is None and right["touchdown_lag_s"] is None and right["touchdown_lag_abs_steps"] is None
    assert g["contact_term"] == ap(left["contact_agreement"] + right["contact_agreement"])
    # a block that is early on average reports a negative lag
    (early,) = track.reduce_imitation(acc[1:2], [[0] * 7], 1, dt, IMAP, JOINTS, period)
    assert early["feet"][0]["touchdown_lag_steps"] == ap(-3.0) and early["feet"][0]["touchdown_lag_s"] == ap(-3.0 * dt)
    assert early["feet"][0]["touchdown_lag_abs_steps"] == ap(3.0) and early["gated_share"] == 0.0

    # the empty block: nothing to average, nothing divides by zero, no NaN
    e = out[1]
    assert tuple(e) == tuple(g) and e["samples"] == 0 and e["period_steps"] == period
    for key in ("gated_share", "joint_pos_term", "joint_vel_term", "contact_term", "speed_rms_error", "reference_speed_mean"):
        assert e[key] is None, key
    assert [j["joint"] for j in e["joints"]] == ["hip", "knee"]
    for j in e["joints"]:
        assert j["range"] == [None, None] and j["reference_range"] == [None, None]
        assert all(j[k] is None for k in ("bias", "rms_error", "peak_error", "vel_rms_error", "amplitude_ratio"))
    for f in e["feet"]:
        assert f["touchdowns"] == 0 and f["reference_touchdowns"] == 0
        assert all(f[k] is None for k in track.IMITATION_FOOT_KEYS if k not in ("foot", "touchdowns", "reference_touchdowns"))
    assert "NaN" not in json.dumps(out)


def test_imitation_report_per_cell_rows_with_pushes():
    """With pushes the accumulator's envs are (command, push) cells of E envs, command blocks outermost: the row pools its cells."""
    from open_duck_playground_amd import track
    blk = _block()
    acc = np.concatenate([blk[:1], blk[1:2], blk[2:3], blk[:1]])       # one command, two pushes, E = 2: cells (env 0, env 1) and (env 2, env 0)
    cells = track.reduce_imitation(acc, [dict(push=[0, 0]), dict(push=[1, 0])], 2, 0.02, IMAP, JOINTS, 27)
    (row,) = track.reduce_imitation(acc, [[0.1, 0, 0, 0, 0, 0, 0]], 4, 0.02, IMAP, JOINTS, 27)
    assert [c["samples"] for c in cells] == [40, 30] and row["samples"] == 70
    assert cells[1]["gated_share"] == 1.0 and row["gated_share"] == pytest.approx(60 / 70)
    assert cells[0]["feet"][0]["touchdown_lag_steps"] == pytest.approx(0.5) and cells[1]["feet"][0]["touchdown_lag_steps"] == pytest.approx(5 / 3)
    assert row["feet"][0]["touchdowns"] == 7 and row["feet"][0]["touchdown_lag_steps"] == pytest.approx(7 / 7)
    assert row["joints"][0]["bias"] == pytest.approx(7.0 / 70) and cells[1]["joints"][0]["range"] == [-0.25, 0.5]


def test_imitation_report_refused_on_the_host(monkeypatch):
    """Standing, and a robot that is not the duck without a reference motion: an error that says why, before any batch is made."""
    from open_duck_playground_amd import track
    monkeypatch.setattr(track, "make_env", lambda *a, **k: pytest.fail("a batch was made"))
    base = ["--checkpoint", "c.pt", "--command", "0.1", "0", "0", "--imitation_report"]
    parse = track.build_parser().parse_args
    with pytest.raises(SystemExit, match="--imitation_report: the standing env has no imitation reward.*--env joystick"):
        track.run(parse(base + ["--env", "standing"]))
    xml = os.path.join(ROOT, "tests", "assets", "biped12.xml")
    with pytest.raises(SystemExit, match="--imitation_report: a robot that is not the duck runs without the imitation reward.*--reference_motion"):
        track.run(parse(base + ["--xml", xml]))
    # what passes: the duck, and another robot that brings its reference motion
    assert track.imitation_refusal(parse(base)) is None
    assert track.imitation_refusal(parse(base + ["--xml", xml, "--reference_motion", "m.pkl"])) is None
    # an env that runs without the reward says so as well (what `run` asks once the env exists)
    with pytest.raises(ValueError, match="runs without the imitation reward"):
        track.imitation_joint_info(types.SimpleNamespace(imitation_joints=None))


def test_imitation_report_command_line_flag():
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt", "--command", "0", "0", "0"]
    assert track.build_parser().parse_args(base).imitation_report is False
    args = track.build_parser().parse_args(base + ["--imitation_report", "--gait", "--posture", "--push_grid", "magnitude=0:1.5:2,direction=0:90:2"])
    assert args.imitation_report is True and args.gait is True and args.posture is True and args.push_grid
    help_text = " ".join(track.build_parser().format_help().split())
    for word in ("--imitation_report", "reference gait", "touchdown lag", "--reference_motion"):
        assert word in help_text, word


def test_imitation_accumulate_rejects_bad_tensors():
    """The tensor checks run before the library is touched, so a stand-in batch (no GPU) reaches them through the real method."""
    import torch
    from open_duck_playground_amd import engine
    n = 8
    stub = types.SimpleNamespace(nenv=n, device=0, model=types.SimpleNamespace(nu=14))
    G, T = engine.IMIT_NACC, engine.TRACK_NACC
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
            engine.Batch.imitation_accumulate(stub, t, torch.zeros(n, T), 12)
        assert "imitation_accumulate: acc" in str(ei.value)
