"""CPU checks of the gait and actuator-load report of `track --gait`: the C-ABI export and the slot names, the report's reduction of a
hand-written gait accumulator, the command-line switch, the torque limits taken from the compiled model and the tensor checks of
`Batch.gait_accumulate`."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = dict(SAMPLES=0, SPEED_SUM=1, ABS_POWER_SUM=2, CONTACT=3, DOUBLE=5, FLIGHT=6, TOUCHDOWNS=7, SWING_STEPS_SUM=9, SLIP_SUM=11, HEIGHT_SUM=13,
               HEIGHT_SQ_SUM=14, ROLLPITCH_RATE_SQ_SUM=15, ACTION_RATE_SUM=16, PREV_CONTACT=17, AIR_RUN=19)
ARRAYS = dict(TORQUE_SQ=32, TORQUE_PEAK=48, VEL_PEAK=64, SAT=80, ABS_POWER=96, RANGE_MIN=112, RANGE_MAX=128)


def test_libodk_exports_the_gait_accumulator_and_the_header_names_its_slots():
    from open_duck_playground_amd import engine, track
    engine.build_library()
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "odk_gait_accumulate")
    assert "odk_gait_accumulate" in engine.EXPORTED_SYMBOLS
    header = engine.header_constants()
    assert header["GAIT_NACC"] == 144 and header["GAIT_STRIDE"] == 16
    assert engine.GAIT_NACC == track.GAIT_NACC == 144 and engine.GAIT_STRIDE == 16
    for name, slot in {**SCALARS, **ARRAYS}.items():
        assert header["GAIT_" + name] == slot == getattr(engine, "GAIT_" + name), name
    # the arrays do not overlap the scalars or one another, and the last one ends the row
    assert max(SCALARS.values()) + 2 <= ARRAYS["TORQUE_SQ"] and sorted(ARRAYS.values()) == list(range(32, 144, 16))


def _row(nu, **kw):
    """one accumulator row: scalars by name (a pair for the per-foot slots), arrays by name as nu values"""
    r = np.zeros(144, np.float32)
    for k, v in kw.items():
        if k in SCALARS:
            v = np.atleast_1d(np.float32(v))
            r[SCALARS[k]:SCALARS[k] + len(v)] = v
        else:
            r[ARRAYS[k]:ARRAYS[k] + nu] = np.float32(v)
    return r


def test_gait_report_reduction(model_a):
    """Three blocks of two envs on the duck's model: block 0 walks (touchdowns on both feet) and holds one env without a sample, block 1 never
    touches down (left foot always, right foot never in contact), block 2 stands on the spot (zero distance).  Every field at its closed form."""
    from open_duck_playground_amd import track
    nu, dt = model_a.nu, 0.02
    assert nu == 14
    ones = np.ones(nu)
    u = np.arange(nu)
    acc = np.stack([
        # block 0: env 0 walked for 100 samples, env 1 ended its first episode at step 0 (a zeroed row)
        _row(nu, SAMPLES=100, SPEED_SUM=10.0, ABS_POWER_SUM=50.0, CONTACT=(60, 70), DOUBLE=35, FLIGHT=5, TOUCHDOWNS=(4, 5), SWING_STEPS_SUM=(36, 30),
             SLIP_SUM=(0.6, 1.4), HEIGHT_SUM=15.0, HEIGHT_SQ_SUM=2.5, ROLLPITCH_RATE_SQ_SUM=4.0, ACTION_RATE_SUM=2.0, PREV_CONTACT=(1, 0), AIR_RUN=(0, 3),
             TORQUE_SQ=100.0 * (u + 1), TORQUE_PEAK=0.1 * (u + 1), VEL_PEAK=u + 0.5, SAT=u, ABS_POWER=2.0 * u, RANGE_MIN=-0.1 * (u + 1), RANGE_MAX=0.2 * u),
        _row(nu),
        # block 1: two envs, the left foot always down, the right one never: no touchdown, no slip on the right
        _row(nu, SAMPLES=40, SPEED_SUM=4.0, ABS_POWER_SUM=8.0, CONTACT=(40, 0), FLIGHT=0, SLIP_SUM=(0.4, 0.0), HEIGHT_SUM=6.0, HEIGHT_SQ_SUM=0.9,
             PREV_CONTACT=(1, 0), AIR_RUN=(0, 40), TORQUE_SQ=ones, TORQUE_PEAK=2.0 * ones, VEL_PEAK=ones, ABS_POWER=ones, RANGE_MIN=-ones, RANGE_MAX=ones),
        _row(nu, SAMPLES=10, SPEED_SUM=1.0, ABS_POWER_SUM=2.0, CONTACT=(10, 0), SLIP_SUM=(0.1, 0.0), HEIGHT_SUM=1.5, HEIGHT_SQ_SUM=0.225,
             PREV_CONTACT=(1, 0), AIR_RUN=(0, 10), TORQUE_SQ=3.0 * ones, TORQUE_PEAK=ones, VEL_PEAK=3.0 * ones, ABS_POWER=ones, RANGE_MIN=-2.0 * ones,
             RANGE_MAX=0.5 * ones),
        # block 2: standing still: 0.4 m of planar speed sum * 0.02 s = 8 mm, under the centimetre
        _row(nu, SAMPLES=50, SPEED_SUM=0.25, ABS_POWER_SUM=5.0, CONTACT=(50, 50), DOUBLE=50, HEIGHT_SUM=7.5, HEIGHT_SQ_SUM=1.125, TORQUE_SQ=ones),
        _row(nu, SAMPLES=50, SPEED_SUM=0.15, ABS_POWER_SUM=5.0, CONTACT=(50, 50), DOUBLE=50, HEIGHT_SUM=7.5, HEIGHT_SQ_SUM=1.125, TORQUE_SQ=ones),
    ])
    cmds = [[0.1, 0, 0, 0, 0, 0, 0], [0.05, 0, 0, 0, 0, 0, 0], [0.0] * 7]
    out = track.reduce_gait(acc, cmds, 2, dt, model_a)
    assert len(out) == 3 and all(tuple(g) == track.GAIT_KEYS for g in out)
    assert json.loads(json.dumps(out)) == out
    names = [str(n) for n in model_a.a["names_actuator"]]
    weight = float(np.sum(model_a.a["body_mass"]) * np.linalg.norm(model_a.a["opt_gravity"]))
    assert weight == pytest.approx(track.nominal_weight(model_a)) and 15.0 < weight < 25.0       # the duck: about 2 kg under 9.81 m/s^2
    limit = track.torque_limits(model_a)
    ap = pytest.approx
    f = lambda x: np.float32(x).astype(np.float64)          # what the float32 row holds

    g = out[0]
    assert g["samples"] == 100 and g["duty_factor"] == ap([0.6, 0.7]) and g["double_support_fraction"] == ap(0.35) and g["flight_fraction"] == ap(0.05)
    assert g["step_frequency_hz"] == ap([4 / (100 * dt), 5 / (100 * dt)]) and g["mean_swing_time_s"] == ap([9 * dt, 6 * dt])
    assert g["foot_slip_mps"] == ap([f(0.6) / 60, f(1.4) / 70])
    assert g["root_height_mean"] == ap(0.15) and g["root_height_std"] == ap(np.sqrt(0.025 - 0.0225)) and g["roll_pitch_rate_rms"] == ap(0.2)
    assert g["action_rate_mean"] == ap(0.02) and g["mean_abs_power_w"] == ap(0.5) and g["cost_of_transport"] == ap(50.0 / (weight * 10.0))
    assert list(g["actuators"]) == names
    for k, nm in enumerate(names):
        a = g["actuators"][nm]
        assert tuple(a) == track.GAIT_ACTUATOR_KEYS
        assert a["torque_rms"] == ap(np.sqrt(k + 1.0)) and a["torque_peak"] == ap(f(0.1 * (k + 1))) and a["torque_limit"] == float(limit[k])
        assert a["saturation_fraction"] == ap(k / 100) and a["velocity_peak"] == ap(k + 0.5) and a["mean_abs_power_w"] == ap(2.0 * k / 100)
        assert a["range"] == ap([f(-0.1 * (k + 1)), f(0.2 * k)])       # the env without a sample does not pull the range to its zeros

    g = out[1]
    assert g["samples"] == 50 and g["duty_factor"] == ap([1.0, 0.0]) and g["double_support_fraction"] == 0.0 and g["flight_fraction"] == 0.0
    assert g["step_frequency_hz"] == [0.0, 0.0] and g["mean_swing_time_s"] == [None, None]
    assert g["foot_slip_mps"][0] == ap(f(0.4) / 50 + f(0.1) / 50) and g["foot_slip_mps"][1] is None
    assert g["root_height_mean"] == ap(0.15) and g["root_height_std"] == ap(0.0, abs=1e-4) and g["cost_of_transport"] == ap(10.0 / (weight * 5.0))
    a = g["actuators"][names[3]]
    assert a["torque_rms"] == ap(np.sqrt(4.0 / 50)) and a["torque_peak"] == 2.0 and a["velocity_peak"] == 3.0 and a["range"] == [-2.0, 1.0]
    assert a["mean_abs_power_w"] == ap(2.0 / 50) and a["saturation_fraction"] == 0.0

    g = out[2]
    assert g["samples"] == 100 and g["duty_factor"] == [1.0, 1.0] and g["double_support_fraction"] == 1.0
    assert g["cost_of_transport"] is None and g["mean_abs_power_w"] == ap(0.1)                  # 0.4 * 0.02 = 0.008 m < 0.01 m
    assert g["mean_swing_time_s"] == [None, None] and g["foot_slip_mps"] == [0.0, 0.0]
    # a block in which nobody has a sample: no range, zero means, nothing divides by zero
    empty = track.reduce_gait(np.zeros((2, 144), np.float32), cmds[:1], 2, dt, model_a)[0]
    assert empty["samples"] == 0 and empty["cost_of_transport"] is None and empty["foot_slip_mps"] == [None, None]
    assert empty["actuators"][names[0]]["range"] == [None, None] and empty["duty_factor"] == [0.0, 0.0]


def test_gait_command_line_switch():
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt", "--command", "0", "0", "0"]
    assert track.build_parser().parse_args(base).gait is False
    assert track.build_parser().parse_args(base + ["--gait"]).gait is True
    help_text = " ".join(track.build_parser().format_help().split())
    for word in ("cost_of_transport", "nominal total mass", "gravity", "under 1 cm"):
        assert word in help_text, word


def test_torque_limits_come_from_the_compiled_model(model_a):
    from open_duck_playground_amd import track
    from open_duck_playground_amd.model import Model
    duck = track.torque_limits(model_a)
    assert duck.dtype == np.float32 and duck.shape == (14,)
    np.testing.assert_array_equal(duck, np.float32(model_a.a["actuator_forcerange"][:, 1]))
    assert np.all(model_a.a["actuator_forcelimited"] != 0) and np.all(duck > 0)
    biped = Model.from_xml(os.path.join(ROOT, "tests", "assets", "biped12.xml"))
    lim = track.torque_limits(biped)
    assert lim.shape == (12,)
    np.testing.assert_array_equal(lim, np.where(biped.a["actuator_forcelimited"] != 0, biped.a["actuator_forcerange"][:, 1], 0).astype(np.float32))
    assert np.all(lim > 0)
    # an actuator without a force range: 0, whatever its (unused) range holds
    fl = np.array(biped.a["actuator_forcelimited"]).copy()
    fl[[2, 7]] = 0
    free = track.torque_limits(Model({**biped.a, "actuator_forcelimited": fl}))
    assert free[2] == 0.0 and free[7] == 0.0
    np.testing.assert_array_equal(np.delete(free, [2, 7]), np.delete(lim, [2, 7]))


def test_gait_accumulate_rejects_bad_tensors():
    """The tensor checks run before the library is touched, so a stand-in batch (no GPU) reaches them through the real method."""
    import torch
    from open_duck_playground_amd import engine
    n, nu = 8, 14
    stub = types.SimpleNamespace(nenv=n, device=0, model=types.SimpleNamespace(nu=nu))
    G, T = engine.GAIT_NACC, engine.TRACK_NACC
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
            engine.Batch.gait_accumulate(stub, t, torch.zeros(n, T))
        assert "gait_accumulate: acc" in str(ei.value)
    # the other two tensors go through the same check (the method reaches them only behind a good `acc`, which needs a device:
    # tests/test_gpu_gait.py does that)
    for t, cols, what in ((torch.zeros(n, T + 1), T, "shape"), (torch.zeros(n, T, dtype=torch.int32), T, "dtype"), (torch.zeros(n, T), T, "cuda:0"),
                          (torch.zeros(1, nu + 1), nu, "shape")):
        with pytest.raises(engine.OdkError, match=what):
            engine.check_accumulator("gait_accumulate: track_acc", t, n if cols == T else 1, cols, 0)
