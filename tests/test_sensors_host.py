"""CPU checks of the sensor-fault stage of `track --sensor` / `--sensor_grid`: the C-ABI export and the slot names, the parsers with every
refusal by its name, the per-env fault rows, the numpy restatement of `odk_sensor_apply` on its own (delays, the refill, the ring beyond
its length, the all-nominal identity with -0.0, NaN and inf) and `reduce_robustness` with per-axis nominals on hand-made cells."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_libodk_exports_the_launch_and_engine_mirrors_every_slot():
    from open_duck_playground_amd import engine
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(lib, "odk_sensor_apply") and "odk_sensor_apply" in engine.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    assert re.search(r"\bint odk_sensor_apply\(const odk_batch\* b, const float\* obs_dev", text)
    names = {k[7:]: v for k, v in engine.header_constants().items() if k.startswith("SENSOR_")}
    assert "#define ODK_SENSOR_NSTATE (16 + ODK_SENSOR_RING * ODK_SENSOR_SAMPLE)" in text
    assert names["NSTATE"] == 16 + names["RING"] * names["SAMPLE"]
    assert set(names) == set(re.findall(r"\bODK_SENSOR_([A-Z_]+)\b", text)), "a name the header mentions has no value here"
    assert len(names) == 19
    for name, v in names.items():
        assert getattr(engine, "SENSOR_" + name) == v, name
    assert sorted(n for n in vars(engine) if n.startswith("SENSOR_")) == sorted("SENSOR_" + n for n in names)
    # the fault row's slots do not overlap and the row holds them; a ring of 8 is 140 ms at 50 Hz
    widths = dict(IMU_ROT=9, GYRO_SCALE=1, GYRO_BIAS=3, ACC_SCALE=1, ACC_BIAS=3, IMU_DELAY=1, JOINT_DELAY=1, ENC_QUANT=1, CONTACT_MODE=2, ENC_OFFSET=16)
    used = sorted(names[k] + i for k, w in widths.items() for i in range(w))
    assert len(set(used)) == len(used) and used[-1] == names["NPRM"] - 1 and names["RING"] == 8
    assert names["S_JOINT_VEL"] + 16 == names["SAMPLE"] and names["S_IMU"] + 6 <= names["S_JOINT_POS"] and names["S_JOINT_POS"] + 16 == names["S_JOINT_VEL"]
    rows = engine.Batch.sensor_fault_rows(3)
    assert rows.dtype == np.float32 and rows.shape == (3, names["NPRM"])
    want = np.zeros(names["NPRM"], np.float32)
    want[[0, 4, 8, names["GYRO_SCALE"], names["ACC_SCALE"]]] = 1.0
    assert all(np.array_equal(bits(r), bits(want)) for r in rows)


def test_the_rotation_is_a_pure_host_function():
    from open_duck_playground_amd import engine
    assert np.array_equal(engine.sensor_rotation(0, 0, 0), np.eye(3, dtype=np.float32))
    r = engine.sensor_rotation(0, 0, 90)      # the sensor's x axis points along the base's y: a base-frame y vector reads as sensor x
    assert r.dtype == np.float32 and np.allclose(r @ np.float32([0, 1, 0]), [1, 0, 0], atol=1e-7)
    r = engine.sensor_rotation(10, 0, 0)      # rolled 10 degrees: gravity's reaction (0, 0, 9.81) gains a y component of +9.81 sin(10)
    assert np.allclose(r @ np.float32([0, 0, 9.81]), [0, 9.81 * np.sin(np.deg2rad(10)), 9.81 * np.cos(np.deg2rad(10))], atol=1e-5)
    r = engine.sensor_rotation(7, -11, 23).astype(np.float64)
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-6) and np.isclose(np.linalg.det(r), 1.0, atol=1e-6)


def test_the_parsers():
    from open_duck_playground_amd import sensors, track
    s = sensors.parse_sensor("gyro_bias_y=0.2, imu_delay=2,contact_left=off")
    assert tuple(s) == sensors.SENSOR_KEYS and track.sensors_from_args is sensors.sensors_from_args
    want = sensors.nominal_sensor()
    want.update(gyro_bias_y=0.2, imu_delay=2, contact_left="off")
    assert s == want and isinstance(s["imu_delay"], int)
    assert sensors.nominal_sensor()["gyro_scale"] == 1.0 and sensors.nominal_sensor()["contact_right"] == "ok"
    grid = sensors.parse_sensor_grid("imu_delay=0:2:3,gyro_bias_y=-0.2:0.2:2")
    assert [(g["imu_delay"], g["gyro_bias_y"]) for g in grid] == [(0, -0.2), (0, 0.2), (1, -0.2), (1, 0.2), (2, -0.2), (2, 0.2)]      # the product, last axis fastest
    assert all(g["acc_scale"] == 1.0 and g["contact_left"] == "ok" for g in grid)
    assert [g["joint_delay"] for g in sensors.parse_sensor_grid("joint_delay=0:7:8")] == list(range(8))
    for spec, message in (("gyro_bias_w=1", "unknown key 'gyro_bias_w'"), ("imu_delay=8", "imu_delay=8 is outside the sample ring: 0 .. 7"),
                          ("joint_delay=-1", "joint_delay=-1 is outside the sample ring"), ("imu_delay=1.5", "not a whole number of control steps"),
                          ("contact_left=stuck", "contact_left='stuck' is not one of ok, off, on"), ("acc_scale=nan", "acc_scale=nan is not finite"),
                          ("encoder_quant=-0.1", "encoder_quant=-0.1 is negative"), ("gyro_scale", "'gyro_scale' is not KEY=VALUE"),
                          ("imu_yaw=1,imu_yaw=2", "key 'imu_yaw' given twice"), ("", "no key given"), ("acc_bias_x=fast", "is not a number")):
        with pytest.raises(ValueError, match=re.escape(message)):
            sensors.parse_sensor(spec)
    for spec, message in (("temperature=0:1:2", "unknown key 'temperature'"), ("imu_delay=0:8:9", "imu_delay=8 is outside the sample ring"),
                          ("imu_delay=0:1:3", "not a whole number"), ("contact_left=0:1:2", "contact_left takes ok / off / on, not a range"),
                          ("gyro_scale=1:2", "is not gyro_scale=start:stop:count"), ("gyro_scale=1:2:0", "needs a count >= 1")):
        with pytest.raises(ValueError, match=re.escape(message)):
            sensors.parse_sensor_grid(spec)


REFUSALS = [
    (["--sensor", "gyro_bias_q=1"], "--sensor: unknown key 'gyro_bias_q'"),
    (["--sensor_grid", "imu_lag=0:1:2"], "--sensor_grid: unknown key 'imu_lag'"),
    (["--sensor", "imu_delay=8"], "--sensor: imu_delay=8 is outside the sample ring"),
    (["--sensor_grid", "joint_delay=0:9:10"], "--sensor_grid: joint_delay=8 is outside the sample ring"),
    (["--sensor", "gyro_bias_y=0.2", "--push", "1", "0"], "--sensor / --sensor_grid do not combine with --push / --push_grid.*third cell axis"),
    (["--sensor_grid", "imu_delay=0:2:3", "--push_grid", "magnitude=0:1:2"], "--sensor / --sensor_grid do not combine with --push / --push_grid"),
    (["--sensor", "gyro_bias_y=0.2", "--plant", "kp=0.6"], "--sensor / --sensor_grid do not combine with --plant / --plant_grid.*third cell axis"),
    (["--sensor_grid", "imu_delay=0:2:3", "--plant_grid", "kp=0.5:1:2"], "--sensor / --sensor_grid do not combine with --plant / --plant_grid"),
]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_come_before_any_batch_work(flags, message):
    """Each as `run` raises it: SystemExit before any batch is made (no GPU here, so getting that far would be another error)."""
    from open_duck_playground_amd import track
    args = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0", "--episode_length", "100"] + flags)
    with pytest.raises(SystemExit, match=message):
        track.sensors_from_args(args)
    with pytest.raises(SystemExit, match=message):
        track.run(args)
    plain = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0"])
    assert track.sensors_from_args(plain) == [] and plain.sensor is None and plain.sensor_grid is None


def test_fault_rows_of_cells():
    from open_duck_playground_amd import engine, sensors
    cells = [sensors.nominal_sensor(), sensors.parse_sensor("acc_bias_x=1.3,imu_roll=5,joint_delay=3,contact_right=on,encoder_quant=0.01"),
             sensors.parse_sensor("encoder_offset=0.05,gyro_scale=1.1")]
    rows = sensors.sensor_blocks(2, cells, 4, seed=7)
    assert rows.dtype == np.float32 and rows.shape == (2 * 3 * 4, engine.SENSOR_NPRM)
    nominal = engine.sensor_fault_rows(1)[0]
    for c in range(2):
        blk = rows[c * 12:(c + 1) * 12]
        assert all(np.array_equal(bits(r), bits(nominal)) for r in blk[0:4])      # bit for bit nominal: no -0.0 from a zero bound
        for r in blk[4:8]:
            assert r[engine.SENSOR_ACC_BIAS] == np.float32(1.3) and r[engine.SENSOR_JOINT_DELAY] == 3 and r[engine.SENSOR_IMU_DELAY] == 0
            assert list(r[engine.SENSOR_CONTACT_MODE:engine.SENSOR_CONTACT_MODE + 2]) == [0, 2] and r[engine.SENSOR_ENC_QUANT] == np.float32(0.01)
            assert np.array_equal(r[:9].reshape(3, 3), engine.sensor_rotation(5, 0, 0)) and not r[engine.SENSOR_ENC_OFFSET:].any()
        off = blk[8:12, engine.SENSOR_ENC_OFFSET:engine.SENSOR_ENC_OFFSET + 16]
        assert (np.abs(off) <= 0.05).all() and len(np.unique(off)) == off.size and np.abs(off).max() > 0.04      # every robot its own draw
        assert (blk[8:12, engine.SENSOR_GYRO_SCALE] == np.float32(1.1)).all()
    unit = np.random.default_rng(7).uniform(-1.0, 1.0, (24, 16))
    np.testing.assert_array_equal(rows[8, engine.SENSOR_ENC_OFFSET:], (unit[8] * 0.05).astype(np.float32))
    np.testing.assert_array_equal(rows[8], sensors.fault_row(cells[2], unit[8]))
    assert not np.array_equal(rows, sensors.sensor_blocks(2, cells, 4, seed=8))


NU, NOBS = 14, 101


def _obs(rng, n, nobs=NOBS):
    return rng.standard_normal((n, nobs)).astype(np.float32)


def _run(sensors, X, fault, done=None, nu=NU, joystick=True):
    state = np.zeros((X[0].shape[0], sensors.SENSOR_NSTATE), np.float32)
    return [sensors.sensor_apply_reference(x, None if done is None else done[t], fault, state, nu, joystick) for t, x in enumerate(X)], state


def test_restatement_delay_d_is_the_raw_sample_of_d_calls_ago_and_the_ring_wraps():
    from open_duck_playground_amd import engine, sensors
    rng = np.random.default_rng(0)
    n, T = 8, 21                                         # env d has delay d, 0 .. 7; 21 calls go round the ring of 8 more than twice
    X = [_obs(rng, n) for _ in range(T)]
    for key, cols in ((engine.SENSOR_IMU_DELAY, np.r_[0:6]), (engine.SENSOR_JOINT_DELAY, np.r_[13:13 + 2 * NU])):
        fault = engine.sensor_fault_rows(n)
        fault[:, key] = np.arange(n)
        Y, state = _run(sensors, X, fault)
        rest = np.setdiff1d(np.arange(NOBS), cols)
        for t in range(T):
            for d in range(n):
                src = X[max(t - d, 0)]                   # before d calls have passed: the first sample (the refill put it in every slot)
                assert np.array_equal(bits(Y[t][d, cols]), bits(src[d, cols])), (t, d)
                assert np.array_equal(bits(Y[t][d, rest]), bits(X[t][d, rest])), (t, d)
        assert (state[:, engine.SENSOR_HEAD] == T).all()
        ring = state[:, engine.SENSOR_RING_AT:].reshape(n, engine.SENSOR_RING, engine.SENSOR_SAMPLE)
        for k in range(T - 8, T):                        # the ring holds the last 8 raw samples, sample k in slot k mod 8, whatever the fault row
            assert np.array_equal(ring[:, k % 8, 0:6], X[k][:, 0:6]) and np.array_equal(ring[:, k % 8, 16:16 + NU], X[k][:, 13:13 + NU])
            assert np.array_equal(ring[:, k % 8, 32:32 + NU], X[k][:, 13 + NU:13 + 2 * NU])
        assert not ring[:, :, 6:16].any() and not ring[:, :, 16 + NU:32].any() and not ring[:, :, 32 + NU:].any() and not state[:, 1:16].any()
    # a delay beyond the ring is clamped to 7, a negative one and NaN to 0, a fraction is dropped
    fault = engine.sensor_fault_rows(5)
    fault[:, engine.SENSOR_IMU_DELAY] = [9.0, -2.0, np.nan, 2.75, np.inf]
    Y, _ = _run(sensors, [x[:5] for x in X], fault)
    for e, d in enumerate((7, 0, 0, 2, 7)):
        assert np.array_equal(Y[12][e, 0:6], X[12 - d][e, 0:6]), e


def test_restatement_refills_on_done():
    from open_duck_playground_amd import engine, sensors
    rng = np.random.default_rng(1)
    n, T = 3, 12
    X = [_obs(rng, n) for _ in range(T)]
    done = np.zeros((T, n), np.float32)
    done[0, 0] = done[5, 0] = done[6, 0] = 1.0           # env 0: at call 0 and on two consecutive calls; env 1: once; env 2: never
    done[9, 1] = 1.0
    fault = engine.sensor_fault_rows(n)
    fault[:, engine.SENSOR_IMU_DELAY] = fault[:, engine.SENSOR_JOINT_DELAY] = 3
    Y, state = _run(sensors, X, fault, done)
    for e in range(n):
        start = 0
        for t in range(T):
            if done[t, e]:
                start = t                                # the observation of a done step is the new episode's first
            src = X[max(t - 3, start)]
            assert np.array_equal(Y[t][e, 0:6], src[e, 0:6]) and np.array_equal(Y[t][e, 13:13 + 2 * NU], src[e, 13:13 + 2 * NU]), (e, t)
        assert state[e, engine.SENSOR_HEAD] == T - start


def test_restatement_all_nominal_is_the_identity_on_every_bit_pattern():
    from open_duck_playground_amd import engine, sensors
    rng = np.random.default_rng(2)
    specials = np.array([-0.0, np.nan, np.inf, -np.inf, 0.0], np.float32)
    for nu, joystick, nobs in ((14, True, 101), (14, False, 85), (16, True, 113), (15, True, 107)):
        X = [_obs(rng, 6, nobs) for _ in range(10)]
        for x in X:
            x[rng.integers(0, 6, 60), rng.integers(0, nobs, 60)] = specials[rng.integers(0, 5, 60)]
            x[0, :] = np.float32(-0.0)
            x[1, :] = np.frombuffer(np.uint32(0xFFC12345).tobytes(), np.float32)[0]      # a NaN with a payload and a sign
        done = (rng.random((10, 6)) < 0.3).astype(np.float32)
        Y, _ = _run(sensors, X, engine.sensor_fault_rows(6), done, nu, joystick)
        for x, y in zip(X, Y):
            assert np.array_equal(bits(x), bits(y))


def test_restatement_each_stage_and_its_select():
    from open_duck_playground_amd import engine, sensors
    rng = np.random.default_rng(3)
    x = _obs(rng, 4)
    x[0, 0:6] = [-0.0, np.inf, 1.0, 2.0, -0.0, 3.0]
    f = engine.sensor_fault_rows(4)
    f[:, engine.SENSOR_GYRO_BIAS + 1] = 0.25
    f[:, engine.SENSOR_ACC_SCALE] = 2.0
    f[:, engine.SENSOR_ENC_OFFSET + 2] = 0.5
    f[:, engine.SENSOR_ENC_QUANT] = 0.125
    f[:, engine.SENSOR_CONTACT_MODE] = 1.0
    f[:, engine.SENSOR_CONTACT_MODE + 1] = 2.0
    y = sensors.sensor_apply_reference(x, None, f, np.zeros((4, engine.SENSOR_NSTATE), np.float32), NU)
    assert np.array_equal(bits(y[:, [0, 2]]), bits(x[:, [0, 2]])) and np.array_equal(y[:, 1], x[:, 1] + np.float32(0.25))      # only y is biased: x keeps its -0.0
    assert np.array_equal(bits(y[:, 3:6]), bits(np.float32(2.0) * x[:, 3:6]))
    p = x[:, 13:13 + NU].copy()
    p[:, 2] += np.float32(0.5)
    assert np.array_equal(y[:, 13:13 + NU], np.float32(0.125) * np.rint(p / np.float32(0.125)))
    assert np.array_equal(bits(y[:, 13 + NU:13 + 2 * NU]), bits(x[:, 13 + NU:13 + 2 * NU]))
    assert (y[:, 13 + 6 * NU] == 0).all() and (y[:, 13 + 6 * NU + 1] == 1).all()
    rest = np.r_[6:13, 13 + 2 * NU:13 + 6 * NU, 13 + 6 * NU + 2:NOBS]
    assert np.array_equal(bits(y[:, rest]), bits(x[:, rest]))
    # Standing: the contacts sit one block of nu earlier (its row has no motor targets)
    ys = sensors.sensor_apply_reference(x[:, :85], None, f, np.zeros((4, engine.SENSOR_NSTATE), np.float32), NU, joystick=False)
    assert (ys[:, 13 + 5 * NU] == 0).all() and (ys[:, 13 + 5 * NU + 1] == 1).all() and np.array_equal(bits(ys[:, 13 + 5 * NU + 2:]), bits(x[:, 13 + 5 * NU + 2:85]))
    # a rotation: R x summed left to right in float32, then scale, then bias
    f = engine.sensor_fault_rows(4)
    R = engine.sensor_rotation(3, -4, 5)
    f[:, :9] = R.reshape(9)
    y = sensors.sensor_apply_reference(x[1:], None, f[1:], np.zeros((3, engine.SENSOR_NSTATE), np.float32), NU)
    for e in range(3):
        g = x[1 + e, 0:3]
        want = [np.float32(np.float32(R[i, 0] * g[0]) + np.float32(R[i, 1] * g[1])) + np.float32(R[i, 2] * g[2]) for i in range(3)]
        assert np.array_equal(y[e, 0:3], np.float32(want))


def _cell(sensor, fall_rate):
    return dict(sensor=sensor, fall_rate=fall_rate, rms_error_vx=0.1, rms_error_vy=0.2, rms_error_wz=0.3, mean_episode_reward=1.0 - fall_rate)


def test_reduce_robustness_with_per_axis_nominals():
    from open_duck_playground_amd import sensors, track
    N = sensors.nominal_sensor
    cells = []
    for d, rate_at_nominal_bias, rate_biased in ((0, 0.0, 0.5), (1, 0.02, 0.6), (2, 0.04, 0.7), (3, 0.30, 0.8), (4, 0.01, 0.9)):
        for b, rate in ((-0.2, rate_biased), (0.0, rate_at_nominal_bias), (0.2, 0.05)):
            cells.append(_cell(dict(N(), imu_delay=d, gyro_bias_y=b), rate))
    out = track.reduce_robustness(cells, 0.05, key="sensor", nominals=N(), order=sensors.sensor_order)
    assert set(out) == {"robust_fall_rate", "gyro_bias_y", "imu_delay", "survived_range"} and out["robust_fall_rate"] == 0.05
    # the delay line runs at bias 0 (its nominal, not 1), the bias line at delay 0
    assert [p["value"] for p in out["imu_delay"]] == [0, 1, 2, 3, 4] and [p["fall_rate"] for p in out["imu_delay"]] == [0.0, 0.02, 0.04, 0.30, 0.01]
    assert [p["value"] for p in out["gyro_bias_y"]] == [-0.2, 0.0, 0.2] and [p["fall_rate"] for p in out["gyro_bias_y"]] == [0.5, 0.0, 0.05]
    assert all(tuple(p) == track.ROBUSTNESS_POINT_KEYS for p in out["imu_delay"] + out["gyro_bias_y"])
    # around 0: delays 0..2 (3 fails, whatever 4 does); the bias run starts at 0 and grows to +0.2 only
    assert out["survived_range"] == {"gyro_bias_y": [0.0, 0.2], "imu_delay": [0, 2]}
    # a scale's nominal is 1, and a grid that misses it starts from the nearest value (the smaller of two equally near)
    cells = [_cell(dict(N(), acc_scale=s), r) for s, r in ((0.8, 0.2), (0.9, 0.0), (1.1, 0.0), (1.2, 0.01), (1.3, 0.5))]
    out = track.reduce_robustness(cells, 0.05, key="sensor", nominals=N(), order=sensors.sensor_order)
    assert out["survived_range"] == {"acc_scale": [0.9, 1.2]}
    cells[1]["fall_rate"] = 0.5
    assert track.reduce_robustness(cells, 0.05, key="sensor", nominals=N(), order=sensors.sensor_order)["survived_range"] == {"acc_scale": None}
    # a foot switch: names on a line ok, off, on, nominal ok
    cells = [_cell(dict(N(), contact_left=m), r) for m, r in (("on", 0.9), ("ok", 0.0), ("off", 0.03))]
    out = track.reduce_robustness(cells, 0.05, key="sensor", nominals=N(), order=sensors.sensor_order)
    assert [p["value"] for p in out["contact_left"]] == ["ok", "off", "on"] and out["survived_range"] == {"contact_left": ["ok", "off"]}
    # the plants' reduction is what it was: scale axes around 1, the delay line from its smallest fixed delay
    plant = lambda kp, delay, r: dict(_cell(None, r), plant=dict(track.nominal_plant(), kp=kp, delay=delay))
    cells = [plant(0.5, 0, 0.4), plant(1.0, 0, 0.0), plant(0.5, 1, 0.6), plant(1.0, 1, 0.02)]
    out = track.reduce_robustness(cells, 0.05)
    assert out["survived_range"] == {"kp": [1.0, 1.0], "delay": [0, 1]} and [p["value"] for p in out["kp"]] == [0.5, 1.0]
