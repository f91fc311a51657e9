"""Sensor faults for `track` (`--sensor`, `--sensor_grid`): the keys and their parsers, the per-env fault rows `odk_sensor_apply` reads
(include/odk.h "Sensor faults"), and a numpy restatement of that kernel with its bits.  Host code only: no GPU, no torch."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from .sweeps import parse_axis_grid, grid_rows, parse_key_values, cell_rows

from .engine import (SENSOR_NPRM, SENSOR_NSTATE, SENSOR_RING, SENSOR_SAMPLE, SENSOR_IMU_ROT, SENSOR_GYRO_SCALE, SENSOR_GYRO_BIAS, SENSOR_ACC_SCALE,
                     SENSOR_ACC_BIAS, SENSOR_IMU_DELAY, SENSOR_JOINT_DELAY, SENSOR_ENC_QUANT, SENSOR_CONTACT_MODE, SENSOR_ENC_OFFSET, SENSOR_HEAD,
                     SENSOR_RING_AT, SENSOR_S_IMU, SENSOR_S_JOINT_POS, SENSOR_S_JOINT_VEL, sensor_fault_rows, sensor_rotation)      # ODK_SENSOR_*

CONTACT_MODES = ("ok", "off", "on")      # a CONTACT_MODE slot's 0, 1, 2: pass through, stuck at 0, stuck at 1
BIAS_KEYS = ("gyro_bias_x", "gyro_bias_y", "gyro_bias_z", "acc_bias_x", "acc_bias_y", "acc_bias_z")      # rad/s, m/s^2
SCALE_KEYS = ("gyro_scale", "acc_scale")
ANGLE_KEYS = ("imu_roll", "imu_pitch", "imu_yaw")      # degrees
DELAY_KEYS = ("imu_delay", "joint_delay")      # whole control steps, 0 .. SENSOR_RING - 1
ENCODER_KEYS = ("encoder_offset", "encoder_quant")      # rad: the bound of the per-actuator zero error, the quantiser's step
CONTACT_KEYS = ("contact_left", "contact_right")
SENSOR_KEYS = BIAS_KEYS[:3] + SCALE_KEYS[:1] + BIAS_KEYS[3:] + SCALE_KEYS[1:] + ANGLE_KEYS + DELAY_KEYS + ENCODER_KEYS + CONTACT_KEYS


def nominal_sensor() -> Dict:
    """The sensors of the robot the env kernels describe: no bias, scales 1, no tilt, no delay, exact encoders, working foot switches."""
    s = {k: 0.0 for k in SENSOR_KEYS}
    s.update({k: 1.0 for k in SCALE_KEYS}, **{k: 0 for k in DELAY_KEYS}, **{k: CONTACT_MODES[0] for k in CONTACT_KEYS})
    return s


def sensor_order(axis: str, value) -> float:
    """Where `value` sits on its axis' line: the number itself, or for a contact axis the index of its mode (ok, off, on)."""
    return float(CONTACT_MODES.index(value)) if axis in CONTACT_KEYS else float(value)


def sensor_value(flag: str, name: str, value) -> object:
    """One axis value as a sensor setting holds it; ValueError with the reason for an unknown key, a contact mode that is not ok / off / on, a
    delay that is not a whole number within 0 .. SENSOR_RING - 1, a negative encoder figure and anything not finite."""
    if name not in SENSOR_KEYS:
        raise ValueError(f"{flag}: unknown key {name!r} (one of {', '.join(SENSOR_KEYS)})")
    if name in CONTACT_KEYS:
        mode = str(value).strip().lower()
        if mode not in CONTACT_MODES:
            raise ValueError(f"{flag}: {name}={value!r} is not one of {', '.join(CONTACT_MODES)}")
        return mode
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{flag}: {name}={value!r} is not a number")
    if not np.isfinite(v):
        raise ValueError(f"{flag}: {name}={value} is not finite")
    if name in DELAY_KEYS:
        if v != round(v):
            raise ValueError(f"{flag}: {name}={value} is not a whole number of control steps")
        if not 0 <= int(v) <= SENSOR_RING - 1:
            raise ValueError(f"{flag}: {name}={int(v)} is outside the sample ring: 0 .. {SENSOR_RING - 1} steps")
        return int(v)
    if name in ENCODER_KEYS and v < 0:
        raise ValueError(f"{flag}: {name}={value} is negative (a bound or a step in radians, 0 = off)")
    return v


def parse_sensor(spec: str) -> Dict:
    """`--sensor gyro_bias_y=0.2,imu_delay=2,contact_left=off` -> a sensor setting: `nominal_sensor()` with the named keys replaced.
    ValueError for an unknown key, a key given twice and a value `sensor_value` refuses."""
    return parse_key_values("--sensor", spec, nominal_sensor(), "key", sensor_value)


def parse_sensor_grid(spec: str) -> List[Dict]:
    """`imu_delay=0:7:8,gyro_bias_y=-0.3:0.3:5` -> the settings of the grid, with `--grid`'s conventions: each axis takes n values from a to b
    (numpy.linspace, ends included), settings in itertools.product order of the axes as written (the last axis varies fastest), keys not
    named stay nominal.  A delay axis must come out as whole numbers within the ring; a contact key is no grid axis (its values are names:
    give one `--sensor` per mode)."""
    no_axis = {k: f"{k} takes {' / '.join(CONTACT_MODES)}, not a range: give one --sensor {k}=MODE per mode" for k in CONTACT_KEYS}
    return grid_rows(parse_axis_grid("--sensor_grid", spec, SENSOR_KEYS, "key", sensor_value, refused=no_axis), nominal_sensor())


def sensors_from_args(args) -> List[Dict]:
    """The sensor settings the command line asks for (`--sensor` in order, then `--sensor_grid`'s), [] without a sensor flag.  SystemExit with
    the reason for a setting that cannot be parsed and for sensors next to `--push` / `--push_grid` or `--plant` / `--plant_grid` (a third cell
    axis) -- host work only, before any batch exists."""
    specs, grid = getattr(args, "sensor", None) or [], getattr(args, "sensor_grid", None)
    try:
        sensors = [parse_sensor(s) for s in specs] + (parse_sensor_grid(grid) if grid else [])
    except ValueError as err:
        raise SystemExit(str(err))
    if sensors and (getattr(args, "push", None) or getattr(args, "push_grid", None)):
        raise SystemExit("--sensor / --sensor_grid do not combine with --push / --push_grid: (command, push, sensor) would be a third cell axis; "
                         "run the push sweep once per sensor setting")
    if sensors and (getattr(args, "plant", None) or getattr(args, "plant_grid", None)):
        raise SystemExit("--sensor / --sensor_grid do not combine with --plant / --plant_grid: (command, plant, sensor) would be a third cell axis; "
                         "run the sensor sweep once per plant")
    return sensors


def fault_row(sensor: Dict, encoder_unit: Optional[np.ndarray] = None) -> np.ndarray:
    """One float32 fault row ([SENSOR_NPRM]) of a sensor setting.  `encoder_unit` ([16], each in -1 .. 1): the robot's draw, which
    `encoder_offset` scales into its actuators' zero errors; without it the offsets stay 0."""
    row = sensor_fault_rows(1)[0]
    row[SENSOR_IMU_ROT:SENSOR_IMU_ROT + 9] = sensor_rotation(sensor["imu_roll"], sensor["imu_pitch"], sensor["imu_yaw"]).reshape(9)
    row[SENSOR_GYRO_SCALE], row[SENSOR_ACC_SCALE] = sensor["gyro_scale"], sensor["acc_scale"]
    row[SENSOR_GYRO_BIAS:SENSOR_GYRO_BIAS + 3] = [sensor["gyro_bias_" + a] for a in "xyz"]
    row[SENSOR_ACC_BIAS:SENSOR_ACC_BIAS + 3] = [sensor["acc_bias_" + a] for a in "xyz"]
    row[SENSOR_IMU_DELAY], row[SENSOR_JOINT_DELAY] = sensor["imu_delay"], sensor["joint_delay"]
    row[SENSOR_ENC_QUANT] = sensor["encoder_quant"]
    row[SENSOR_CONTACT_MODE:SENSOR_CONTACT_MODE + 2] = [CONTACT_MODES.index(sensor[k]) for k in CONTACT_KEYS]
    if encoder_unit is not None and float(sensor["encoder_offset"]) > 0:
        row[SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16] = np.asarray(encoder_unit, np.float64) * float(sensor["encoder_offset"])
    return row


def sensor_blocks(ncommands: int, sensors: Sequence[Dict], envs_per_cell: int, seed: int = 0) -> np.ndarray:
    """float32 [n, SENSOR_NPRM] with n = ncommands * len(sensors) * envs_per_cell: cell (c, s) drives envs (c * len(sensors) + s) *
    envs_per_cell onwards -- `plant_blocks`' layout with sensor settings where the plants are.  Every env draws its 16 encoder units
    uniformly in -1 .. 1 from numpy.random.default_rng(seed), whether its cell has an `encoder_offset` or not (so a cell's robots do not
    depend on the other cells' settings): a cell with an offset is a population of miscalibrated robots."""
    E, S = int(envs_per_cell), len(sensors)
    n = int(ncommands) * S * E
    unit = np.random.default_rng(int(seed)).uniform(-1.0, 1.0, (n, 16))
    rows = cell_rows(np.stack([fault_row(s) for s in sensors]), ncommands, E)
    bound = cell_rows(np.asarray([float(s["encoder_offset"]) for s in sensors], np.float64), ncommands, E)[:, None]
    rows[:, SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16] = np.where(bound > 0, unit * bound, 0.0)      # (fault_row's product, for every env at once)
    return rows


def sensor_apply_reference(obs: np.ndarray, done: Optional[np.ndarray], fault: np.ndarray, state: np.ndarray, nu: int, joystick: bool = True) -> np.ndarray:
    """`odk_sensor_apply` restated in numpy float32, bit for bit: returns the output rows for `obs` ([n, nobs]) and advances `state`
    ([n, SENSOR_NSTATE] float32) in place.  `done`: [n] or None.  Every operation is one float32 operation of the kernel's, in its order, and
    every nominal stage is the same select (numpy.where moves bits: -0.0, NaN and inf come through).  A HEAD beyond int32 is not restated."""
    X, F, S = np.asarray(obs, np.float32), np.asarray(fault, np.float32), state
    assert S.dtype == np.float32 and S.shape == (X.shape[0], SENSOR_NSTATE) and F.shape == (X.shape[0], SENSOR_NPRM) and nu <= 16
    n, rows = X.shape[0], np.arange(X.shape[0])
    jv_at, contact_at = 13 + nu, 13 + (6 if joystick else 5) * nu
    Y = X.copy()                                  # the columns nothing touches
    ring = S[:, SENSOR_RING_AT:].reshape(n, SENSOR_RING, SENSOR_SAMPLE)      # a view: stores land in `state`
    n0 = S[:, SENSOR_HEAD].copy()
    with np.errstate(all="ignore"):
        refill = (n0 == 0) | ((np.asarray(done) != 0) if done is not None else False)
        cur = np.where(refill, 0, (n0.astype(np.int64) & 0xFFFFFFFF) % SENSOR_RING).astype(np.int64)
        top = np.float32(SENSOR_RING - 1)
        di = np.fmin(np.fmax(F[:, SENSOR_IMU_DELAY], np.float32(0)), top).astype(np.int64)
        dj = np.fmin(np.fmax(F[:, SENSOR_JOINT_DELAY], np.float32(0)), top).astype(np.int64)
        old_i = ring[rows, (cur + SENSOR_RING - di) & (SENSOR_RING - 1)]      # (copies: the delayed samples, loaded before the store)
        old_j = ring[rows, (cur + SENSOR_RING - dj) & (SENSOR_RING - 1)]
        raw_i, raw_p, raw_v = X[:, 0:6], np.zeros((n, 16), np.float32), np.zeros((n, 16), np.float32)
        raw_p[:, :nu], raw_v[:, :nu] = X[:, 13:13 + nu], X[:, jv_at:jv_at + nu]
        imu_now, joint_now = (refill | (di == 0))[:, None], (refill | (dj == 0))[:, None]
        vec = np.where(imu_now, raw_i, old_i[:, SENSOR_S_IMU:SENSOR_S_IMU + 6])
        p = np.where(joint_now, raw_p, old_j[:, SENSOR_S_JOINT_POS:SENSOR_S_JOINT_POS + 16])
        v = np.where(joint_now, raw_v, old_j[:, SENSOR_S_JOINT_VEL:SENSOR_S_JOINT_VEL + 16])
        for e in rows:                            # the store: every slot on a refill, else slot HEAD mod RING
            slots = slice(None) if refill[e] else slice(cur[e], cur[e] + 1)
            ring[e, slots, SENSOR_S_IMU:SENSOR_S_IMU + 6] = raw_i[e]
            ring[e, slots, SENSOR_S_JOINT_POS:SENSOR_S_JOINT_POS + 16] = raw_p[e]
            ring[e, slots, SENSOR_S_JOINT_VEL:SENSOR_S_JOINT_VEL + 16] = raw_v[e]
        S[:, SENSOR_HEAD] = np.where(refill, np.float32(1), n0 + np.float32(1))
        # the IMU: out = scale (R x) + bias, each stage behind its select
        R = F[:, SENSOR_IMU_ROT:SENSOR_IMU_ROT + 9].reshape(n, 3, 3)
        ident = np.all(R == np.eye(3, dtype=np.float32), axis=(1, 2))[:, None]
        for base, scale_at, bias_at in ((0, SENSOR_GYRO_SCALE, SENSOR_GYRO_BIAS), (3, SENSOR_ACC_SCALE, SENSOR_ACC_BIAS)):
            x = vec[:, base:base + 3]
            rot = (R[:, :, 0] * x[:, 0:1] + R[:, :, 1] * x[:, 1:2]) + R[:, :, 2] * x[:, 2:3]
            r = np.where(ident, x, rot)
            scale, bias = F[:, scale_at:scale_at + 1], F[:, bias_at:bias_at + 3]
            r = np.where(scale != 1, scale * r, r)
            r = np.where(bias != 0, r + bias, r)
            Y[:, base:base + 3] = r
        # the encoders: offset, then the quantiser; the velocities are only late
        off, q = F[:, SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16], F[:, SENSOR_ENC_QUANT:SENSOR_ENC_QUANT + 1]
        p = np.where(off != 0, p + off, p)
        p = np.where(q > 0, q * np.rint(p / q), p)
        Y[:, 13:13 + nu], Y[:, jv_at:jv_at + nu] = p[:, :nu], v[:, :nu]
        # the foot switches
        mode, c = F[:, SENSOR_CONTACT_MODE:SENSOR_CONTACT_MODE + 2], X[:, contact_at:contact_at + 2]
        Y[:, contact_at:contact_at + 2] = np.where(mode == 1, np.float32(0), np.where(mode == 2, np.float32(1), c))
    assert Y.dtype == np.float32
    return Y
