"""Training under sensor and actuation faults that are redrawn per episode (`runner --train_sensor` / `--train_actuation`): the flags'
parser, the table of ranges `odk_fault_resample` reads (include/odk.h "Fault resampling"), a numpy restatement of that kernel with its
bits, and `FaultStage`, which a rollout runs between the env and the policy.  The keys, their validators and their units are `track`'s
(sensors.py, actuation.py): what `track --sensor_grid` / `--actuation_grid` measures is what these flags train under.  torch is imported
only where a stage is built."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import actuation, sensors
from .engine import (SENSOR_NPRM, SENSOR_NSTATE, ACT_NPRM, ACT_NSTATE, FAULT_NSLOT, FAULT_NSTATE, FAULT_HEAD, FAULT_EPISODE, FAULT_FIXED,
                     FAULT_UNIFORM, FAULT_WHOLE, SENSOR_GYRO_SCALE, SENSOR_GYRO_BIAS, SENSOR_ACC_SCALE, SENSOR_ACC_BIAS, SENSOR_IMU_DELAY,
                     SENSOR_JOINT_DELAY, SENSOR_ENC_QUANT, SENSOR_ENC_OFFSET, ACT_GAIN, ACT_NOISE, ACT_LIMIT, ACT_ALPHA, ACT_QUANT, ACT_DROP_P,
                     ACT_DROP_LEN, ACT_SEED, ACT_OFFSET)      # ODK_FAULT_*, ODK_SENSOR_*, ODK_ACT_*

SENSOR_FLAG, ACTUATION_FLAG = "--train_sensor", "--train_actuation"
STREAM0 = 32      # slot s draws from stream STREAM0 + s of the action stage's hash (its own streams are 0 .. 16)

# the keys that take no range, with the reason
_SENSOR_FIXED_ONLY = {**{k: "the mounting rotation is built on the host (no sin or cos runs on the device)" for k in sensors.ANGLE_KEYS},
                      **{k: f"it takes {' / '.join(sensors.CONTACT_MODES)}" for k in sensors.CONTACT_KEYS},
                      "encoder_offset": "X is already a bound: every actuator's zero error is redrawn in +-X per episode"}
_ACTUATION_FIXED_ONLY = {"freeze": "it takes an actuator's name", "freeze_at": "it belongs to freeze's one actuator",
                         "offset": "X is already a bound: every actuator's horn error is redrawn in +-X per episode"}
# a ranged key's slot of its row; the per-actuator bounds and cutoff are built apart
_SENSOR_SLOT = {**{f"gyro_bias_{a}": SENSOR_GYRO_BIAS + i for i, a in enumerate("xyz")}, "gyro_scale": SENSOR_GYRO_SCALE,
                **{f"acc_bias_{a}": SENSOR_ACC_BIAS + i for i, a in enumerate("xyz")}, "acc_scale": SENSOR_ACC_SCALE,
                "imu_delay": SENSOR_IMU_DELAY, "joint_delay": SENSOR_JOINT_DELAY, "encoder_quant": SENSOR_ENC_QUANT}
_ACTUATION_SLOT = {"gain": ACT_GAIN, "noise": ACT_NOISE, "limit": ACT_LIMIT, "cutoff": ACT_ALPHA, "quant": ACT_QUANT, "drop": ACT_DROP_P,
                   "drop_len": ACT_DROP_LEN}
_WHOLE_KEYS = sensors.DELAY_KEYS + ("drop_len",)


def _parse(flag: str, items: Optional[Sequence[str]], nominal: Dict, value, fixed_only: Dict[str, str]) -> Dict:
    """`nominal` with the keys of every `KEY=V` / `KEY=LO:HI` part of every item replaced: a number (a name) as `value(flag, key, text)`
    holds it, or a (lo, hi) tuple of two such.  ValueError, naming `flag` and the key, for what `value` refuses, a key given twice (in one
    item or two), a part without `=`, a range for a key of `fixed_only`, a range that is not lo:hi with lo <= hi, and no key at all."""
    out, seen = dict(nominal), []
    for item in items or ():
        for part in str(item).split(","):
            part = part.strip()
            if not part:
                continue
            name, eq, text = part.partition("=")
            name, text = name.strip(), text.strip()
            if not eq:
                raise ValueError(f"{flag}: {part!r} is not KEY=VALUE or KEY=LO:HI")
            if name in seen:
                raise ValueError(f"{flag}: key {name!r} given twice")
            if ":" not in text:
                out[name] = value(flag, name, text)      # (an unknown key is refused here)
            else:
                value(flag, name, nominal.get(name, 0))      # the unknown key first, by its own message
                if name in fixed_only:
                    raise ValueError(f"{flag}: {name}={text} is a range, and {name} takes one value: {fixed_only[name]}")
                ends = text.split(":")
                if len(ends) != 2 or not all(e.strip() for e in ends):
                    raise ValueError(f"{flag}: {name}={text} is not {name}=LO:HI")
                lo, hi = (value(flag, name, e.strip()) for e in ends)
                if not lo <= hi:
                    raise ValueError(f"{flag}: {name}={text} has LO above HI")
                out[name] = (lo, hi)
            seen.append(name)
    if not seen:
        raise ValueError(f"{flag}: no key given")
    return out


def parse_train_sensor(items: Optional[Sequence[str]]) -> Dict:
    """`--train_sensor imu_delay=0:3,acc_bias_x=1.3` (repeatable) -> a sensor setting of sensors.py whose ranged keys hold (lo, hi): redrawn
    per episode, uniformly (the two delays: the whole steps lo .. hi).  The IMU mounting angles, the contact modes and `encoder_offset`
    (a bound already) take one value only."""
    return _parse(SENSOR_FLAG, items, sensors.nominal_sensor(), sensors.sensor_value, _SENSOR_FIXED_ONLY)


def parse_train_actuation(items: Optional[Sequence[str]]) -> Dict:
    """`--train_actuation cutoff=15:40,drop=0:0.05` (repeatable) -> an actuation setting of actuation.py whose ranged keys hold (lo, hi).
    `freeze`, `freeze_at` and `offset` (a bound already) take one value only; a `cutoff` range that holds 0 (the filter off) is refused:
    the filter coefficient has no value between "off" and the lowest cutoff's."""
    out = _parse(ACTUATION_FLAG, items, actuation.nominal_actuation(), actuation.actuation_value, _ACTUATION_FIXED_ONLY)
    cutoff = out["cutoff"]
    if isinstance(cutoff, tuple) and not cutoff[0] > 0:
        raise ValueError(f"{ACTUATION_FLAG}: cutoff={cutoff[0]:g}:{cutoff[1]:g} holds 0, which is the filter off: give a range of cutoffs above 0")
    return out


def fault_spec(sensor: Optional[Dict] = None, actuation_setting: Optional[Dict] = None) -> Dict:
    """The JSON-able spec of a stage: {"sensor": setting, "actuation": setting}, a ranged key as [lo, hi]; a part not given is nominal."""
    listed = lambda d: {k: list(v) if isinstance(v, tuple) else v for k, v in d.items()}
    return dict(sensor=listed(sensors.nominal_sensor() if sensor is None else sensor),
                actuation=listed(actuation.nominal_actuation() if actuation_setting is None else actuation_setting))


def spec_from_args(args) -> Optional[Dict]:
    """The spec the command line asks for, None without either flag (no stage at all).  ValueError as the parsers'."""
    s, a = getattr(args, "train_sensor", None), getattr(args, "train_actuation", None)
    if not s and not a:
        return None
    return fault_spec(parse_train_sensor(s) if s else None, parse_train_actuation(a) if a else None)


def _ends(v) -> Tuple[object, object, bool]:
    ranged = isinstance(v, (tuple, list))
    return (v[0], v[1], True) if ranged else (v, v, False)


def spec_table(spec: Dict, action_scale: float, ctrl_dt: float, actuator_names: Optional[Sequence[str]] = None) -> np.ndarray:
    """float32 [3, FAULT_NSLOT] -- lo, hi, kind per slot -- of a `fault_spec`: what `odk_fault_resample` reads.  The fixed slots are
    `sensors.fault_row`'s and `actuation.fault_row`'s of the setting's fixed part, bit for bit; a ranged key is FAULT_UNIFORM, the delays and
    `drop_len` FAULT_WHOLE.  `cutoff=a:b` draws the filter coefficient uniformly between filter_alpha(b) and filter_alpha(a) (BUILD-DEFINED:
    uniform in what the stage consumes, no division on the device); `quant` (radians) is divided by `action_scale`; `encoder_offset=X` and
    `offset=X` make every actuator's slot uniform in +-X (+-X / action_scale); the actuation SEED is the whole numbers 0 .. 2^24 - 1.
    ValueError (as `--train_actuation`'s) for a `freeze` the robot does not have."""
    scale = float(action_scale)
    table = np.zeros((3, FAULT_NSLOT), np.float32)
    S, A = table[:, :SENSOR_NPRM], table[:, SENSOR_NPRM:]      # views
    sen, act = dict(spec["sensor"]), dict(spec["actuation"])
    fixed = {k: _ends(v)[0] for k, v in sen.items()}
    S[0] = S[1] = sensors.fault_row(dict(fixed, encoder_offset=0.0))
    for k, v in sen.items():
        lo, hi, ranged = _ends(v)
        if ranged:
            S[:, _SENSOR_SLOT[k]] = lo, hi, FAULT_WHOLE if k in _WHOLE_KEYS else FAULT_UNIFORM
    bound = np.float32(float(sen["encoder_offset"]))
    if bound > 0:
        S[0, SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16], S[1, SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16] = -bound, bound
        S[2, SENSOR_ENC_OFFSET:SENSOR_ENC_OFFSET + 16] = FAULT_UNIFORM
    fixed = {k: _ends(v)[0] for k, v in act.items()}
    try:
        A[0] = A[1] = actuation.fault_row(dict(fixed, offset=0.0), scale, ctrl_dt, actuator_names)
    except ValueError as err:
        raise ValueError(str(err).replace("--actuation:", ACTUATION_FLAG + ":", 1))
    for k, v in act.items():
        lo, hi, ranged = _ends(v)
        if not ranged:
            continue
        if k == "cutoff":      # the coefficient falls as the cutoff rises
            lo, hi = actuation.filter_alpha(hi, ctrl_dt), actuation.filter_alpha(lo, ctrl_dt)
        elif k == "quant":
            lo, hi = float(lo) / scale, float(hi) / scale
        A[:, _ACTUATION_SLOT[k]] = lo, hi, FAULT_WHOLE if k in _WHOLE_KEYS else FAULT_UNIFORM
    bound = np.float32(float(act["offset"]) / scale)
    if bound > 0:
        A[0, ACT_OFFSET:ACT_OFFSET + 16], A[1, ACT_OFFSET:ACT_OFFSET + 16], A[2, ACT_OFFSET:ACT_OFFSET + 16] = -bound, bound, FAULT_UNIFORM
    A[:, ACT_SEED] = 0.0, actuation.SEED_SPAN - 1, FAULT_WHOLE
    return table


def fault_resample_reference(done: Optional[np.ndarray], spec: np.ndarray, seed: int, env_id_offset: int, state: np.ndarray,
                             sensor_fault: np.ndarray, act_fault: np.ndarray) -> np.ndarray:
    """`odk_fault_resample` restated in numpy float32, bit for bit: advances `state` ([n, FAULT_NSTATE] float32) and rewrites the redrawn
    envs' rows of `sensor_fault` ([n, SENSOR_NPRM]) and `act_fault` ([n, ACT_NPRM]) in place; returns the [n] mask of the redrawn envs.
    `done`: [n] or None; `spec`: [3, FAULT_NSLOT] float32.  Every operation is one float32 operation of the kernel's, in its order, and a
    FIXED slot is the same select (numpy.where moves bits: -0.0 and NaN come through).  Counts beyond 2^24 are not restated."""
    T, S = np.asarray(spec), state
    n = S.shape[0]
    assert T.dtype == np.float32 and T.shape == (3, FAULT_NSLOT) and S.dtype == np.float32 and S.shape == (n, FAULT_NSTATE)
    assert sensor_fault.dtype == np.float32 and sensor_fault.shape == (n, SENSOR_NPRM) and act_fault.dtype == np.float32 and act_fault.shape == (n, ACT_NPRM)
    one = np.float32(1)
    n0, ep0 = S[:, FAULT_HEAD].copy(), S[:, FAULT_EPISODE].copy()
    with np.errstate(all="ignore"):
        redraw = (n0 == 0) | ((np.asarray(done) != 0) if done is not None else False)
        episode = np.where(redraw, ep0 + one, ep0)
        env = (np.uint32(int(env_id_offset) & 0xFFFFFFFF) + np.arange(n, dtype=np.uint32)).astype(np.uint32)
        u = actuation.action_uniform(np.uint32(int(seed) & 0xFFFFFFFF), env[:, None], actuation._u32(episode)[:, None], np.uint32(0),
                                     (np.uint32(STREAM0) + np.arange(FAULT_NSLOT, dtype=np.uint32))[None, :])
        lo, hi, kind = T[0][None, :], T[1][None, :], T[2][None, :]
        uniform = lo + ((hi - lo) * u)
        whole = np.fmin(lo + np.floor(((hi - lo) + one) * u), hi)
        v = np.where(kind == FAULT_UNIFORM, uniform, np.where(kind == FAULT_WHOLE, whole, lo))
    assert v.dtype == np.float32 and v.shape == (n, FAULT_NSLOT)
    sensor_fault[redraw], act_fault[redraw] = v[redraw, :SENSOR_NPRM], v[redraw, SENSOR_NPRM:]
    S[:, FAULT_HEAD], S[:, FAULT_EPISODE] = n0 + one, episode
    return redraw


class FaultStage:
    """The faulty robot between a training env and its policy: per step `observe` redraws the fault rows of the envs that start an episode
    (`odk_fault_resample`) and hands the policy the observation their sensors deliver (`odk_sensor_apply`), `deliver` turns the policy's
    action into what the servos receive (`odk_action_apply`).  Owns the spec tensor, the two fault tables, the three state tensors,
    `sensor_obs` and `delivered`; three launches per step, fixed addresses, nothing allocated after construction.  `spec`: a `fault_spec`
    (an all-nominal one still runs: it hands every bit through); `seed`: the run's; the env's own `env_id_offset` separates the ranks."""

    def __init__(self, env, spec: Dict, seed: int = 0):
        import torch
        b = self.batch = env.batch
        self.spec, self.seed, self.env_id_offset = spec, int(seed) & 0xFFFFFFFF, int(getattr(env, "env_id_offset", 0)) & 0xFFFFFFFF
        names = [str(s) for s in b.model.a["names_actuator"]] if "names_actuator" in b.model.a else None
        self.action_scale, self.ctrl_dt = float(b.cfg.action_scale), float(env.dt)
        table = spec_table(spec, self.action_scale, self.ctrl_dt, names)
        n, dev = b.nenv, torch.device("cuda", b.device)
        Z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.table = torch.from_numpy(table).to(dev)
        self.sensor_fault, self.act_fault = torch.from_numpy(b.sensor_fault_rows(n)).to(dev), torch.from_numpy(b.action_fault_rows(n)).to(dev)
        self.fault_state, self.sensor_state, self.act_state = Z(n, FAULT_NSTATE), Z(n, SENSOR_NSTATE), Z(n, ACT_NSTATE)
        self.sensor_obs, self.delivered = Z(n, b.nobs), Z(n, int(b.model.nu))

    def reset(self) -> None:
        """After every reset of the env: the three states are zeroed, so the next `observe` redraws every env and both stages refill."""
        self.fault_state.zero_(); self.sensor_state.zero_(); self.act_state.zero_()

    def observe(self, obs, done):
        """`sensor_obs`, the row the policy reads, from the env's observation `obs` and the `done` of the step that wrote it."""
        b = self.batch
        b.fault_resample(done, self.table, self.seed, self.env_id_offset, self.fault_state, self.sensor_fault, self.act_fault)
        b.sensor_apply(obs, done, self.sensor_fault, self.sensor_state, self.sensor_obs)
        return self.sensor_obs

    def deliver(self, action, done):
        """`delivered`, the action the env steps with, from the policy's `action`; `done` is `observe`'s."""
        self.batch.action_apply(action, done, self.act_fault, self.act_state, self.delivered)
        return self.delivered

    def describe(self) -> Dict:
        """JSON-able: the spec with what it was drawn from -- what a checkpoint stores as `fault_spec` and `track` reports as `trained_under`."""
        return dict(sensor=dict(self.spec["sensor"]), actuation=dict(self.spec["actuation"]), seed=self.seed, redrawn="per episode")
