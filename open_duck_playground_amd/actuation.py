"""Actuation faults for `track` (`--actuation`, `--actuation_grid`): the keys and their parsers, the per-env fault rows `odk_action_apply`
reads (include/odk.h "Actuation faults"), and a numpy restatement of that kernel with its bits.  Host code only: no GPU, no torch."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from .sweeps import parse_axis_grid, grid_rows, parse_key_values, cell_rows

from .engine import (ACT_NPRM, ACT_NSTATE, ACT_GAIN, ACT_NOISE, ACT_LIMIT, ACT_ALPHA, ACT_QUANT, ACT_DROP_P, ACT_DROP_LEN, ACT_SEED, ACT_OFFSET,
                     ACT_FREEZE_AT, ACT_HEAD, ACT_EPISODE, ACT_HOLD, ACT_CALLS, ACT_DROPS, ACT_FILT, ACT_PREV, action_fault_rows)      # ODK_ACT_*

FREEZE_NONE = "none"
BOUND_KEYS = ("offset", "noise", "limit", "cutoff", "quant")      # rad, action units, action units, Hz, rad: each >= 0, 0 = off
STEP_KEYS = ("drop_len", "freeze_at")      # whole control steps: >= 1, >= 0
ACTUATION_KEYS = ("gain", "offset", "noise", "limit", "cutoff", "quant", "drop", "drop_len", "freeze", "freeze_at")
SEED_SPAN = 1 << 24      # a SEED slot is a whole number below it (exact in float32)


def nominal_actuation() -> Dict:
    """The link the env kernels describe: the servos receive what the policy asked for."""
    return dict(gain=1.0, offset=0.0, noise=0.0, limit=0.0, cutoff=0.0, quant=0.0, drop=0.0, drop_len=1, freeze=FREEZE_NONE, freeze_at=0)


def actuation_order(axis: str, value) -> float:
    """Where `value` sits on its axis' line: the number itself; for `freeze` 0 for `none` and 1 for any actuator; for `cutoff` and `limit`,
    whose 0 means off -- no filter is an infinite cutoff, no clamp an infinite limit -- minus the reciprocal, 0 for off: the values keep
    their order, and off, the nominal, ends the line above the largest of them instead of sitting below the smallest."""
    if axis == "freeze":
        return float(value != FREEZE_NONE)
    if axis in ("cutoff", "limit"):
        return -1.0 / float(value) if float(value) > 0 else 0.0
    return float(value)


def actuation_value(flag: str, name: str, value) -> object:
    """One value as an actuation setting holds it; ValueError with the reason for an unknown key, a `drop` outside 0 .. 1, a `drop_len` or
    `freeze_at` that is not a whole number of steps (>= 1, >= 0), a negative bound, step or cutoff and anything not finite.  `freeze` is
    an actuator's name or `none`: `actuation_blocks` knows the robot and checks it."""
    if name not in ACTUATION_KEYS:
        raise ValueError(f"{flag}: unknown key {name!r} (one of {', '.join(ACTUATION_KEYS)})")
    if name == "freeze":
        text = str(value).strip()
        if not text:
            raise ValueError(f"{flag}: freeze= needs an actuator's name, or {FREEZE_NONE}")
        return text
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{flag}: {name}={value!r} is not a number")
    if not np.isfinite(v):
        raise ValueError(f"{flag}: {name}={value} is not finite")
    if name in STEP_KEYS:
        least = 1 if name == "drop_len" else 0
        if v != round(v):
            raise ValueError(f"{flag}: {name}={value} is not a whole number of control steps")
        if int(v) < least:
            raise ValueError(f"{flag}: {name}={int(v)} is below {least} (whole control steps >= {least})")
        return int(v)
    if name == "drop" and not 0.0 <= v <= 1.0:
        raise ValueError(f"{flag}: drop={value} is outside 0 .. 1 (the probability that a step's command packet is lost)")
    if name in BOUND_KEYS and v < 0:
        raise ValueError(f"{flag}: {name}={value} is negative (0 = off)")
    return v


def parse_actuation(spec: str) -> Dict:
    """`--actuation cutoff=37.5,drop=0.05,freeze=left_knee,freeze_at=100` -> an actuation setting: `nominal_actuation()` with the named keys
    replaced.  ValueError for an unknown key, a key given twice and a value `actuation_value` refuses."""
    return parse_key_values("--actuation", spec, nominal_actuation(), "key", actuation_value)


def parse_actuation_grid(spec: str) -> List[Dict]:
    """`cutoff=5:40:3,drop=0:0.2:2` -> the settings of the grid, with `--grid`'s conventions (numpy.linspace, ends included, the last axis
    varies fastest, keys not named stay nominal).  `drop_len` and `freeze_at` axes must come out as whole numbers; `freeze` is no grid
    axis (its values are names)."""
    no_axis = {"freeze": "freeze takes an actuator's name, not a range: give one --actuation freeze=NAME per joint"}
    return grid_rows(parse_axis_grid("--actuation_grid", spec, ACTUATION_KEYS, "key", actuation_value, refused=no_axis), nominal_actuation())


def actuations_from_args(args) -> List[Dict]:
    """The actuation settings the command line asks for (`--actuation` in order, then `--actuation_grid`'s), [] without either flag.
    SystemExit with the reason for a setting that cannot be parsed and for actuation next to `--push` / `--push_grid`, `--plant` /
    `--plant_grid` or `--sensor` / `--sensor_grid` (a third cell axis) -- host work only, before any batch exists."""
    specs, grid = getattr(args, "actuation", None) or [], getattr(args, "actuation_grid", None)
    try:
        settings = [parse_actuation(s) for s in specs] + (parse_actuation_grid(grid) if grid else [])
    except ValueError as err:
        raise SystemExit(str(err))
    for other, noun in (("push", "push"), ("plant", "plant"), ("sensor", "sensor setting")):
        if settings and (getattr(args, other, None) or getattr(args, other + "_grid", None)):
            raise SystemExit(f"--actuation / --actuation_grid do not combine with --{other} / --{other}_grid: (command, {other}, actuation) would be "
                             f"a third cell axis; run the actuation sweep once per {noun}")
    return settings


def filter_alpha(cutoff_hz: float, ctrl_dt: float) -> np.float32:
    """The reference's `LowPassActionFilter.compute_alpha` with control_freq = 1 / ctrl_dt: (1 / cutoff) / (1 / control_freq + 1 / cutoff),
    in float64 and rounded once.  A cutoff of 0 is the filter off: 0."""
    cutoff = float(cutoff_hz)
    if not cutoff > 0.0:
        return np.float32(0.0)
    return np.float32((1.0 / cutoff) / (1.0 / (1.0 / float(ctrl_dt)) + 1.0 / cutoff))


def env_seeds(seed: int, n: int) -> np.ndarray:
    """[n] whole numbers below 2^24 from the run seed and the env index: env e's SEED slot."""
    return np.random.default_rng([int(seed), 0xAC7]).integers(0, SEED_SPAN, int(n)).astype(np.float32)


def freeze_index(setting: Dict, actuator_names: Optional[Sequence[str]]) -> int:
    """The actuator a setting freezes, -1 for `none`; ValueError (as `--actuation`'s) for a name the robot does not have."""
    name = setting["freeze"]
    if name == FREEZE_NONE:
        return -1
    names = [str(s) for s in (actuator_names or [])]
    if name not in names:
        raise ValueError(f"--actuation: freeze={name!r} is not one of the robot's actuators ({', '.join(names) or 'no names given'}), nor {FREEZE_NONE}")
    return names.index(name)


def fault_row(setting: Dict, action_scale: float, ctrl_dt: float, actuator_names: Optional[Sequence[str]] = None,
              offset_unit: Optional[np.ndarray] = None, seed: float = 0.0) -> np.ndarray:
    """One float32 fault row ([ACT_NPRM]) of an actuation setting, in action units: `offset` and `quant` (radians) are divided by
    `action_scale`, `cutoff` becomes `filter_alpha`.  `offset_unit` ([16], each in -1 .. 1): the robot's draw, which `offset` scales into
    its actuators' horn errors; without it the offsets stay 0."""
    row = action_fault_rows(1)[0]
    scale = float(action_scale)
    row[ACT_GAIN], row[ACT_NOISE], row[ACT_LIMIT] = setting["gain"], setting["noise"], setting["limit"]
    row[ACT_ALPHA] = filter_alpha(setting["cutoff"], ctrl_dt)
    row[ACT_QUANT] = float(setting["quant"]) / scale
    row[ACT_DROP_P], row[ACT_DROP_LEN], row[ACT_SEED] = setting["drop"], setting["drop_len"], seed
    if offset_unit is not None and float(setting["offset"]) > 0:
        row[ACT_OFFSET:ACT_OFFSET + 16] = np.asarray(offset_unit, np.float64) * (float(setting["offset"]) / scale)
    k = freeze_index(setting, actuator_names)
    if k >= 0:
        row[ACT_FREEZE_AT + k] = setting["freeze_at"]
    return row


def actuation_blocks(ncommands: int, settings: Sequence[Dict], envs_per_cell: int, seed: int, action_scale: float, ctrl_dt: float,
                     actuator_names: Optional[Sequence[str]] = None) -> np.ndarray:
    """float32 [n, ACT_NPRM] with n = ncommands * len(settings) * envs_per_cell: cell (c, s) drives envs (c * len(settings) + s) *
    envs_per_cell onwards -- `sweeps.cell_rows`' layout.  Every env draws its 16 offset units uniformly in -1 .. 1 from
    numpy.random.default_rng(seed), whether its cell has an `offset` or not (so a cell's robots do not depend on the other cells'
    settings): a cell with an offset is a population of mis-assembled robots.  Every env gets its own SEED (`env_seeds`)."""
    E, S = int(envs_per_cell), len(settings)
    n = int(ncommands) * S * E
    unit = np.random.default_rng(int(seed)).uniform(-1.0, 1.0, (n, 16))
    rows = cell_rows(np.stack([fault_row(s, action_scale, ctrl_dt, actuator_names) for s in settings]), ncommands, E)
    bound = cell_rows(np.asarray([float(s["offset"]) / float(action_scale) for s in settings], np.float64), ncommands, E)[:, None]
    rows[:, ACT_OFFSET:ACT_OFFSET + 16] = np.where(bound > 0, unit * bound, 0.0)      # (fault_row's product, for every env at once)
    rows[:, ACT_SEED] = env_seeds(seed, n)
    return rows


def reduce_link(state: np.ndarray, nblocks: int, envs_per_block: int) -> List[Dict]:
    """The "link" object of every block of `envs_per_block` envs from the stage's state rows: `dropped_share` = sum of DROPS / sum of CALLS
    over the block's envs (0 before any call)."""
    S = np.asarray(state, np.float64).reshape(int(nblocks), int(envs_per_block), ACT_NSTATE)
    calls, drops = S[:, :, ACT_CALLS].sum(axis=1), S[:, :, ACT_DROPS].sum(axis=1)
    return [dict(dropped_share=float(d / c) if c > 0 else 0.0) for c, d in zip(calls, drops)]


_M = (np.uint32(0x9E3779B9), np.uint32(0x85EBCA6B), np.uint32(0xC2B2AE35), np.uint32(0x27D4EB2F), np.uint32(0x7FEB352D), np.uint32(0x846CA68B))


def action_uniform(seed: np.ndarray, env: np.ndarray, episode: np.ndarray, step: np.ndarray, stream: np.ndarray) -> np.ndarray:
    """The stage's stateless uniform draw (include/odk.h), uint32 arrays in (they broadcast), float32 in 0 .. 1 (exclusive) out."""
    with np.errstate(over="ignore"):
        x = (np.asarray(seed, np.uint32) + _M[0] * np.asarray(env, np.uint32) + _M[1] * np.asarray(episode, np.uint32)
             + _M[2] * np.asarray(step, np.uint32) + _M[3] * np.asarray(stream, np.uint32)).astype(np.uint32)
        x = x ^ (x >> np.uint32(16))
        x = (x * _M[4]).astype(np.uint32)
        x = x ^ (x >> np.uint32(15))
        x = (x * _M[5]).astype(np.uint32)
        x = x ^ (x >> np.uint32(16))
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _u32(x: np.ndarray) -> np.ndarray:
    """A float32 count as the kernel's unsigned: the fraction dropped (counts here are whole and below 2^32)."""
    return np.asarray(x).astype(np.int64).astype(np.uint32)


def action_apply_reference(act: np.ndarray, done: Optional[np.ndarray], fault: np.ndarray, state: np.ndarray, nu: int) -> np.ndarray:
    """`odk_action_apply` restated in numpy float32, bit for bit: returns the delivered rows for `act` ([n, nu]) and advances `state`
    ([n, ACT_NSTATE] float32) in place.  `done`: [n] or None.  Every operation is one float32 operation of the kernel's, in its order, and
    every nominal stage is the same select (numpy.where moves bits: -0.0, NaN and inf come through).  Counts beyond 2^24 are not restated."""
    A, F, S = np.asarray(act, np.float32), np.asarray(fault, np.float32), state
    n = A.shape[0]
    assert S.dtype == np.float32 and S.shape == (n, ACT_NSTATE) and F.shape == (n, ACT_NPRM) and A.shape == (n, nu) and nu <= 16
    one, zero = np.float32(1), np.float32(0)
    a = np.zeros((n, 16), np.float32)
    a[:, :nu] = A
    n0, ep0, hold0, calls0, drops0 = (S[:, k].copy() for k in (ACT_HEAD, ACT_EPISODE, ACT_HOLD, ACT_CALLS, ACT_DROPS))
    filt0, prev0 = S[:, ACT_FILT:ACT_FILT + 16].copy(), S[:, ACT_PREV:ACT_PREV + 16].copy()
    with np.errstate(all="ignore"):
        # 1. the refill
        refill = (n0 == 0) | ((np.asarray(done) != 0) if done is not None else False)
        step, episode, hold = np.where(refill, zero, n0), np.where(refill, ep0 + one, ep0), np.where(refill, zero, hold0)
        y_prev, prev = np.where(refill[:, None], zero, filt0), np.where(refill[:, None], zero, prev0)
        seed = _u32(np.fmin(np.fmax(F[:, ACT_SEED], zero), np.float32(SEED_SPAN - 1)))
        env, uep, ust = np.arange(n, dtype=np.uint32), _u32(episode), _u32(step)
        # 2. gain, offset, noise, limit, filter, quantiser
        gain, off, amp, lim = F[:, ACT_GAIN:ACT_GAIN + 1], F[:, ACT_OFFSET:ACT_OFFSET + 16], F[:, ACT_NOISE:ACT_NOISE + 1], F[:, ACT_LIMIT:ACT_LIMIT + 1]
        alpha, q = F[:, ACT_ALPHA:ACT_ALPHA + 1], F[:, ACT_QUANT:ACT_QUANT + 1]
        a = np.where((gain < 1) | (gain > 1), gain * a, a)
        a = np.where((off < 0) | (off > 0), a + off, a)
        un = action_uniform(seed[:, None], env[:, None], uep[:, None], ust[:, None], np.arange(1, 17, dtype=np.uint32)[None, :])
        a = np.where(amp > 0, a + amp * ((un + un) - one), a)
        a = np.where(lim > 0, np.fmin(np.fmax(a, -lim), lim), a)
        y = (alpha * y_prev) + ((one - alpha) * a)
        filt = np.where(alpha > 0, y, y_prev)
        a = np.where(alpha > 0, y, a)
        a = np.where(q > 0, q * np.rint(a / q), a)
        # 3. packet loss
        u0 = action_uniform(seed, env, uep, ust, np.uint32(0))
        held = hold > 0
        drawn = ~held & (u0 < F[:, ACT_DROP_P])
        lost = held | drawn
        hold1 = np.where(held, hold - one, np.where(drawn, np.fmax(F[:, ACT_DROP_LEN], one) - one, hold))
        a = np.where(lost[:, None], prev, a)
        # 4. freeze
        f = F[:, ACT_FREEZE_AT:ACT_FREEZE_AT + 16]
        a = np.where((f >= 0) & (step[:, None] >= f), prev, a)
        # 5. the stores
        S[:, ACT_FILT:ACT_FILT + nu], S[:, ACT_PREV:ACT_PREV + nu] = filt[:, :nu], a[:, :nu]
        S[:, ACT_HEAD], S[:, ACT_EPISODE], S[:, ACT_HOLD] = step + one, episode, hold1
        S[:, ACT_CALLS], S[:, ACT_DROPS] = calls0 + one, np.where(lost, drops0 + one, drops0)
    out = np.ascontiguousarray(a[:, :nu])
    assert out.dtype == np.float32 and filt.dtype == np.float32 and hold1.dtype == np.float32
    return out
