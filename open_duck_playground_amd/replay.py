"""Fit the simulated plant to a recorded robot log by batched replay.

    python -m open_duck_playground_amd.replay --log robot_saved_obs.pkl --task flat_terrain_backlash \\
        --fit kp=0.5:1.5,frictionloss=0.3:3,armature=0.5:2,delay=0:2 --output fit.json

The log is the reference's `mujoco_saved_obs.pkl` (mujoco_infer.py pickles the observation row of every control step; the robot runtime
writes the same rows; `track --save_obs` writes the format).  Its actions are replayed open-loop through a batch whose envs are candidate
plants -- `track`'s plant axes: kp, mass, frictionloss, armature as scales on the model's values, delay in whole control steps -- and every
candidate is scored by how far its joints end up from what the log's encoders recorded: the numeric form of plot_saved_obs.py's overlay of
`last_action` and `dof_pos`.  `--fit` searches a box by the cross-entropy method, `--fit_grid` scores an explicit grid, `--synthesize` records a
log from a known plant (the tool's own sanity check).

The host part (the readers, the canonical table, the float32 restatements of the two kernels, score, ranking, the search) needs neither a
GPU nor torch; `Replayer` and `record` run the batch: a reset and T - 1 replays of one captured graph of (odk_log_apply, odk_step,
odk_replay_accumulate, odk_tracking_accumulate).  Only the accumulators come to the host."""
from __future__ import annotations

import argparse
import json
import pickle
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import engine
from .engine import (LOG_ACTION, LOG_COMMAND, REPLAY_ACCEL_ERR_SQ, REPLAY_CONTACT_AGREE, REPLAY_GYRO_ERR_SQ, REPLAY_NSLOT, REPLAY_POS_ERR_PEAK,
                     REPLAY_POS_ERR_SQ, REPLAY_POS_ERR_SUM, REPLAY_SAMPLES, REPLAY_VEL_ERR_SQ, TRACK_ENDED, TRACK_NACC, TRACK_STEPS, log_offsets, log_row)
from .sweeps import grid_rows, parse_axis_grid, parse_key_values
from .track import DELAY_RANDOM, DELAY_VALUES, PLANT_AXES, PLANT_SCALE_AXES, _plant_value

ENVS = ("joystick", "standing")
CHANNELS = ("pos", "vel", "gyro", "accel", "contact")
# BUILD-DEFINED search settings (INTEGRATION.md "Replaying a log")
DEFAULT_GENERATIONS = 6
ELITE_SHARE = 8            # the elites are the best 1 / ELITE_SHARE of a generation
DELAY_SHARE_FLOOR = 0.05   # no delay value's share falls below this between generations
DEFAULT_FIT_ENVS = 1024
START_WARN_RAD = 0.2       # a log must begin near the home pose: the warning threshold on O_0's largest joint deviation
EXCITATION_AMPLITUDE, EXCITATION_RAMP_STEPS, EXCITATION_HZ = 0.3, 25, (0.5, 2.0)
# what training randomises each axis over (randomize.py:48-59, :69-71, :89-95; the action delay is drawn from 0..2 every step)
TRAINING_RANGES = {"kp": (0.9, 1.1), "mass": (0.9, 1.1), "frictionloss": (0.9, 1.1), "armature": (1.0, 1.05), "delay": (0, 2)}


# ---- the log and its canonical table (host, numpy)
def obs_width(nu: int, env: str = "joystick") -> int:
    """The env's nobs for a model with `nu` actuators: Joystick 17 + 6 nu, Standing 15 + 5 nu (include/odk.h)."""
    return 17 + 6 * int(nu) if env == "joystick" else 15 + 5 * int(nu)


def obs_fields(nu: int, env: str = "joystick") -> Dict[str, int]:
    """Where the fields of an observation row start (csrc/odk_obs_layout.h obs_at)."""
    nu = int(nu)
    f = {"gyro": 0, "accel": 3, "command": 6, "pos": 13, "vel": 13 + nu, "last_act": 13 + 2 * nu, "last_last_act": 13 + 3 * nu,
         "last_last_last_act": 13 + 4 * nu}
    if env == "joystick":
        f["motor_targets"] = 13 + 5 * nu
    f["contact"] = 13 + (6 if env == "joystick" else 5) * nu
    return f


def read_log(path: str) -> np.ndarray:
    """The rows of a log, [T, width] float32: the reference's pickle (a list of 1-D arrays, one per control step; read with
    reference_motion's numpy-only unpickler) or an .npz with an `obs` array.  ValueError for anything else."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            if "obs" not in z.files:
                raise ValueError(f"{path}: an .npz log holds an `obs` array [T, width]; it has {', '.join(z.files) or 'nothing'}")
            rows = np.asarray(z["obs"])
    else:
        from .reference_motion import safe_load
        with open(path, "rb") as f:
            try:
                data = safe_load(f.read())
            except pickle.UnpicklingError as err:
                raise ValueError(f"{path}: {err}")
        if not isinstance(data, (list, tuple)) or not data:
            raise ValueError(f"{path}: a log is a pickled list of one 1-D array per control step, got {type(data).__name__}")
        try:
            rows = np.stack([np.asarray(r, np.float32).reshape(-1) for r in data])
        except ValueError:
            raise ValueError(f"{path}: the rows of the log differ in length")
    if rows.ndim != 2 or rows.dtype.kind != "f":
        raise ValueError(f"{path}: a log is [T, width] floats, got shape {rows.shape} of {rows.dtype}")
    if not np.isfinite(rows).all():
        raise ValueError(f"{path}: the log holds values that are not finite")
    return np.ascontiguousarray(rows, np.float32)


def write_log(path: str, rows: np.ndarray) -> None:
    """The reference's format (track.save_obs), or an .npz with `obs`."""
    if str(path).endswith(".npz"):
        np.savez_compressed(path, obs=np.asarray(rows, np.float32))
        return
    with open(path, "wb") as f:
        pickle.dump([np.array(o, np.float32) for o in rows], f)


def check_width(rows: np.ndarray, nu: int, env: str = "joystick") -> None:
    """ValueError, naming both widths, for rows that are not this env's observation of this model; and for a log too short to replay."""
    want = obs_width(nu, env)
    if rows.shape[1] != want:
        other = [e for e in ENVS if e != env][0]
        raise ValueError(f"the log's rows are {rows.shape[1]} floats wide, the {env} env of a model with {nu} actuators observes {want} "
                         f"({'17 + 6 nu' if env == 'joystick' else '15 + 5 nu'}; --env {other} observes {obs_width(nu, other)})")
    if rows.shape[0] < 2:
        raise ValueError(f"a log of {rows.shape[0]} row(s) replays no step: row k + 1 holds the action and the answer of step k")


def log_table(rows: np.ndarray, nu: int, env: str = "joystick") -> np.ndarray:
    """The canonical table [T - 1, log_row(nu)] float32 of a log [T, nobs] (include/odk.h "Log replay").  Row O_k was saved before the policy
    computed a_k, so a_k = O_{k+1}[last_act]: table row k holds the command, the action, the joint positions, the joint velocities (the
    observation's own float32, NOT divided by dof_vel_scale: that division is not invertible in float32 and the kernel multiplies instead),
    the gyro, the accelerometer and the contacts of O_{k+1} -- what step k applies and what the robot then reported."""
    check_width(rows, nu, env)
    f, o, nu = obs_fields(nu, env), log_offsets(nu), int(nu)
    nxt = np.asarray(rows, np.float32)[1:]
    t = np.zeros((nxt.shape[0], log_row(nu)), np.float32)
    for dst, src, n in (("command", "command", 7), ("action", "last_act", nu), ("pos", "pos", nu), ("vel", "vel", nu), ("gyro", "gyro", 3),
                        ("accel", "accel", 3), ("contact", "contact", 2)):
        t[:, o[dst]:o[dst] + n] = nxt[:, f[src]:f[src] + n]
    return t


def start_deviation(rows: np.ndarray, nu: int, env: str = "joystick") -> float:
    """The largest joint deviation of O_0 from the home pose, radians."""
    f = obs_fields(nu, env)
    return float(np.abs(rows[0, f["pos"]:f["pos"] + int(nu)]).max())


def excitation(nu: int, steps: int, seed: int = 0) -> np.ndarray:
    """The open-loop excitation [steps, nu] float32: per actuator a sinusoid of amplitude 0.3 action units, frequency U(0.5, 2) Hz and phase
    U(0, 2 pi) from numpy.random.default_rng(seed) (frequencies drawn first), ramped in linearly over 25 steps; 50 control steps a second."""
    rng = np.random.default_rng(int(seed))
    hz, ph = rng.uniform(*EXCITATION_HZ, size=int(nu)), rng.uniform(0.0, 2.0 * np.pi, size=int(nu))
    k = np.arange(int(steps), dtype=np.float64)[:, None]
    ramp = np.minimum(1.0, (k + 1.0) / EXCITATION_RAMP_STEPS)
    return (EXCITATION_AMPLITUDE * ramp * np.sin(2.0 * np.pi * hz[None] * k * 0.02 + ph[None])).astype(np.float32)


def as_logged(first: np.ndarray, obs: np.ndarray, actions: np.ndarray, nu: int, env: str = "joystick") -> np.ndarray:
    """The env's observation rows after steps 0 .. n - 1 (`obs` [n, nobs]) behind the log's row 0 (`first`), in the LOG's convention.  The env
    builds the observation of step k before it stores a_k (joystick.py:437-466: its last_act is a_{k-1}); mujoco_infer.py and the robot
    runtime store a_k first, so the logged row k + 1 carries last_act = a_k, last_last_act = a_{k-1}, last_last_last_act = a_{k-2} -- the
    three columns are rewritten from `actions` ([n, nu]) and row 0's own history."""
    f, nu = obs_fields(nu, env), int(nu)
    rows = np.concatenate([np.asarray(first, np.float32).reshape(1, -1), np.asarray(obs, np.float32)])
    cols = [f["last_act"], f["last_last_act"], f["last_last_last_act"]]
    past = [rows[0, c:c + nu].copy() for c in cols]                 # a_{-1}, a_{-2}, a_{-3}
    hist = past[::-1] + [np.asarray(a, np.float32) for a in actions]   # a_{-3} .. a_{n-1}: a_k sits at 3 + k
    for k in range(len(obs)):
        for j, c in enumerate(cols):
            rows[k + 1, c:c + nu] = hist[3 + k - j]
    return rows


# ---- float32 restatements of the two kernels (csrc/odk_reports.hip log_apply_kernel / replay_kernel): they have the kernels' bits
def log_apply_np(table: np.ndarray, track: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(action [nenv, nu], command [nenv, 7]) of the step about to run: row min(max(t, 0), nrow - 1), t = STEPS (STEPS - 1 once ENDED)."""
    table, track = np.asarray(table, np.float32), np.asarray(track, np.float32)
    nu = (table.shape[1] - 15) // 3
    t = np.where(track[:, TRACK_ENDED] != 0, track[:, TRACK_STEPS] - np.float32(1), track[:, TRACK_STEPS])
    k = np.minimum(np.maximum(t, np.float32(0)), np.float32(table.shape[0] - 1)).astype(np.int64)
    return table[k, LOG_ACTION:LOG_ACTION + nu].copy(), table[k, LOG_COMMAND:LOG_COMMAND + 7].copy()


def replay_accumulate_np(acc: np.ndarray, priv: np.ndarray, done: np.ndarray, track: np.ndarray, table: np.ndarray, nobs: int,
                         vel_scale: float) -> np.ndarray:
    """One odk_replay_accumulate launch on host arrays: `acc` [nenv, 16, REPLAY_NSLOT] float32 is updated in place and returned.  `track` is
    the tracking accumulator BEFORE this step's odk_tracking_accumulate.  Every operation is a float32 one, products rounded before sums."""
    F = np.float32
    table = np.asarray(table, F)
    nu = (table.shape[1] - 15) // 3
    o = log_offsets(nu)
    s = np.asarray(track, F)[:, TRACK_STEPS]
    sample = (np.asarray(track, F)[:, TRACK_ENDED] == 0) & (np.asarray(done, F) == 0) & (s >= 0) & (s < F(table.shape[0]))
    vs = F(vel_scale)
    for e in np.nonzero(sample)[0]:
        Q, L, A = np.asarray(priv[e, nobs:], F), table[int(s[e])], acc[e]
        dp = Q[15:15 + nu] - L[o["pos"]:o["pos"] + nu]
        dv = (Q[15 + nu:15 + 2 * nu] * vs).astype(F) - L[o["vel"]:o["vel"] + nu]
        A[:nu, REPLAY_POS_ERR_SUM] += dp
        A[:nu, REPLAY_POS_ERR_SQ] += (dp * dp).astype(F)
        A[:nu, REPLAY_VEL_ERR_SQ] += (dv * dv).astype(F)
        A[:nu, REPLAY_POS_ERR_PEAK] = np.maximum(A[:nu, REPLAY_POS_ERR_PEAK], np.abs(dp))
        dg, da = Q[0:3] - L[o["gyro"]:o["gyro"] + 3], Q[3:6] - L[o["accel"]:o["accel"] + 3]
        A[:3, REPLAY_GYRO_ERR_SQ] += (dg * dg).astype(F)
        A[:3, REPLAY_ACCEL_ERR_SQ] += (da * da).astype(F)
        A[:2, REPLAY_CONTACT_AGREE] += ((Q[16 + 3 * nu:18 + 3 * nu] != 0) == (L[o["contact"]:o["contact"] + 2] > F(0.5))).astype(F)
        A[0, REPLAY_SAMPLES] += F(1)
    return acc


# ---- score and ranking (host, float64 from the accumulator)
def default_weights(vel_scale: float) -> Dict[str, float]:
    """Joint position 1, joint velocity dof_vel_scale^2 (a rad/s residual weighs as the policy sees it), the base-side channels 0: they drift
    open-loop, and mujoco_infer.py adds 1.3 to the accelerometer."""
    return {"pos": 1.0, "vel": float(vel_scale) ** 2, "gyro": 0.0, "accel": 0.0, "contact": 0.0}


def channel_means(acc: np.ndarray, nu: int, vel_scale: float) -> Dict[str, np.ndarray]:
    """Per env the mean squared residual of every channel, float64: pos in rad^2 and vel in (rad/s)^2 over samples x actuators, gyro and accel
    over samples x 3 axes, contact the share of (sample, foot) pairs that disagree.  An env without a sample has NaN everywhere."""
    a = np.asarray(acc, np.float64).reshape(-1, 16, REPLAY_NSLOT)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(a[:, 0, REPLAY_SAMPLES] > 0, a[:, 0, REPLAY_SAMPLES], np.nan)
        return {"pos": a[:, :nu, REPLAY_POS_ERR_SQ].sum(1) / (n * nu),
                "vel": a[:, :nu, REPLAY_VEL_ERR_SQ].sum(1) / (n * nu) / float(vel_scale) ** 2,
                "gyro": a[:, :3, REPLAY_GYRO_ERR_SQ].sum(1) / (n * 3), "accel": a[:, :3, REPLAY_ACCEL_ERR_SQ].sum(1) / (n * 3),
                "contact": 1.0 - a[:, :2, REPLAY_CONTACT_AGREE].sum(1) / (n * 2)}


def score(acc: np.ndarray, nu: int, vel_scale: float, weights: Optional[Dict[str, float]] = None) -> np.ndarray:
    """Per env the sum over the channels of weight x mean squared residual (a channel of weight 0 is not read); inf without a sample."""
    w = default_weights(vel_scale) if weights is None else weights
    means = channel_means(acc, nu, vel_scale)
    total = np.zeros(len(means["pos"]), np.float64)
    for c in CHANNELS:
        if float(w.get(c, 0.0)) != 0.0:
            total = total + float(w[c]) * means[c]
    return np.where(np.isnan(total), np.inf, total)


def survival(track: np.ndarray, nrow: int) -> Tuple[np.ndarray, np.ndarray]:
    """(lasted [nenv] bool, steps [nenv]) from the tracking accumulator after the nrow replayed steps: an env lasted when its first episode was
    still running at the end of the log; `steps` are the first-episode steps it ran."""
    t = np.asarray(track, np.float64)
    return (t[:, TRACK_ENDED] == 0) & (t[:, TRACK_STEPS] >= nrow), t[:, TRACK_STEPS].astype(np.int64)


def rank_order(scores: Sequence[float], lasted: Sequence[bool], steps: Sequence[int]) -> np.ndarray:
    """The candidates, best first.  Lexicographic, no penalty constant: a candidate whose episode ended before the log did ranks behind every
    one that lasted; among the early enders the longer survivor comes first; the score decides within equal survival."""
    scores, lasted, steps = np.asarray(scores, np.float64), np.asarray(lasted, bool), np.asarray(steps, np.int64)
    return np.lexsort((scores, np.where(lasted, 0, -steps), ~lasted))


# ---- the fitted axes
def replay_plant(spec: Optional[str] = None) -> Dict:
    """`--plant KEY=V,...` for a replay: every scale 1 and delay 0 with the named axes replaced, `track`'s validators; the sampled delay
    (`random`) is refused, a replay is deterministic."""
    base = {"kp": 1.0, "mass": 1.0, "frictionloss": 1.0, "armature": 1.0, "delay": 0}
    plant = parse_key_values("--plant", spec, base, "axis", _plant_value) if spec else base
    if plant["delay"] == DELAY_RANDOM:
        raise ValueError("--plant: delay=random is a sampled delay; a replay binds every env's delay (0, 1 or 2)")
    return plant


def parse_fit(spec: str) -> List[Tuple[str, float, float]]:
    """`AXIS=LO:HI,...` -> (axis, lo, hi) in the order written: `track`'s plant axes, both ends through `track`'s validators (a scale is a
    finite number > 0, a delay a whole number within 0..2), lo <= hi.  ValueError as `--fit`'s otherwise."""
    axes = []
    for part in str(spec).split(","):
        part = part.strip()
        if not part:
            continue
        name, _, rng = part.partition("=")
        name = name.strip()
        if name not in PLANT_AXES:
            raise ValueError(f"--fit: unknown axis {name!r} (one of {', '.join(PLANT_AXES)})")
        if any(name == a for a, _, _ in axes):
            raise ValueError(f"--fit: axis {name!r} given twice")
        bits = rng.split(":")
        if len(bits) != 2:
            raise ValueError(f"--fit: {part!r} is not {name}=LO:HI")
        lo, hi = (_plant_value("--fit", name, b.strip()) for b in bits)
        if DELAY_RANDOM in (lo, hi):
            raise ValueError(f"--fit: {part!r}: a fitted delay is a range within {DELAY_VALUES[0]}..{DELAY_VALUES[-1]}")
        if lo > hi:
            raise ValueError(f"--fit: {part!r}: LO is above HI")
        axes.append((name, lo, hi))
    if not axes:
        raise ValueError("--fit: no axis given")
    return axes


def parse_fit_grid(spec: str, base: Dict) -> List[Dict]:
    """`AXIS=a:b:n,...` -> the plants of the grid (sweeps.parse_axis_grid, `track --plant_grid`'s conventions), the axes not named from `base`."""
    def value(flag, name, v):
        out = _plant_value(flag, name, v)
        if out == DELAY_RANDOM:
            raise ValueError(f"{flag}: delay=random is a sampled delay; a replay binds every env's delay")
        return out
    return grid_rows(parse_axis_grid("--fit_grid", spec, PLANT_AXES, value=value), base)


def parse_weights(specs: Optional[Sequence[str]], vel_scale: float) -> Dict[str, float]:
    """`--weight CHANNEL=W` (repeatable) on top of `default_weights`: a finite weight >= 0 of one of CHANNELS."""
    w = default_weights(vel_scale)
    for spec in specs or []:
        name, eq, text = str(spec).partition("=")
        name = name.strip()
        if not eq or name not in CHANNELS:
            raise ValueError(f"--weight: {spec!r} is not CHANNEL=W with a channel of {', '.join(CHANNELS)}")
        try:
            v = float(text)
        except ValueError:
            raise ValueError(f"--weight: {spec!r}: {text!r} is not a number")
        if not np.isfinite(v) or v < 0:
            raise ValueError(f"--weight: {spec!r}: a weight is a finite number >= 0")
        w[name] = v
    return w


def plant_string(plant: Dict) -> str:
    """A plant as a `--plant` string that `track.parse_plant` accepts (repr floats: they parse back to the same float64)."""
    return ",".join(f"{k}={int(plant[k]) if k == 'delay' else repr(float(plant[k]))}" for k in PLANT_AXES)


def in_training_ranges(plant: Dict) -> Dict[str, bool]:
    return {k: bool(TRAINING_RANGES[k][0] <= float(plant[k]) <= TRAINING_RANGES[k][1]) for k in PLANT_AXES}


# ---- the search (host)
def cem(evaluate: Callable, axes: Sequence[Tuple[str, float, float]], n: int, generations: int = DEFAULT_GENERATIONS, seed: int = 0) -> Dict:
    """Cross-entropy search, one candidate per env.  `evaluate({axis: [n] values}) -> (scores, lasted, steps)`; `axes` as `parse_fit` gives
    them.  Generation 0 is uniform in the box; the elites are the best n // ELITE_SHARE (at least 2) in `rank_order`; the next generation is
    Gaussian with the elites' mean and std per axis, clipped to the box; `delay` is categorical over the whole numbers of its range with
    the elites' shares, floored at DELAY_SHARE_FLOOR.  Draws come from numpy.random.default_rng(seed).  Returns the best candidate ever
    seen (in rank order: a candidate that lasted beats one that did not), the history per generation, and the share of candidates that
    did not last."""
    rng = np.random.default_rng(int(seed))
    n, nel = int(n), max(2, int(n) // ELITE_SHARE)
    if n < 2:
        raise ValueError(f"a search needs at least 2 candidates a generation, got {n}")
    cont = [(a, float(lo), float(hi)) for a, lo, hi in axes if a != "delay"]
    dl = next(((int(lo), int(hi)) for a, lo, hi in axes if a == "delay"), None)
    dvals = np.arange(dl[0], dl[1] + 1) if dl else None
    mean, std, shares = {}, {}, (np.full(len(dvals), 1.0 / len(dvals)) if dl else None)
    best, history, fell, total = None, [], 0, 0
    for g in range(int(generations)):
        cand = {}
        for a, lo, hi in cont:
            cand[a] = rng.uniform(lo, hi, size=n) if g == 0 else np.clip(rng.normal(mean[a], std[a], size=n), lo, hi)
        if dl:
            cand["delay"] = rng.choice(dvals, size=n, p=shares)
        scores, lasted, steps = (np.asarray(x) for x in evaluate(cand))
        order = rank_order(scores, lasted, steps)
        el = order[:nel]
        for a, _, _ in cont:
            mean[a], std[a] = float(cand[a][el].mean()), float(cand[a][el].std())
        if dl:
            shares = np.maximum(np.array([(cand["delay"][el] == v).mean() for v in dvals]), DELAY_SHARE_FLOOR)
            shares = shares / shares.sum()
        i = int(order[0])
        top = dict(plant={a: (int(cand[a][i]) if a == "delay" else float(cand[a][i])) for a in cand}, score=float(scores[i]), lasted=bool(lasted[i]),
                   steps=int(steps[i]), generation=g)
        if best is None or rank_order([best["score"], top["score"]], [best["lasted"], top["lasted"]], [best["steps"], top["steps"]])[0] == 1:
            best = top
        fell += int((~np.asarray(lasted, bool)).sum()); total += n
        history.append(dict(generation=g, best_score=top["score"], best_plant=top["plant"], elite_mean=dict(mean), elite_std=dict(std),
                            delay_shares=({int(v): float(s) for v, s in zip(dvals, shares)} if dl else None),
                            fell_share=float((~np.asarray(lasted, bool)).mean())))
    return dict(best=best, history=history, fell_share=fell / max(total, 1), elite_mean=dict(mean), elite_std=dict(std),
                delay_shares=history[-1]["delay_shares"])


def joint_report(acc_row: np.ndarray, nu: int, vel_scale: float, names: Sequence[str]) -> List[Dict]:
    """Per joint the RMS, bias and peak of the position residual (rad) and the RMS of the velocity residual (rad/s) of one env's accumulator
    row [16, REPLAY_NSLOT]: the numeric form of plot_saved_obs.py's first figure."""
    a = np.asarray(acc_row, np.float64).reshape(16, REPLAY_NSLOT)
    n = a[0, REPLAY_SAMPLES]
    if n <= 0:
        return []
    return [dict(joint=str(names[u]), pos_rms=float(np.sqrt(a[u, REPLAY_POS_ERR_SQ] / n)), pos_bias=float(a[u, REPLAY_POS_ERR_SUM] / n),
                 pos_peak=float(a[u, REPLAY_POS_ERR_PEAK]), vel_rms=float(np.sqrt(a[u, REPLAY_VEL_ERR_SQ] / n) / float(vel_scale))) for u in range(int(nu))]


# ---- the batch
def make_env(task: str, env: str, num_envs: int, steps: int, device: int = 0, xml: Optional[str] = None):
    """The env a replay runs on: noise level 0, pushes off, no domain randomisation, an episode longer than the log."""
    from . import joystick, standing
    if env not in ENVS:
        raise ValueError(f"unknown env {env!r} (one of {', '.join(ENVS)})")
    cls = joystick.Joystick if env == "joystick" else standing.Standing
    overrides = {"episode_length": int(steps) + 16, "noise_config.level": 0.0, "push_config.enable": False}
    return cls(task=task, num_envs=int(num_envs), device=int(device), autoreset=True, lanes_per_env=64 if int(num_envs) <= 1024 else 0,
               config_overrides=overrides, **({"xml_path": xml} if xml else {}))


class Replayer:
    """`num_envs` candidate plants replaying one log of T rows (`rows` [T, nobs]) on the GPU.  `run(plants)` is a reset, the start state of
    O_0 in every env, and T - 1 replays of one captured graph of (log_apply, step, replay_accumulate, tracking_accumulate); it returns the
    replay accumulator [num_envs, 16, REPLAY_NSLOT] and the tracking accumulator as numpy arrays.  `trace`: also the observation rows of
    that env, [T - 1, nobs]."""

    def __init__(self, rows: np.ndarray, task: str = "flat_terrain", env: str = "joystick", num_envs: int = 64, device: int = 0,
                 xml: Optional[str] = None, use_graph: bool = True):
        import torch
        self.torch, self.kind = torch, env
        self.env = make_env(task, env, num_envs, len(rows), device, xml)
        b = self.batch = self.env.batch
        self.nu, self.n = int(b.model.nu), int(num_envs)
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.table_np = log_table(self.rows, self.nu, env)
        self.nrow = int(self.table_np.shape[0])
        self.vel_scale = float(np.float32(b.cfg.dof_vel_scale))
        dev = b.obs.device
        self.table = torch.from_numpy(self.table_np).to(dev)
        self.cmd = torch.zeros(self.n, engine.NCOMMAND, device=dev)
        self.delays = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.action = torch.zeros(self.n, self.nu, device=dev)
        self.track = torch.zeros(self.n, TRACK_NACC, device=dev)
        self.acc = torch.zeros(self.n, 16, REPLAY_NSLOT, device=dev)
        self.env.set_commands(self.cmd)
        self.env.set_action_delays(self.delays)
        self.use_graph, self.graph = use_graph, None

    def close(self):
        self.env.set_commands(None)
        self.env.set_action_delays(None)
        self.batch.close()

    def _one_step(self):
        b = self.batch
        b.log_apply(self.table, self.track, self.action)
        b.step(self.action)
        b.replay_accumulate(self.acc, self.track, self.table)       # before the tracking accumulator advances STEPS and sets ENDED
        b.tracking_accumulate(self.track)

    def _start(self):
        """Every env at the one deterministic start of O_0: home keyframe for the floating base, the actuated joints at default + O_0's
        deviations with O_0's velocities, backlash joints 0, everything else at rest, warm start 0; the carried actions and (Joystick) the
        motor targets from O_0."""
        b, nu, f = self.batch, self.nu, obs_fields(self.nu, self.kind)
        a = b.model.a
        o0 = self.rows[0]
        trn = np.asarray(a["actuator_trnid"]).reshape(nu, -1)[:, 0]
        qadr, dadr = np.asarray(a["jnt_qposadr"])[trn], np.asarray(a["jnt_dofadr"])[trn]
        qpos = np.array(a["key_qpos"], np.float64).reshape(-1)[:b.model.nq].copy()
        free = np.ones(b.model.nq, bool); free[:7] = False
        qpos[free] = 0.0                                            # (backlash joints and any other passive joint)
        qpos[qadr] = (np.asarray(a["key_ctrl"], np.float32).reshape(-1)[:nu] + o0[f["pos"]:f["pos"] + nu]).astype(np.float32)
        qvel = np.zeros(b.model.nv, np.float32)
        qvel[dadr] = o0[f["vel"]:f["vel"] + nu] / np.float32(self.vel_scale)
        rep = lambda v: np.repeat(np.asarray(v, np.float32)[None], self.n, axis=0)
        b.set_state(rep(qpos), rep(qvel), np.zeros((self.n, b.model.nv), np.float32))
        info = b.info()
        hist = np.concatenate([o0[f[k]:f[k] + nu] for k in ("last_act", "last_last_act", "last_last_last_act")])
        for k in ("last_act", "last_last_act", "last_last_last_act"):
            info[k][:, :nu] = o0[f[k]:f[k] + nu]
        info["action_history"][:, :3 * nu] = hist
        if "motor_targets" in f:
            info["motor_targets"][:, :nu] = o0[f["motor_targets"]:f["motor_targets"] + nu]
        b.set_records(info["_records"])

    def set_plants(self, plants: Dict[str, np.ndarray]) -> None:
        """Env e's plant: `plants[axis][e]` for every axis of PLANT_AXES (scales in float64; randomize.scale_fields rounds once)."""
        from . import randomize
        scales = {k: np.asarray(plants[k], np.float64).reshape(self.n) for k in PLANT_SCALE_AXES}
        randomize.apply(self.batch, randomize.scale_fields(randomize.nominal_fields(self.batch.model, self.n), scales))
        self.delays.copy_(self.torch.from_numpy(np.asarray(plants["delay"], np.int32).reshape(self.n)))

    def run(self, plants: Dict[str, np.ndarray], trace: Optional[int] = None, seed: int = 0, steps: Optional[int] = None,
            after_start: Optional[Callable] = None):
        """One replay of `plants` (`set_plants`).  `steps`: control steps to run (default: the table's rows; past them the accumulator is
        left alone); `after_start(batch)`: a preset of the caller's on top of the start state (tests)."""
        torch = self.torch
        steps = self.nrow if steps is None else int(steps)
        self.set_plants(plants)
        self.track.zero_(); self.acc.zero_()
        self._first_command()
        self.env.reset(int(seed))
        self._start()
        if after_start is not None:
            after_start(self.batch)
        rows = torch.zeros(steps, self.batch.nobs, device=self.acc.device) if trace is not None else None
        for k in range(steps):
            if not self.use_graph:
                self._one_step()
            elif self.graph is None:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._one_step()                    # warm-up: this IS step 0
                torch.cuda.current_stream().wait_stream(side)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self._one_step()                    # captured, not executed
            else:
                self.graph.replay()
            if rows is not None:
                rows[k].copy_(self.batch.obs[int(trace)])
        out = self.acc.cpu().numpy(), self.track.cpu().numpy()
        return out + (rows.cpu().numpy(),) if rows is not None else out

    def _first_command(self):
        """The command row that the reset must find: the log's first (a zeroed clock reads row 0)."""
        self.cmd.copy_(self.table[0, LOG_COMMAND:LOG_COMMAND + 7].expand(self.n, 7))

    def evaluate(self, plants: Dict[str, np.ndarray], weights: Optional[Dict[str, float]] = None):
        """(scores, lasted, steps, acc, track) of one replay of `plants`."""
        acc, track = self.run(plants)
        lasted, steps = survival(track, self.nrow)
        return score(acc, self.nu, self.vel_scale, weights), lasted, steps, acc, track


def plant_columns(plants: Sequence[Dict], n: int) -> Dict[str, np.ndarray]:
    """One env per plant, the envs past the last plant repeating it: {axis: [n]}."""
    idx = np.minimum(np.arange(int(n)), len(plants) - 1)
    return {k: np.asarray([plants[i][k] for i in idx], np.int32 if k == "delay" else np.float64) for k in PLANT_AXES}


def record(task: str = "flat_terrain", env: str = "joystick", plant: Optional[Dict] = None, actions: Optional[np.ndarray] = None, steps: int = 60,
           command: Optional[Sequence[float]] = None, device: int = 0, xml: Optional[str] = None, seed: int = 0) -> np.ndarray:
    """A synthetic log [steps + 1, nobs] float32 in the reference's layout: `actions` ([steps, nu]; default: `excitation(nu, steps, seed)`) run
    open-loop on `plant` from the home pose at rest, through the replay's own start and launch sequence.  Row 0 is the start (zero joint
    deviations, velocities and past actions, the home motor targets, the command), row k + 1 the observation after step k.  RuntimeError
    when the robot falls before the log ends."""
    from . import constants
    plant = dict(replay_plant(), **(plant or {}))
    if xml is None:
        nu = int(constants.task_to_model(task).nu)
    else:
        from .model import Model
        nu = int(Model.from_xml(xml).nu)
    acts = excitation(nu, steps, seed) if actions is None else np.ascontiguousarray(actions, np.float32).reshape(-1, nu)
    f, W = obs_fields(nu, env), obs_width(nu, env)
    rows = np.zeros((len(acts) + 1, W), np.float32)
    rows[1:, f["last_act"]:f["last_act"] + nu] = acts
    if command is not None:
        rows[:, f["command"]:f["command"] + 7] = np.asarray(command, np.float32).reshape(7)
    r = Replayer(rows, task, env, 1, device, xml, use_graph=False)
    try:
        if "motor_targets" in f:
            r.rows[0, f["motor_targets"]:f["motor_targets"] + nu] = np.asarray(r.batch.model.a["key_ctrl"], np.float32).reshape(-1)[:nu]
        acc, track, obs = r.run(plant_columns([plant], 1), trace=0)
        if not survival(track, r.nrow)[0][0]:
            raise RuntimeError(f"record: the robot fell after {int(track[0, TRACK_STEPS])} of {r.nrow} steps on plant {plant_string(plant)}")
        return as_logged(r.rows[0], obs, acts, nu, env)
    finally:
        r.close()


# ---- the command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m open_duck_playground_amd.replay", description=__doc__.split("\n\n")[0])
    p.add_argument("--log", help="the log to fit: mujoco_saved_obs.pkl's format, or an .npz with an `obs` array")
    p.add_argument("--task", default="flat_terrain")
    p.add_argument("--env", default="joystick", choices=ENVS)
    p.add_argument("--xml", default=None, help="a robot of one's own instead of a shipped task")
    p.add_argument("--fit", default=None, help="AXIS=LO:HI[,...]: search this box by the cross-entropy method")
    p.add_argument("--fit_grid", default=None, help="AXIS=a:b:n[,...]: score this grid, one env per cell")
    p.add_argument("--plant", default=None, help="KEY=V[,...]: the axes that are not fitted (default: every scale 1, delay 0)")
    p.add_argument("--weight", action="append", default=None, help=f"CHANNEL=W, repeatable; channels: {', '.join(CHANNELS)}")
    p.add_argument("--generations", type=int, default=DEFAULT_GENERATIONS)
    p.add_argument("--num_envs", type=int, default=DEFAULT_FIT_ENVS, help="candidates per generation of --fit")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--output", default=None, help="fit.json")
    p.add_argument("--save_obs", default=None, help="the best candidate's simulated rows, in the log's format")
    p.add_argument("--synthesize", default=None, help="write a log recorded on --plant instead of fitting one")
    p.add_argument("--excitation", type=int, default=60, help="--synthesize: control steps of the built-in excitation")
    p.add_argument("--actions", default=None, help="--synthesize: an .npy / .npz (`actions`) of [steps, nu] actions instead of the excitation")
    return p


def check_args(args) -> Dict:
    """Everything the command line can be refused for before a batch exists (SystemExit with the reason); returns the parsed pieces."""
    try:
        if args.fit and args.fit_grid:
            raise ValueError("--fit and --fit_grid exclude each other: a box to search, or a grid to score")
        base = replay_plant(args.plant)
        out = dict(base=base, fit=parse_fit(args.fit) if args.fit else None, grid=parse_fit_grid(args.fit_grid, base) if args.fit_grid else None)
        if args.synthesize:
            if args.fit or args.fit_grid:
                raise ValueError("--synthesize records a log; it does not combine with --fit / --fit_grid")
            if int(args.excitation) < 1:
                raise ValueError("--excitation is a number of control steps >= 1")
        else:
            if not args.log:
                raise ValueError("give a --log to fit (or --synthesize to record one)")
            if not (args.fit or args.fit_grid):
                raise ValueError("give --fit AXIS=LO:HI or --fit_grid AXIS=a:b:n")
            if args.fit and (int(args.generations) < 1 or int(args.num_envs) < 2 * ELITE_SHARE):
                raise ValueError(f"--fit needs --generations >= 1 and --num_envs >= {2 * ELITE_SHARE}")
        parse_weights(args.weight, 1.0)
        return out
    except ValueError as err:
        raise SystemExit(str(err))


FIT_KEYS = ("settings", "best_plant", "best_plant_values", "best_score", "best_lasted", "score_history", "identifiability_hint", "joints",
            "channels", "fell_share", "inside_training_ranges", "cells")


def run(args, out=sys.stdout) -> Dict:
    parsed = check_args(args)
    base = parsed["base"]
    if args.synthesize:
        actions = None
        if args.actions:
            z = np.load(args.actions, allow_pickle=False)
            actions = np.asarray(z["actions"] if hasattr(z, "files") else z, np.float32)
        rows = record(args.task, args.env, base, actions, int(args.excitation), device=args.device, xml=args.xml, seed=args.seed)
        write_log(args.synthesize, rows)
        print(f"{args.synthesize}: {len(rows)} rows on plant {plant_string(base)}", file=sys.stderr)
        return {"rows": int(len(rows)), "plant": plant_string(base)}
    try:
        rows = read_log(args.log)
    except (ValueError, OSError) as err:
        raise SystemExit(str(err))
    grid = parsed["grid"]
    n = len(grid) if grid else int(args.num_envs)
    try:
        rp = Replayer(rows, args.task, args.env, max(n, 2), args.device, args.xml)
    except ValueError as err:
        raise SystemExit(str(err))
    try:
        dev0 = start_deviation(rows, rp.nu, args.env)
        if dev0 > START_WARN_RAD:
            print(f"warning: the log starts {dev0:.3f} rad from the home pose (largest joint deviation of row 0); a log must begin with the "
                  "robot standing near its home pose", file=sys.stderr)
        weights = parse_weights(args.weight, rp.vel_scale)
        cells, hint, history = None, None, None
        if grid:
            scores, lasted, steps, _, _ = rp.evaluate(plant_columns(grid, rp.n), weights)
            scores, lasted, steps = scores[:n], lasted[:n], steps[:n]
            order = rank_order(scores, lasted, steps)
            cells = [dict(plant=grid[i], score=float(scores[i]) if np.isfinite(scores[i]) else None, lasted=bool(lasted[i]), steps=int(steps[i]))
                     for i in range(n)]
            best = dict(plant=dict(grid[int(order[0])]), score=float(scores[order[0]]), lasted=bool(lasted[order[0]]))
            fell = float((~lasted).mean())
        else:
            def evaluate(cand):
                cols = {k: (cand[k] if k in cand else np.full(rp.n, base[k])) for k in PLANT_AXES}
                return rp.evaluate(cols, weights)[:3]
            res = cem(evaluate, parsed["fit"], rp.n, int(args.generations), int(args.seed))
            best = dict(plant=dict(base, **res["best"]["plant"]), score=res["best"]["score"], lasted=res["best"]["lasted"])
            history, fell = res["history"], res["fell_share"]
            hint = dict(note="the elites' mean and std of the last generation: how sharply the log pins each axis down, NOT a confidence interval",
                        elite_mean=res["elite_mean"], elite_std=res["elite_std"], delay_shares=res["delay_shares"])
        nominal = dict(base, **{a: 1.0 for a in PLANT_SCALE_AXES})
        acc, track, sim = rp.run(plant_columns([best["plant"], nominal], rp.n), trace=0)
        names = [str(s) for s in rp.batch.model.a["names_actuator"]][:rp.nu]
        means = channel_means(acc, rp.nu, rp.vel_scale)
        report = dict(
            settings=dict(log=args.log, rows=int(len(rows)), steps=rp.nrow, task=args.task, env=args.env, num_envs=rp.n, fit=args.fit, fit_grid=args.fit_grid,
                          plant=args.plant, weights=weights, generations=int(args.generations) if args.fit else None, seed=int(args.seed),
                          start_deviation_rad=dev0, search="cross-entropy method" if args.fit else "grid"),
            best_plant=plant_string(best["plant"]), best_plant_values=best["plant"], best_score=best["score"], best_lasted=best["lasted"],
            score_history=history, identifiability_hint=hint,
            joints=dict(best=joint_report(acc[0], rp.nu, rp.vel_scale, names), nominal=joint_report(acc[1], rp.nu, rp.vel_scale, names),
                        nominal_plant=plant_string(nominal)),
            channels={c: dict(best=float(means[c][0]), nominal=float(means[c][1])) for c in CHANNELS},
            fell_share=fell, inside_training_ranges=in_training_ranges(best["plant"]), cells=cells)
        if args.save_obs:
            write_log(args.save_obs, as_logged(rows[0], sim, rp.table_np[:, LOG_ACTION:LOG_ACTION + rp.nu], rp.nu, args.env))
    finally:
        rp.close()
    text = json.dumps(report, indent=1)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text + "\n")
    print(f"best plant: --plant {report['best_plant']}  (score {report['best_score']:.3e})", file=out)
    return report


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
