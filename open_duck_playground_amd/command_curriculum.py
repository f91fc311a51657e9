"""A grid-adaptive command curriculum for training (`runner --command_curriculum`): the flags' parser, the struct the two kernels read
(include/odk.h "Command curriculum"), numpy restatements of `odk_curriculum_step` and `odk_curriculum_update` with their bits, and
`CommandCurriculum`, which a rollout runs behind every env step.  Command space (vx, vy, wz) is split into bins; commands are drawn from the
bins that are open, in proportion to their level, and a bin's axis neighbours open once the policy tracks well inside it.  torch is imported
only where a curriculum is built."""
from __future__ import annotations

import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import actuation
from .engine import (Curriculum, CURR_LMAX, CURR_MAX_AXIS, CURR_MAX_BINS, CURR_NSTATE, CURR_HEAD, CURR_EPISODE, CURR_STINT, CURR_STEP, CURR_BIN,
                     CURR_SAMPLES, CURR_SQLIN, CURR_SQYAW, CURR_STAT_UPDATES, CURR_STAT_JUDGED, CURR_STAT_PROMOTED, CURR_STAT_TRIES, CURR_STREAM0,
                     NCOMMAND, curriculum_nbins)      # ODK_CURR_*

GRID_FLAG, START_FLAG = "--command_curriculum", "--curriculum_start"
AXES = ("vx", "vy", "wz")
CONFIG_KEYS = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw")      # the env config's range of each axis
TABLE_KEYS = ("dx_range", "dy_range", "dtheta_range")        # the reference-motion table's
OBS_COMMAND = 6                                              # the command's first column in both observation rows (odk_obs_layout.h)
PRIV_LINVEL, PRIV_GYRO_Z = 9, 2                              # offsets into the privileged tail (priv_at::LOCAL_LINVEL, priv_at::GYRO + 2)
# p_zero and period are the reference's (joystick.py:457-461, 671-725).  BUILD-DEFINED controller settings: LMAX, skip, min_samples, min_tries,
# promote_rate.  tol_lin / tol_yaw are measured: the upper quartile over the 27 cells of `track --grid vx=-0.15:0.15:3,vy=-0.2:0.2:3,
# wz=-1:1:3` of a nominal 150 M-step flat_terrain checkpoint's planar and yaw RMS errors, rounded up to two digits
# (profiles/curriculum/NOTES.md)
SETTINGS = dict(period=500, skip=25, min_samples=50, min_tries=16, promote_rate=0.75, tol_lin=0.27, tol_yaw=0.69, p_zero=0.1)
_WHOLE = ("period", "skip", "min_samples", "min_tries")


def _parse_axes(flag: str, text, fields: int) -> Dict[str, Tuple[float, ...]]:
    """`vx=LO:HI:BINS,...` (fields 3) or `vx=LO:HI,...` (fields 2) -> axis -> numbers.  ValueError, naming the flag and the axis, for an
    unknown axis, an axis given twice, a part that is not AXIS=..., the wrong number of fields, anything not finite and LO above HI."""
    shape = "AXIS=LO:HI:BINS" if fields == 3 else "AXIS=LO:HI"
    out: Dict[str, Tuple[float, ...]] = {}
    items = [text] if isinstance(text, str) else list(text or ())
    for item in items:
        for part in str(item).split(","):
            part = part.strip()
            if not part:
                continue
            name, eq, value = part.partition("=")
            name = name.strip()
            if not eq:
                raise ValueError(f"{flag}: {part!r} is not {shape}")
            if name not in AXES:
                raise ValueError(f"{flag}: unknown axis {name!r} (the axes are {', '.join(AXES)})")
            if name in out:
                raise ValueError(f"{flag}: axis {name!r} given twice")
            ends = [e.strip() for e in value.split(":")]
            try:
                if len(ends) != fields:
                    raise ValueError
                nums = tuple(float(e) for e in ends[:2]) + ((int(ends[2]),) if fields == 3 else ())
            except ValueError:
                raise ValueError(f"{flag}: {part!r} is not {shape}") from None
            if not all(np.isfinite(nums[:2])) or nums[0] > nums[1]:
                raise ValueError(f"{flag}: {name}={value} needs finite LO <= HI")
            out[name] = nums
    return out


def curriculum_spec(grid, start=None, env_ranges: Optional[Sequence[Sequence[float]]] = None, table_ranges: Optional[Dict] = None,
                    allow_clipped_reference: bool = False, **settings) -> Dict:
    """The JSON-able spec of a curriculum from `--command_curriculum vx=-0.15:0.222:8,wz=-1.2:1.2:8` (`grid`) and `--curriculum_start
    vx=-0.15:0.15,...` (`start`, default: `env_ranges`).  `env_ranges`: the env config's (lo, hi) of vx, vy, wz (default: joystick.py's);
    an axis the grid does not name keeps it with one bin.  `table_ranges` (axis -> (lo, hi), or None when the imitation reward is off): a
    grid that leaves both the reference-motion table and the env's own range is refused -- beyond the table the imitation reward follows a
    clipped reference -- unless `allow_clipped_reference`, which warns.  `settings`: SETTINGS' keys.  ValueError, by name, for what
    `_parse_axes` refuses, a bin count outside 1 .. 16, more than 4096 bins, a start outside the grid, an empty start (no bin centre inside
    it) and a setting out of range."""
    if env_ranges is None:
        from .joystick import default_config
        env_ranges = [default_config()[k] for k in CONFIG_KEYS]
    env_ranges = [(float(r[0]), float(r[1])) for r in env_ranges]
    given = _parse_axes(GRID_FLAG, grid, 3)
    if not given:
        raise ValueError(f"{GRID_FLAG}: no axis given")
    G: Dict[str, list] = {}
    for a, axis in enumerate(AXES):
        lo, hi, n = given.get(axis, env_ranges[a] + (1,))
        if not 1 <= n <= CURR_MAX_AXIS:
            raise ValueError(f"{GRID_FLAG}: {axis} has {n} bins (1 .. {CURR_MAX_AXIS} per axis)")
        if n > 1 and not lo < hi:
            raise ValueError(f"{GRID_FLAG}: {axis}={lo:g}:{hi:g}:{n} has several bins of no width")
        G[axis] = [lo, hi, int(n)]
    nbins = int(np.prod([G[x][2] for x in AXES]))
    if nbins > CURR_MAX_BINS:
        raise ValueError(f"{GRID_FLAG}: {nbins} bins (at most {CURR_MAX_BINS})")
    if table_ranges is not None:
        for a, axis in enumerate(AXES):
            t_lo, t_hi = (float(v) for v in table_ranges[axis])
            # (the env's own range is not refused: vy = +-0.2 and vx = -0.15 already lie beyond the shipped table in nominal training)
            if G[axis][0] < min(t_lo, env_ranges[a][0]) - 1e-9 or G[axis][1] > max(t_hi, env_ranges[a][1]) + 1e-9:
                text = (f"{GRID_FLAG}: {axis}={G[axis][0]:g}:{G[axis][1]:g} is wider than the reference-motion table, whose {axis} range is "
                        f"{t_lo:g} .. {t_hi:g}: beyond it the imitation reward follows a clipped reference")
                if not allow_clipped_reference:
                    raise ValueError(text + " (--curriculum_allow_clipped_reference trains on it all the same)")
                warnings.warn(text)
    begun = _parse_axes(START_FLAG, start, 2)
    S: Dict[str, list] = {}
    for a, axis in enumerate(AXES):
        lo, hi = begun.get(axis, env_ranges[a])
        if axis not in begun:      # the env's own range, as far as the grid holds it
            lo, hi = max(lo, G[axis][0]), min(hi, G[axis][1])
        elif lo < G[axis][0] or hi > G[axis][1]:
            raise ValueError(f"{START_FLAG}: {axis}={lo:g}:{hi:g} lies outside the grid's {G[axis][0]:g} .. {G[axis][1]:g}")
        S[axis] = [lo, hi]
    out = dict(SETTINGS)
    for k, v in settings.items():
        if k not in SETTINGS:
            raise ValueError(f"curriculum: unknown setting {k!r}")
        if v is not None:
            out[k] = v
    for k in _WHOLE:
        if isinstance(out[k], bool) or int(out[k]) != out[k] or int(out[k]) < (0 if k in ("skip", "min_samples") else 1):
            raise ValueError(f"--curriculum_{k}: {out[k]!r} is not a whole number >= {0 if k in ('skip', 'min_samples') else 1}")
        out[k] = int(out[k])
    for k in ("promote_rate", "p_zero"):
        if not 0.0 <= float(out[k]) <= 1.0:
            raise ValueError(f"--curriculum_{k}: {out[k]!r} is not a share in 0 .. 1")
    for k in ("tol_lin", "tol_yaw"):
        if not (np.isfinite(float(out[k])) and float(out[k]) >= 0.0):
            raise ValueError(f"--curriculum_{k}: {out[k]!r} is not a finite tolerance >= 0")
    spec = dict(grid=G, start=S, lmax=CURR_LMAX, **{k: (out[k] if k in _WHOLE else float(out[k])) for k in SETTINGS})
    if not initial_levels(spec).any():
        raise ValueError(f"{START_FLAG}: the start is empty: no bin's centre lies inside "
                         + ", ".join(f"{x}={S[x][0]:g}:{S[x][1]:g}" for x in AXES))
    return spec


def bin_edges(spec: Dict) -> Dict[str, list]:
    """axis -> the n + 1 edges of its bins."""
    return {x: np.linspace(spec["grid"][x][0], spec["grid"][x][1], spec["grid"][x][2] + 1).tolist() for x in AXES}


def grid_shape(spec: Dict) -> Tuple[int, int, int]:
    return tuple(int(spec["grid"][x][2]) for x in AXES)


def initial_levels(spec: Dict) -> np.ndarray:
    """int32 [nbins]: CURR_LMAX in exactly the bins whose centre lies inside the start range on every axis, 0 in the others."""
    inside = []
    for x in AXES:
        e = np.asarray(bin_edges(spec)[x])
        centre = 0.5 * (e[:-1] + e[1:])
        inside.append((centre >= spec["start"][x][0]) & (centre <= spec["start"][x][1]))
    open_ = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    return np.where(open_, CURR_LMAX, 0).astype(np.int32).reshape(-1)


def curriculum_struct(spec: Dict, head_ranges: Sequence[Sequence[float]], seed: int = 0, env_id_offset: int = 0) -> Curriculum:
    """The `engine.Curriculum` (odk_curriculum) of a spec.  `head_ranges`: the batch config's cmd_range rows 3..6.  width is the float32
    quotient (hi - lo) / n of the float32 ends: the one division, made here."""
    c = Curriculum()
    for a, x in enumerate(AXES):
        lo, hi, n = spec["grid"][x]
        c.lo[a], c.hi[a], c.n[a] = lo, hi, n
        c.width[a] = (np.float32(c.hi[a]) - np.float32(c.lo[a])) / np.float32(n)
    for j in range(4):
        c.head_lo[j], c.head_hi[j] = float(head_ranges[j][0]), float(head_ranges[j][1])
    for k in SETTINGS:
        setattr(c, k, spec[k])
    c.seed, c.env_id_offset = int(seed) & 0xFFFFFFFF, int(env_id_offset) & 0xFFFFFFFF
    return c


def curriculum_step_reference(cur: Curriculum, nobs: int, priv: np.ndarray, done: Optional[np.ndarray], truncation: Optional[np.ndarray],
                              cdf: np.ndarray, counts: np.ndarray, state: np.ndarray, cmd: np.ndarray, obs: Optional[np.ndarray] = None,
                              patch_priv: bool = True) -> np.ndarray:
    """`odk_curriculum_step` restated in numpy float32, bit for bit: advances `state` ([n, CURR_NSTATE] float32), adds the judged stints to
    `counts` ([nbins, 2] int32) and stores the drawn rows into `cmd` ([n, 7]) and columns 6 .. 12 of `obs` (or None) and, with `patch_priv`,
    of `priv` ([n, npriv]), all in place; returns the [n] mask of the envs that drew.  `done` / `truncation`: [n] or None.  Every operation
    is one float32 operation of the kernel's, in its order; the counters are integers, so the order of the envs does not matter.  Counts
    beyond 2^24 are not restated."""
    f = np.float32
    S, n = state, state.shape[0]
    nbins = curriculum_nbins(cur)
    assert S.dtype == np.float32 and S.shape == (n, CURR_NSTATE) and cmd.dtype == np.float32 and cmd.shape == (n, NCOMMAND)
    assert priv.dtype == np.float32 and priv.shape[0] == n and cdf.dtype == np.int32 and cdf.shape == (nbins,)
    assert counts.dtype == np.int32 and counts.shape == (nbins, 2) and (obs is None or (obs.dtype == np.float32 and obs.shape == (n, nobs)))
    head0, ep0, stint0, step0, bin0, samp0, sql0, sqy0 = (S[:, k].copy() for k in range(CURR_NSTATE))
    d = np.zeros(n, f) if done is None else np.asarray(done, f)
    tr = np.zeros(n, f) if truncation is None else np.asarray(truncation, f)
    one = f(1)
    with np.errstate(all="ignore"):
        ex, ey = priv[:, nobs + PRIV_LINVEL] - cmd[:, 0], priv[:, nobs + PRIV_LINVEL + 1] - cmd[:, 1]
        ez = priv[:, nobs + PRIV_GYRO_Z] - cmd[:, 2]
        first = head0 == 0
        ended = ~first & (d != 0)
        sample = ~first & (d == 0) & (step0 >= f(cur.skip))
        samp = np.where(sample, samp0 + one, samp0)
        sql = np.where(sample, sql0 + (ex * ex + ey * ey), sql0)
        sqy = np.where(sample, sqy0 + ez * ez, sqy0)
        step = np.where(first, step0, step0 + one)
        end = ended | (~first & (step == f(cur.period)))
        fall = ended & (tr == 0)
        judged = end & (bin0 >= 0)
        counted = judged & (fall | (samp >= f(cur.min_samples)))
        tol_lin2, tol_yaw2 = f(cur.tol_lin) * f(cur.tol_lin), f(cur.tol_yaw) * f(cur.tol_yaw)
        success = counted & ~fall & (sql <= tol_lin2 * samp) & (sqy <= tol_yaw2 * samp)
        np.add.at(counts[:, 0], bin0[counted].astype(np.int64), 1)
        np.add.at(counts[:, 1], bin0[success].astype(np.int64), 1)
        draw, fresh = first | end, first | ended
        episode, stint = np.where(fresh, ep0 + one, ep0), np.where(fresh, f(0), stint0)
        env = (np.uint32(int(cur.env_id_offset)) + np.arange(n, dtype=np.uint32)).astype(np.uint32)
        u = lambda k: actuation.action_uniform(np.uint32(int(cur.seed)), env, actuation._u32(episode), actuation._u32(stint),
                                               np.uint32(CURR_STREAM0 + k))
        total = int(cdf[nbins - 1])
        zero = (u(0) < f(cur.p_zero)) | (total <= 0)
        t = np.minimum((u(1) * f(total)).astype(np.int32), np.int32(total - 1))
        b = np.minimum(np.searchsorted(cdf, t, side="right"), nbins - 1).astype(np.int64)      # the first bin with cdf[bin] > t
        n1, n2 = int(cur.n[1]), int(cur.n[2])
        index = (b // (n1 * n2), (b // n2) % n1, b % n2)
        row = np.zeros((n, NCOMMAND), f)
        for a in range(3):
            row[:, a] = np.fmin(f(cur.lo[a]) + f(cur.width[a]) * (index[a].astype(f) + u(2 + a)), f(cur.hi[a]))
        for j in range(4):
            row[:, 3 + j] = f(cur.head_lo[j]) + (f(cur.head_hi[j]) - f(cur.head_lo[j])) * u(5 + j)
        row[zero] = 0
        drawn_bin = np.where(zero, f(-1), b.astype(f))
    zeros = np.zeros(n, f)
    S[:, CURR_HEAD] = head0 + one
    S[:, CURR_EPISODE], S[:, CURR_STINT] = np.where(draw, episode, ep0), np.where(draw, stint + one, stint0)
    S[:, CURR_STEP], S[:, CURR_BIN] = np.where(draw, zeros, step), np.where(draw, drawn_bin, bin0)
    S[:, CURR_SAMPLES], S[:, CURR_SQLIN], S[:, CURR_SQYAW] = np.where(draw, zeros, samp), np.where(draw, zeros, sql), np.where(draw, zeros, sqy)
    cmd[draw] = row[draw]
    if obs is not None:
        obs[draw, OBS_COMMAND:OBS_COMMAND + NCOMMAND] = row[draw]
    if patch_priv:
        priv[draw, OBS_COMMAND:OBS_COMMAND + NCOMMAND] = row[draw]
    return draw


def curriculum_update_reference(cur: Curriculum, levels: np.ndarray, cdf: np.ndarray, counts: np.ndarray, stats: np.ndarray) -> None:
    """`odk_curriculum_update` restated in numpy, bit for bit (all integers but the promotion test, which is the kernel's float32 product
    and comparison): `levels`, `cdf` ([nbins] int32), `counts` ([nbins, 2] int32) and `stats` ([4] int32) advance in place.  Every level is
    computed from the counters and levels as they were before the call."""
    f = np.float32
    nbins, shape = curriculum_nbins(cur), tuple(int(v) for v in cur.n)
    assert all(a.dtype == np.int32 for a in (levels, cdf, counts, stats))
    assert levels.shape == cdf.shape == (nbins,) and counts.shape == (nbins, 2) and stats.shape == (4,)
    tries, wins = counts[:, 0].copy(), counts[:, 1].copy()
    judged = tries >= int(cur.min_tries)
    promoted = judged & (wins.astype(f) >= f(cur.promote_rate) * tries.astype(f))
    p = promoted.reshape(shape).astype(np.int32)
    P = p.copy()
    for a in range(3):      # the neighbour one step down and one step up each axis; the grid does not wrap
        lower, upper = [slice(None)] * 3, [slice(None)] * 3
        lower[a], upper[a] = slice(0, -1), slice(1, None)
        P[tuple(upper)] += p[tuple(lower)]
        P[tuple(lower)] += p[tuple(upper)]
    levels[:] = np.minimum(CURR_LMAX, levels + P.reshape(-1))
    counts[judged] = 0
    cdf[:] = np.cumsum(levels, dtype=np.int64).astype(np.int32)
    stats[CURR_STAT_UPDATES] += 1
    stats[CURR_STAT_JUDGED] += int(judged.sum())
    stats[CURR_STAT_PROMOTED] += int(promoted.sum())
    stats[CURR_STAT_TRIES] += int(tries[judged].sum())


def env_command_ranges(env) -> list:
    """The (lo, hi) of vx, vy, wz an env samples its commands from: its config's keys, else the batch config's cmd_range rows 0..2."""
    cfg = getattr(env, "_config", None)
    if cfg is not None and all(k in cfg for k in CONFIG_KEYS):
        return [(float(cfg[k][0]), float(cfg[k][1])) for k in CONFIG_KEYS]
    return [(float(env.batch.cfg.cmd_range[a][0]), float(env.batch.cfg.cmd_range[a][1])) for a in range(3)]


def table_command_ranges(env) -> Optional[Dict]:
    """axis -> (lo, hi) of the reference-motion table an env's imitation reward reads, None when that reward is off."""
    if not int(env.batch.cfg.use_imitation):
        return None
    motion = getattr(env, "reference_motion", None)
    if motion is None:
        from .reference_motion import ReferenceMotion
        motion = ReferenceMotion.from_npz()
    return {x: tuple(float(v) for v in getattr(motion, k)) for x, k in zip(AXES, TABLE_KEYS)}


def settings_from_args(args) -> Dict:
    """The `--curriculum_*` settings a command line gives (None: the default)."""
    return {k: getattr(args, "curriculum_" + k, None) for k in SETTINGS}


def spec_from_args(args, env=None) -> Optional[Dict]:
    """The spec the command line asks for, None without `--command_curriculum`.  Without `env` the ranges are joystick.py's defaults and the
    reference-motion table is not looked at (the check of the flags before any GPU set-up); ValueError as `curriculum_spec`'s, and for a
    `--curriculum_*` flag without the grid."""
    grid = getattr(args, "command_curriculum", None)
    if not grid:
        extra = [k for k, v in settings_from_args(args).items() if v is not None]
        if getattr(args, "curriculum_start", None) or extra or getattr(args, "curriculum_allow_clipped_reference", False):
            raise ValueError(f"--curriculum_* flags need {GRID_FLAG}")
        return None
    return curriculum_spec(grid, getattr(args, "curriculum_start", None), None if env is None else env_command_ranges(env),
                           None if env is None else table_command_ranges(env),
                           bool(getattr(args, "curriculum_allow_clipped_reference", False)), **settings_from_args(args))


class CommandCurriculum:
    """The curriculum of one training env: owns the command buffer (bound with `env.set_commands`), levels, cdf, counts, stats and the per-env
    state; fixed addresses, nothing allocated after construction.  `reset(state)` after every reset of the env, `after_step(state)` after
    every step of a rollout, `update(group)` once per training iteration.  `spec`: a `curriculum_spec`; `seed`: the run's; the env's own
    `env_id_offset` separates the ranks' draws."""

    def __init__(self, env, spec: Dict, seed: int = 0):
        import torch
        b = self.batch = env.batch
        self.spec, self.seed = spec, int(seed) & 0xFFFFFFFF
        head = [(float(b.cfg.cmd_range[3 + j][0]), float(b.cfg.cmd_range[3 + j][1])) for j in range(4)]
        self.cur = curriculum_struct(spec, head, self.seed, int(getattr(env, "env_id_offset", 0)))
        self.nbins = curriculum_nbins(self.cur)
        dev = torch.device("cuda", b.device)
        I = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        levels = initial_levels(spec)
        self.levels = torch.from_numpy(levels).to(dev)
        self.cdf = torch.from_numpy(np.cumsum(levels, dtype=np.int64).astype(np.int32)).to(dev)
        self.counts, self.stats = I(self.nbins, 2), I(4)
        self.state = torch.zeros(b.nenv, CURR_NSTATE, dtype=torch.float32, device=dev)
        self.commands = torch.zeros(b.nenv, NCOMMAND, dtype=torch.float32, device=dev)
        env.set_commands(self.commands)

    def reset(self, state) -> None:
        """After every reset of the env: the per-env state is zeroed and every env draws; the reset's observation shows its command."""
        self.state.zero_()
        self.batch.curriculum_step(self.cur, state.obs["privileged_state"], None, None, self.cdf, self.counts, self.state, self.commands,
                                   obs=state.obs["state"])

    def after_step(self, state) -> None:
        """After every env step: the step's sample, the judgement of the stints that end, their next commands."""
        self.batch.curriculum_step(self.cur, state.obs["privileged_state"], state.done, state.info["truncation"], self.cdf, self.counts,
                                   self.state, self.commands, obs=state.obs["state"])

    def update(self, group=None) -> None:
        """Once per training iteration: with a process group the ranks' counters are summed first, so every rank holds the same levels."""
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(self.counts, group=group)
        self.batch.curriculum_update(self.cur, self.levels, self.cdf, self.counts, self.stats)

    def metrics(self) -> Dict[str, float]:
        """coverage: the share of bins that are open; mean_level: over all bins; promotions: bins promoted so far (synchronises)."""
        levels, stats = self.levels.cpu().numpy(), self.stats.cpu().numpy()
        return dict(coverage=float((levels > 0).mean()), mean_level=float(levels.mean()), promotions=int(stats[CURR_STAT_PROMOTED]))

    def describe(self) -> Dict:
        """JSON-able: the spec, the levels as a nested [n_vx][n_vy][n_wz] list, the bin edges, coverage and mean level -- what a checkpoint
        stores as `command_curriculum` and `track` reports as `trained_with_curriculum`."""
        m = self.metrics()
        stats = self.stats.cpu().numpy()
        return dict(spec=self.spec, seed=self.seed, levels=self.levels.cpu().numpy().reshape(grid_shape(self.spec)).tolist(),
                    edges=bin_edges(self.spec), coverage=m["coverage"], mean_level=m["mean_level"],
                    stats=dict(updates=int(stats[CURR_STAT_UPDATES]), judged=int(stats[CURR_STAT_JUDGED]),
                               promoted=int(stats[CURR_STAT_PROMOTED]), tries=int(stats[CURR_STAT_TRIES])))
