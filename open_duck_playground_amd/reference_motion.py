"""Reference motions of the imitation reward (reference playground/common/poly_reference_motion.py).

The reference's README trains with the imitation reward by generating a reference motion, copying its
`polynomial_coefficients.pkl` into `playground/<robot>/data/` and turning `USE_IMITATION_REWARD` on.  Here that file is
read by `ReferenceMotion.from_pickle` (for any robot) and handed to the env kernels in the one layout they know: a
`[nx, ny, nth, 40, 16]` table of highest-power-first polynomial coefficients per grid cell.  `imitation_joint_map` says
which actuator is compared with which frame joint (custom_rewards.py:80-88, generalised).

A frame of a motion with J joints has D = 2J + 8 dims (poly_reference_motion.py:6-51): joint positions (J), joint
velocities (J), foot contacts (2), base linear velocity (3), base angular velocity (3).  In the canonical table frame joint
j sits on rows j and 16 + j, the contacts and velocities on rows 32-39, and unused joint rows are zero.  Polynomials of fewer
than 16 coefficients get leading zeros (Horner's `fma(0, t, c) = c` is exact).
"""
from __future__ import annotations

import hashlib
import io
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_JOINTS = 16          # frame joints the canonical table holds
MAX_COEFFS = 16          # polynomial coefficients per dim
MAX_GRID = 16            # grid points per axis (odk_batch_create)
NROWS = 40

# poly_reference_motion.py:6-22: the duck's frame joints, antennas included
DUCK_FRAME_JOINTS = ("left_hip_yaw", "left_hip_roll", "left_hip_pitch", "left_knee", "left_ankle", "neck_pitch", "head_pitch", "head_yaw",
                     "head_roll", "left_antenna", "right_antenna", "right_hip_yaw", "right_hip_roll", "right_hip_pitch", "right_knee", "right_ankle")
# frame joints of the duck that no actuator of the duck's models drives (custom_rewards.py:80-88 drops them with the head)
DUCK_UNDRIVEN = ("left_antenna", "right_antenna")


def _allowed_globals() -> Dict:
    """What a pickle of numpy scalars / arrays needs to rebuild them, under numpy 1's (`numpy.core`) and numpy 2's (`numpy._core`) module
    names; resolved here without importing anything the pickle names."""
    try:
        from numpy._core import multiarray as ma, numeric as nm
    except ImportError:      # numpy < 2
        from numpy.core import multiarray as ma, numeric as nm
    out = {("numpy", "dtype"): np.dtype, ("numpy", "ndarray"): np.ndarray}
    for mod in ("numpy.core", "numpy._core"):
        out[(mod + ".multiarray", "scalar")] = ma.scalar
        out[(mod + ".multiarray", "_reconstruct")] = ma._reconstruct
        if hasattr(nm, "_frombuffer"):
            out[(mod + ".numeric", "_frombuffer")] = nm._frombuffer
    return out


class _SafeUnpickler(pickle.Unpickler):
    """Only numpy's scalar, dtype and ndarray reconstruction; any other global is refused before it is looked up or called."""

    _ALLOWED = None

    def find_class(self, module, name):
        if _SafeUnpickler._ALLOWED is None:
            _SafeUnpickler._ALLOWED = _allowed_globals()
        fn = _SafeUnpickler._ALLOWED.get((module, name))
        if fn is None:
            raise pickle.UnpicklingError(f"reference motion: the pickle names {module}.{name}, which is not a numpy scalar / array "
                                         "reconstructor (refused)")
        return fn


def safe_load(raw: bytes):
    return _SafeUnpickler(io.BytesIO(raw)).load()


def canonical_row(f: int, J: int) -> int:
    """Row of the canonical [.., 40, 16] table that frame dim f (of a J-joint frame) goes to."""
    if f < J:
        return f
    if f < 2 * J:
        return 16 + f - J
    return 32 + f - 2 * J


class ReferenceMotion:
    """A polynomial reference motion in the kernels' canonical layout.  Attributes: `dxs`, `dys`, `dthetas` (sorted float64 grids),
    `dx_range`, `dy_range`, `dtheta_range`, `period`, `fps`, `nb_steps_in_period`, `n_joints` (J), `n_dims` (D = 2J + 8),
    `n_coeffs` (per polynomial in the source), `table64` ([nx, ny, nth, 40, 16] float64, highest power first), `sha256` (of the source
    file), `path`."""

    def __init__(self, table64, dxs, dys, dthetas, ranges, period, fps, nb_steps_in_period, n_joints, n_coeffs, sha256, path=None):
        self.table64 = np.ascontiguousarray(table64, np.float64)
        self.dxs, self.dys, self.dthetas = (np.asarray(v, np.float64) for v in (dxs, dys, dthetas))
        self.dx_range, self.dy_range, self.dtheta_range = (np.asarray(r, np.float64) for r in ranges)
        self.period, self.fps = period, fps
        self.nb_steps_in_period = int(nb_steps_in_period)
        self.n_joints, self.n_dims, self.n_coeffs = int(n_joints), 2 * int(n_joints) + 8, int(n_coeffs)
        self.sha256, self.path = str(sha256), path
        if self.nb_steps_in_period < 1:
            raise ValueError(f"reference motion: nb_steps_in_period = int(period * fps) = {self.nb_steps_in_period} (period {period}, fps {fps}): "
                             "it must be >= 1")

    @property
    def table(self) -> np.ndarray:
        return self.table64.astype(np.float32)

    # ---- loaders
    @classmethod
    def from_pickle(cls, path: str) -> "ReferenceMotion":
        """Reads a `polynomial_coefficients.pkl` as PolyReferenceMotion.process (poly_reference_motion.py:74-144) does; ValueError
        names what is outside the kernels' limits."""
        with open(path, "rb") as f:
            raw = f.read()
        return cls.from_bytes(raw, path=str(path))

    @classmethod
    def from_bytes(cls, raw: bytes, path: Optional[str] = None) -> "ReferenceMotion":
        data = safe_load(raw)
        if not isinstance(data, dict) or not data:
            raise ValueError("reference motion: expected a non-empty dict of '<dx>_<dy>_<dtheta>' entries")
        dxs: List[float] = []; dys: List[float] = []; dths: List[float] = []
        rx, ry, rt = [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]      # ranges start at [0, 0] and widen (poly_reference_motion.py:58-60,101-106)
        period = fps = None
        nsteps = None
        cells: Dict = {}
        D = K = None
        for name, entry in data.items():
            parts = str(name).split("_")
            if len(parts) != 3:
                raise ValueError(f"reference motion: key {name!r} is not '<dx>_<dy>_<dtheta>'")
            dx, dy, dth = (float(p) for p in parts)
            if period is None:       # the first entry's period and fps (poly_reference_motion.py:85-93), int(period * fps) in float64
                period, fps = entry["period"], entry["fps"]
                nsteps = int(period * fps)
            for v, grid in ((dx, dxs), (dy, dys), (dth, dths)):
                if v not in grid:
                    grid.append(v)
            rx = [min(dx, rx[0]), max(dx, rx[1])]
            ry = [min(dy, ry[0]), max(dy, ry[1])]
            rt = [min(dth, rt[0]), max(dth, rt[1])]
            coeffs = [np.asarray(v, np.float64).reshape(-1) for v in entry["coefficients"].values()]    # dict order, lowest order first
            d = len(coeffs)
            ks = {len(c) for c in coeffs}
            if len(ks) != 1:
                raise ValueError(f"reference motion: entry {name!r} mixes polynomials of {sorted(ks)} coefficients")
            k = ks.pop()
            if D is None:
                D, K = d, k
                if D % 2 or D < 10:
                    raise ValueError(f"reference motion: a frame of {D} dims; expected 2J + 8 (joint positions, joint velocities, 2 foot "
                                     "contacts, base linear and angular velocity): an even number >= 10")
                if (D - 8) // 2 > MAX_JOINTS:
                    raise ValueError(f"reference motion: J = {(D - 8) // 2} joints per frame; the kernels hold at most {MAX_JOINTS}")
                if K > MAX_COEFFS:
                    raise ValueError(f"reference motion: {K} coefficients per polynomial (degree {K - 1}); the kernels hold at most {MAX_COEFFS}")
                if K < 1:
                    raise ValueError("reference motion: polynomials without coefficients")
            elif (d, k) != (D, K):
                raise ValueError(f"reference motion: entry {name!r} has {d} dims of {k} coefficients, the first entry {D} dims of {K}")
            cells[(dx, dy, dth)] = np.stack([np.flip(c) for c in coeffs])      # highest power first (jp.flip)
        dxs, dys, dths = sorted(dxs), sorted(dys), sorted(dths)
        for axis, grid in (("dx", dxs), ("dy", dys), ("dtheta", dths)):
            if len(grid) > MAX_GRID:
                raise ValueError(f"reference motion: {len(grid)} {axis} grid points; the kernels take at most {MAX_GRID} per axis")
        J = (D - 8) // 2
        table = np.zeros((len(dxs), len(dys), len(dths), NROWS, MAX_COEFFS))
        rows = [canonical_row(f, J) for f in range(D)]
        for ix, dx in enumerate(dxs):
            for iy, dy in enumerate(dys):
                for it, dth in enumerate(dths):
                    c = cells.get((dx, dy, dth))
                    if c is None:
                        raise ValueError(f"reference motion: grid cell dx={dx} dy={dy} dtheta={dth} has no entry (the grid must be complete)")
                    if not np.isfinite(c).all():
                        raise ValueError(f"reference motion: cell dx={dx} dy={dy} dtheta={dth} has a coefficient that is not finite")
                    table[ix, iy, it, rows, MAX_COEFFS - K:] = c
        return cls(table, dxs, dys, dths, (rx, ry, rt), period, fps, nsteps, J, K, hashlib.sha256(raw).hexdigest(), path)

    @classmethod
    def from_npz(cls, path: Optional[str] = None) -> "ReferenceMotion":
        """The shipped table (assets/prm_table.npz, converted from the duck's polynomial_coefficients.pkl); `sha256` is its source pickle's."""
        if path is None:
            from .model import asset_path
            path = asset_path("prm_table.npz")
        z = np.load(path)
        return cls(z["table64"], z["dxs"], z["dys"], z["dthetas"], (z["dx_range"], z["dy_range"], z["dtheta_range"]), float(z["period"][0]),
                   int(z["fps"][0]), int(z["nb_steps_in_period"][0]), MAX_JOINTS, MAX_COEFFS, str(z["source_sha256"]), str(path))

    # ---- what the engine takes
    def prm(self) -> Dict[str, np.ndarray]:
        """The dict `engine.Batch(prm=...)` takes (the layout of assets/prm_table.npz)."""
        return dict(table=self.table, table64=self.table64, dxs=self.dxs.copy(), dys=self.dys.copy(), dthetas=self.dthetas.copy(),
                    dx_range=self.dx_range.copy(), dy_range=self.dy_range.copy(), dtheta_range=self.dtheta_range.copy(),
                    nb_steps_in_period=np.array([self.nb_steps_in_period]), period=np.array([self.period]), fps=np.array([self.fps]),
                    source_sha256=np.array(self.sha256))

    def describe(self) -> str:
        return (f"reference motion {self.path}: grid {len(self.dxs)} x {len(self.dys)} x {len(self.dthetas)} (dx x dy x dtheta), "
                f"J = {self.n_joints}, nb_steps_in_period = {self.nb_steps_in_period}, sha256 {self.sha256}")

    # ---- float64 restatement of get_reference_motion (poly_reference_motion.py:148-168)
    def index(self, dx: float, dy: float, dtheta: float):
        """Nearest grid indices after clipping to the ranges; ties go to the first index (argmin)."""
        out = []
        for v, grid, r in ((dx, self.dxs, self.dx_range), (dy, self.dys, self.dy_range), (dtheta, self.dthetas, self.dtheta_range)):
            out.append(int(np.argmin(np.abs(grid - np.clip(float(v), r[0], r[1])))))
        return tuple(out)

    def evaluate(self, dx: float, dy: float, dtheta: float, i: int) -> np.ndarray:
        """The D-dim frame (frame order) at step i of the period, in float64."""
        ix, iy, it = self.index(dx, dy, dtheta)
        n = self.nb_steps_in_period
        t = min(max((int(i) % n) / n, 0.0), 1.0)
        c = self.table64[ix, iy, it]
        return np.array([np.polyval(c[canonical_row(f, self.n_joints)], t) for f in range(self.n_dims)])


def actuated_joint_names(model) -> List[str]:
    """The joint each actuator drives, in actuator order."""
    a = model.a
    jn = [str(n) for n in a["names_jnt"]]
    trn = np.asarray(a["actuator_trnid"]).reshape(model.nu, -1)[:, 0]
    return [jn[int(j)] for j in trn]


def imitation_joint_map(model, motion: ReferenceMotion, joints: Optional[Sequence[str]] = None,
                        ignore: Optional[Sequence[str]] = None) -> List[int]:
    """For each actuator u, the frame index of its joint, or -1 where the imitation reward does not compare that actuator
    (odk_batch_set_imitation_joints).

    `joints`: the names of the motion's J frame joints, in frame order.  Default: the duck's 16 (poly_reference_motion.py:6-22) for the
    duck, the actuated joints in actuator order for another robot (then J must equal the actuator count).  The reward compares the leg
    joints (`constants.robot_of(model).joints_order_no_head`) and leaves every other frame joint out, as custom_rewards.py:80-88 leaves out
    the duck's head and antennas.  `ignore`: frame joints to leave out as well (default: the duck's antennas for the duck, none otherwise).
    ValueError for a name that is not a joint of the model, a frame joint that no actuator drives and that is not in `ignore`, a name given
    twice, or a `joints` list whose length is not J."""
    from . import constants
    robot = constants.robot_of(model)
    J = motion.n_joints
    act = actuated_joint_names(model)
    if joints is None:
        if robot.is_open_duck:
            frame = list(DUCK_FRAME_JOINTS)
            if J != len(frame):
                raise ValueError(f"reference motion: J = {J} frame joints, the duck's frame has {len(frame)} (poly_reference_motion.py:6-22); "
                                 "name them (imitation_joints)")
        else:
            frame = list(act)
            if J != len(frame):
                raise ValueError(f"reference motion: J = {J} frame joints but the robot has nu = {len(frame)} actuators; name the frame's "
                                 "joints (imitation_joints)")
    else:
        frame = [str(n) for n in joints]
        if len(frame) != J:
            raise ValueError(f"imitation_joints: {len(frame)} names, the reference motion has J = {J} frame joints")
    if ignore is None:
        ignore = list(DUCK_UNDRIVEN) if robot.is_open_duck and joints is None else []
    ignore = [str(n) for n in ignore]
    known = {str(n) for n in model.a["names_jnt"]}
    for what, names in (("imitation_joints", frame), ("imitation_ignore", ignore)):
        seen = set()
        for n in names:
            if n in seen:
                raise ValueError(f"{what}: {n!r} given twice")
            seen.add(n)
    for n in ignore:
        if n not in frame:
            raise ValueError(f"imitation_ignore: {n!r} is not one of the frame's joints ({', '.join(frame)})")
    for n in frame:
        if n in ignore:
            continue
        if n not in act:
            if n not in known:
                raise ValueError(f"imitation_joints: {n!r} is not a joint of the model")
            raise ValueError(f"imitation_joints: frame joint {n!r} is driven by no actuator (leave it out with imitation_ignore)")
    compared = set(robot.joints_order_no_head) - set(ignore)
    return [frame.index(n) if (n in compared and n in frame) else -1 for n in act]
