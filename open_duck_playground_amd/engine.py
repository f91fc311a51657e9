"""ctypes binding of libodk.so (include/odk.h): the MI355X-native batched env engine.

This is the host side of the drop-in boundary: it owns no arithmetic.  PyTorch-ROCm is
used for device memory and streams only; every number comes out of the HIP kernels in csrc/.
There is no CPU fallback: importing works without the library, but constructing a `Batch` raises
if `csrc/libodk.so` is missing or no HIP device is visible.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re
import subprocess
from typing import Dict, List, Optional

import numpy as np

from .model import Model, asset_path

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("ODK_LIB", os.path.join(_CSRC, "libodk.so"))  # ODK_LIB: e.g. the -DODK_PROFILE build
POISON_LIB_PATH = os.path.join(_CSRC, "libodk_poison.so")   # the -DODK_POISON_LDS build (csrc/odk_poison.h): load it through ODK_LIB


class OdkError(RuntimeError):
    pass


class OdkValueError(OdkError, ValueError):
    """An argument refused before any launch (`check_action_delays`): an OdkError that `except ValueError` catches too."""


def library_sources() -> list:
    """The files a library in csrc/ is built from (what build_library and the poison tests call stale against)."""
    srcs = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".hip", ".h", ".inc")) or f == "Makefile"]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "odk.h"))
    return srcs


_FLOAT = r"(?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+"
_TOKEN = re.compile(rf"\s*(?:({_FLOAT})f?(?![\w.])|(\d+)(?![\w.])|(ODK_\w+)|([-+*()]))")


def header_constants(text: Optional[str] = None) -> Dict[str, object]:
    """name (without ODK_) -> int or float of every constant include/odk.h (or `text`) gives a value: object-like `#define ODK_NAME body`
    and enum entries `ODK_NAME = body`, in the order they stand.  A body is made of integer and float literals (a trailing f allowed),
    ODK_ names defined before it, + - * and parentheses: all integers give an int, anything else a float.  A define without a body and a
    function-like macro are skipped; a name given a value twice, a name used before its definition, any other character or operator and
    an enum entry without `= value` are an OdkError that names the constant."""
    if text is None:
        path = os.path.normpath(library_sources()[-1])
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise OdkError(f"{path}: cannot read the header ({e.strerror})")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    vals: Dict[str, object] = {}

    def give(name: str, body: str) -> None:
        if name[4:] in vals:
            raise OdkError(f"{name}: given a value twice")
        expr, at = "", 0
        while body[at:].strip():
            m = _TOKEN.match(body, at)
            if not m:
                raise OdkError(f"{name}: cannot read '{body.strip()}' at '{body[at:].strip()}' (literals, earlier ODK_ names, + - * and parentheses only)")
            flt, integer, ref, op = m.groups()
            if ref and ref[4:] not in vals:
                raise OdkError(f"{name}: refers to {ref}, which is not defined before it")
            expr += f"({vals[ref[4:]]!r})" if ref else flt or integer or op
            at = m.end()
        try:
            v = eval(expr, {"__builtins__": {}})       # expr: nothing but the tokens checked above
        except (SyntaxError, TypeError):
            v = None
        if type(v) not in (int, float):
            raise OdkError(f"{name}: '{body.strip()}' is not an expression")
        vals[name[4:]] = v

    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(ODK_\w+)(.*)$|\benum\b[^{;]*\{([^}]*)\}", text, re.M):
        name, body, block = m.groups()
        if name:
            if body.strip() and not body.startswith("("):      # neither `#define ODK_H` nor `#define ODK_LOG_ROW(nu) ...`
                give(name, body)
            continue
        for entry in filter(None, (e.strip() for e in block.split(","))):
            name, eq, body = (s.strip() for s in entry.partition("="))
            if not re.fullmatch(r"ODK_\w+", name) or not body:
                raise OdkError(f"{name or entry}: an enum entry must read `ODK_NAME = value`, got '{entry}'")
            give(name, body)
    return vals


# Every constant of include/odk.h -- sizes, strides, accumulator slots, status codes -- as a module global under its name without ODK_
# (GAIT_NACC, SENSOR_NSTATE, ERR_INVALID ...): the header is their one definition, and a new slot is an enum entry there and nothing else.
_HEADER = header_constants()
globals().update(_HEADER)

# What the header does not say.
NCOMMAND = 7    # lin_vel_x, lin_vel_y, ang_vel_yaw, neck_pitch, head_pitch, head_yaw, head_roll
MLP_HIDDEN = (MLP_H1, MLP_H2, MLP_H3)     # the hidden widths the fused network kernels are built for
MLP_MAX_OUT = 32
CURR_STREAM0 = 128      # draw k of a stint comes from stream CURR_STREAM0 + k of the action stage's hash (the fault rows' end at 127)
METRIC_NAMES = ("reward/tracking_lin_vel", "reward/tracking_ang_vel", "cost/torques", "cost/action_rate", "cost/stand_still",
                "reward/alive", "reward/imitation", "swing_peak")
# reward-library terms of the step kernel (enum odk_xterm): scale keys of reward_config.scales, in column order of Batch.xmetrics;
# each is the function of the same name in reference playground/common/rewards.py (cost_* / reward_*)
XTERM_NAMES = tuple(k[6:].lower() for k in sorted((k for k in _HEADER if k.startswith("XTERM_")), key=_HEADER.get))


class EnvConfig(C.Structure):
    """odk_env_config (include/odk.h) == default_config() of reference joystick.py:49-102."""
    _fields_ = [
        ("ctrl_dt", C.c_float), ("action_scale", C.c_float), ("dof_vel_scale", C.c_float), ("max_motor_velocity", C.c_float),
        ("noise_level", C.c_float), ("noise_gyro", C.c_float), ("noise_accelerometer", C.c_float), ("noise_gravity", C.c_float),
        ("noise_joint_vel", C.c_float),
        ("qpos_noise_scale", C.c_float * 16), ("reward_scales", C.c_float * 7), ("tracking_sigma", C.c_float),
        ("push_enable", C.c_float), ("push_interval_range", C.c_float * 2), ("push_magnitude_range", C.c_float * 2),
        ("cmd_range", (C.c_float * 2) * 7),
        ("use_imitation", C.c_int32), ("use_motor_speed_limits", C.c_int32), ("autoreset", C.c_int32), ("episode_length", C.c_int32),
        ("n_substeps", C.c_int32), ("lanes_per_env", C.c_int32), ("env_kind", C.c_int32), ("reset_base_qvel", C.c_float),
        ("hfield_up_normals_only", C.c_int32),
    ]


class Outputs(C.Structure):
    _fields_ = [("obs_dev", C.c_void_p), ("priv_dev", C.c_void_p), ("reward_dev", C.c_void_p), ("done_dev", C.c_void_p),
                ("truncation_dev", C.c_void_p), ("metrics_dev", C.c_void_p)]


class RewardTerms(C.Structure):
    """odk_reward_terms (include/odk.h): one scale per XTERM_NAMES entry (0 = off) and the terms' parameters."""
    _fields_ = [("scale", C.c_float * NXTERM), ("base_height_target", C.c_float), ("max_foot_height", C.c_float),
                ("air_time_range", C.c_float * 2), ("soft_joint_pos_limit_factor", C.c_float), ("pose_weight", C.c_float * 16)]


class Curriculum(C.Structure):
    """odk_curriculum (include/odk.h "Command curriculum"): the grid over (vx, vy, wz), the head ranges and the controller's settings."""
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("n", C.c_int32 * 3), ("width", C.c_float * 3), ("head_lo", C.c_float * 4),
                ("head_hi", C.c_float * 4), ("p_zero", C.c_float), ("period", C.c_int32), ("skip", C.c_int32), ("min_samples", C.c_int32),
                ("tol_lin", C.c_float), ("tol_yaw", C.c_float), ("min_tries", C.c_int32), ("promote_rate", C.c_float), ("seed", C.c_uint32),
                ("env_id_offset", C.c_uint32)]


class MlpDesc(C.Structure):
    """odk_mlp_desc (include/odk.h)."""
    _fields_ = [("x", C.c_void_p), ("in_mean", C.c_void_p), ("in_std", C.c_void_p), ("wf", C.c_void_p * 4), ("wb", C.c_void_p * 4), ("b", C.c_void_p * 4), ("xp", C.c_void_p), ("h", C.c_void_p * 3),
                ("g", C.c_void_p * 3), ("out", C.c_void_p), ("dout", C.c_void_p), ("doutp", C.c_void_p), ("dz", C.c_void_p * 3),
                ("bias_partial", C.c_void_p * 4), ("n", C.c_int), ("n_in", C.c_int), ("n_out", C.c_int),
                ("row_idx", C.c_void_p), ("cursor", C.c_void_p), ("x_tail", C.c_void_p), ("traj_len", C.c_int), ("n_main", C.c_int), ("n_traj", C.c_int)]


class StepTail(C.Structure):
    """odk_step_tail (include/odk.h)."""
    _fields_ = [("cursor_dev", C.c_void_p), ("loss_partials_dev", C.c_void_p), ("n_loss_partials", C.c_int), ("losses_dev", C.c_void_p)]


class GaeHeadArgs(C.Structure):
    """odk_gae_head_args (include/odk.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("logits", "values", "raw_action", "old_log_prob", "reward", "termination", "truncation", "noise", "row_idx", "cursor",
                                         "dlogits", "dvalues", "losses", "loss_partials", "adv_out", "vs_out", "stats_out")] + \
               [(k, C.c_int) for k in ("B", "T", "action_size", "n_traj", "normalize_advantage")] + \
               [(k, C.c_float) for k in ("gae_lambda", "discount", "clipping_epsilon", "entropy_cost", "grad_scale")]


class GradFinish(C.Structure):
    """odk_grad_finish (include/odk.h)."""
    _fields_ = [("bias_partial", C.c_void_p * 8), ("bias_grad", C.c_void_p * 8), ("width", C.c_int * 8), ("nblk", C.c_int * 8), ("nbias", C.c_int),
                ("sq_partials_dev", C.c_void_p), ("step_counter_dev", C.c_void_p), ("nblocks", C.c_int)]


class WeightTableC(C.Structure):
    """odk_weight_table (include/odk.h)."""
    _fields_ = [("count", C.c_int), ("off", C.c_longlong * 8), ("rows", C.c_int * 8), ("cols", C.c_int * 8), ("fwd_off", C.c_longlong * 8),
                ("bwd_off", C.c_longlong * 8)]


def build_library(force: bool = False, poison: bool = False) -> str:
    """Compiles csrc/ for gfx950 with hipcc (cross-compiles without a GPU): the objects side by side (MAX_JOBS, else the CPU count; 16 at the
    most).  force: everything again; otherwise what make's prerequisites say a newer source needs.  poison: libodk_poison.so (every kernel
    starts from NaN-filled LDS) as a second goal of the same make, so that both libraries' objects share the one job pool."""
    goals = [LIB_PATH] + ([POISON_LIB_PATH] if poison else [])
    newest = max(os.path.getmtime(s) for s in library_sources())
    if not force and all(os.path.exists(g) and os.path.getmtime(g) >= newest for g in goals):
        return LIB_PATH
    try:
        jobs = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:       # unset or not a number
        jobs = os.cpu_count() or 1
    jobs = max(1, min(16, jobs))
    subprocess.check_call(["make", "-C", _CSRC, "-s", f"-j{jobs}"] + (["-B"] if force else []) + ["libodk.so"] + (["libodk_poison.so"] if poison else []))
    return LIB_PATH


_lib = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OdkError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the env engine)")
    # torch first: its wheel carries its own HIP runtime (torch/lib/libamdhip64.so), and the process must end up with ONE
    # runtime -- libodk.so takes torch's device pointers and streams.  Loaded the other way round (dlopen here before any
    # `import torch`, e.g. build() then smoke() in one process), libodk.so pulls /opt/rocm's copy in first and its
    # hipSetDevice then reports "no ROCm-capable device" on a box whose GPU torch drives happily.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _signatures() -> Dict[str, tuple]:
    """name -> (restype, argtypes) of every function include/odk.h declares, each once: what `load_library` binds and `EXPORTED_SYMBOLS`
    lists.  tests/test_abi_host.py holds it to the header's prototypes: names, argument count and kind, return type, and a struct pointer as
    POINTER(its Structure).  P: a device pointer, a stream or an opaque odk_model* / odk_batch*."""
    I, F, LL, P, S = C.c_int, C.c_float, C.c_longlong, C.c_void_p, C.c_char_p
    PP, FP, DP, IP, LP, I32P = (C.POINTER(t) for t in (C.c_void_p, C.c_float, C.c_double, C.c_int, C.c_longlong, C.c_int32))
    CFG, OUTS, TABLE = C.POINTER(EnvConfig), C.POINTER(Outputs), C.POINTER(WeightTableC)
    report = [P, P, P, P, P]                        # batch, priv, done, truncation, track_acc: how every report's accumulate starts
    adam = [P, P, P, P, P, LL, F, F, F, F, F]       # params, grads, m, v, acc, n, lr, b1, b2, eps, max_grad_norm
    packed = adam + [P, LL, P, LL, TABLE, I]        # + the two packed copies with their sizes, the table, norm_blocks
    return {
        "odk_last_error": (S, []),
        "odk_default_config": (None, [CFG]),
        "odk_default_config_standing": (None, [CFG]),
        "odk_obs_sizes": (None, [I, IP, IP]),
        "odk_model_load": (I, [S, C.c_uint64, PP]),
        "odk_model_free": (None, [P]),
        "odk_model_dims": (I, [P, IP, IP, IP, IP]),
        "odk_model_obs_sizes": (I, [P, I, IP, IP]),
        "odk_model_reduced": (I, [P, IP, IP, IP, IP, IP, IP]),
        "odk_model_body_lanes": (I, [P, I, IP, I]),
        "odk_model_env_lds_floats": (I, [P]),
        "odk_model_hot_words": (I, [P, IP, IP]),
        "odk_batch_create": (I, [P, CFG, I, I, FP, DP, I, DP, I, DP, I, DP, I, PP]),
        "odk_batch_destroy": (None, [P]),
        "odk_batch_set_config": (I, [P, CFG]),
        "odk_batch_set_param": (I, [P, I, FP, I]),
        "odk_reset": (I, [P, C.c_uint32, C.c_uint32, OUTS, P]),
        "odk_step": (I, [P, P, OUTS, P]),
        "odk_batch_bind_commands": (I, [P, P, I]),
        "odk_batch_set_reward_terms": (I, [P, C.POINTER(RewardTerms)]),
        "odk_batch_bind_reward_metrics": (I, [P, P]),
        "odk_batch_set_imitation_joints": (I, [P, I32P, I]),
        "odk_batch_set_head_joints": (I, [P, I32P, I]),
        "odk_tracking_accumulate": (I, [P, P, P, P, P, P, P]),
        "odk_batch_bind_pushes": (I, [P, P, I]),
        "odk_batch_bind_action_delays": (I, [P, P, I]),
        "odk_push_accumulate": (I, report + [F, F, P, P]),
        "odk_gait_accumulate": (I, report + [P, P, P]),
        "odk_posture_accumulate": (I, report + [F, P, P]),
        "odk_imitation_accumulate": (I, report + [I, P, P]),
        "odk_command_schedule_apply": (I, [P, P, I, I, P, P, P]),
        "odk_response_accumulate": (I, report + [P, I, I, P, F, F, I, P, P]),
        "odk_fall_row_floats": (I, [P, I]),
        "odk_fall_accumulate": (I, report + [P, F, I, P, I, P]),
        "odk_path_begin": (I, [P, P, P]),
        "odk_path_accumulate": (I, [P, P, P, P, P, I, P, F, P, P]),
        "odk_waypoint_command_apply": (I, [P, P, I, P, P, P, F, F, F, F, P]),
        "odk_sensor_apply": (I, [P, P, P, P, P, P, P]),
        "odk_action_apply": (I, [P, P, P, P, P, P, P]),
        "odk_fault_resample": (I, [P, P, P, C.c_uint32, C.c_uint32, P, P, P, P]),
        "odk_curriculum_step": (I, [P, C.POINTER(Curriculum), P, P, P, P, P, P, P, P, P, P]),
        "odk_curriculum_update": (I, [P, C.POINTER(Curriculum), P, P, P, P, P]),
        "odk_log_apply": (I, [P, P, I, P, P, P]),
        "odk_replay_accumulate": (I, report + [P, I, P, P]),
        "odk_physics_step": (I, [P, P, I, P]),
        "odk_batch_get_state": (I, [P, FP, FP, FP]),
        "odk_batch_set_state": (I, [P, FP, FP, FP]),
        "odk_batch_get_debug": (I, [P, FP, FP, FP, FP]),
        "odk_set_debug_dump": (None, [I]),
        "odk_batch_lds_size": (I, [P]),
        "odk_batch_get_lds": (I, [P, FP]),
        "odk_lds_offset": (I, [P, S]),
        "odk_batch_lanes": (I, [P]),
        "odk_batch_record_size": (I, [P]),
        "odk_batch_get_records": (I, [P, FP]),
        "odk_batch_set_records": (I, [P, FP]),
        "odk_record_field": (I, [P, S, IP, IP, IP]),
        "odk_gae": (I, [P, P, P, P, P, P, P, P, I, I, F, F, P]),
        "odk_ppo_head": (I, [P] * 11 + [I, I, F, F, F, P]),
        "odk_policy_sample": (I, [P, P, P, P, P, I, I, P]),
        "odk_adam_clip": (I, adam + [P]),
        "odk_silu_bwd_colsum": (I, [P, P, P, P, P, I, I, P]),
        "odk_colsum_partial": (I, [P, P, I, I, P]),
        "odk_colsum_finalize": (I, [PP, PP, IP, I, I, P]),
        "odk_dw_gemm": (I, [PP, PP, IP, IP, LP, I, IP, I, P, LL, P, C.POINTER(GradFinish), P]),
        "odk_mlp_forward": (I, [C.POINTER(MlpDesc), I, P]),
        "odk_mlp_backward": (I, [C.POINTER(MlpDesc), I, P]),
        "odk_dw_set_profile": (None, [P]),
        "odk_mlp_set_profile": (None, [P]),
        "odk_mlp_set_wg_profile": (None, [P]),
        "odk_pack_weights": (I, [P, LL, P, LL, P, LL, TABLE, P]),
        "odk_adam_clip_packed": (I, packed + [P]),
        "odk_adam_clip_packed_tail": (I, packed + [C.POINTER(StepTail), P]),
        "odk_ppo_gae_head": (I, [C.POINTER(GaeHeadArgs), P]),
        "odk_col_moments": (I, [P, LL, I, I, P, P]),
        "odk_moments_update": (I, [P, I, I, LL, P, P, P, P, F, F, P]),
        "odk_colsum_fold": (I, [PP, PP, IP, IP, I, P]),
        "odk_gather_rows": (I, [PP, PP, IP, LP, I, P, I, LL, P]),
        "odk_batch_timing": (I, [P, I, FP, IP]),
    }


SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def _check_placement(name: str, t, dtype, device: int) -> None:
    """What every tensor argument's check ends with: the dtype, contiguous, on cuda:`device`."""
    if t.dtype != dtype:
        raise OdkError(f"{name}: dtype must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise OdkError(f"{name}: the tensor must be contiguous")
    if t.device.type != "cuda" or t.device.index != int(device):
        raise OdkError(f"{name}: the tensor must live on cuda:{device} (the env's device), got {t.device}")


def _check_tensor(name: str, t, dtype: str, device: int, want: str, shape_ok, or_none: str = "") -> None:
    """What every `check_*` of a tensor argument does, in this order: a tensor at all, `shape_ok(tuple(t.shape))` (`want` says the shape in
    words), then `_check_placement` with torch's `dtype`."""
    import torch
    if not torch.is_tensor(t):
        raise OdkError(f"{name}: expected a torch tensor{or_none}, got {type(t).__name__}")
    if not shape_ok(tuple(t.shape)):
        raise OdkError(f"{name}: shape must be {want}, got {tuple(t.shape)}")
    _check_placement(name, t, getattr(torch, dtype), device)


def check_commands(cmd, nenv: int, device: int) -> None:
    """What `Batch.bind_commands` accepts: a contiguous float32 [nenv, 7] tensor on cuda:`device`; raises OdkError otherwise."""
    _check_tensor("commands", cmd, "float32", device, f"({nenv}, {NCOMMAND})", lambda s: s == (int(nenv), NCOMMAND), " or None")


def sensor_fault_rows(n: int) -> np.ndarray:
    """[n, SENSOR_NPRM] float32 all-nominal fault rows to fill in: the identity rotation, both scales 1, zeros elsewhere.  `odk_sensor_apply`
    hands back the input's bits under such a row."""
    rows = np.zeros((int(n), SENSOR_NPRM), np.float32)
    rows[:, SENSOR_IMU_ROT:SENSOR_IMU_ROT + 9] = np.eye(3, dtype=np.float32).reshape(9)
    rows[:, SENSOR_GYRO_SCALE] = rows[:, SENSOR_ACC_SCALE] = 1.0
    return rows


def action_fault_rows(n: int) -> np.ndarray:
    """[n, ACT_NPRM] float32 all-nominal fault rows to fill in: gain 1, a loss run of 1, no actuator ever frozen (-1), zeros elsewhere.
    `odk_action_apply` hands back the input's bits under such a row."""
    rows = np.zeros((int(n), ACT_NPRM), np.float32)
    rows[:, ACT_GAIN] = rows[:, ACT_DROP_LEN] = 1.0
    rows[:, ACT_FREEZE_AT:ACT_FREEZE_AT + 16] = -1.0
    return rows


def curriculum_nbins(cur) -> int:
    """The bin count of a `Curriculum`; OdkError, by name, for an axis outside 1 .. CURR_MAX_AXIS bins or more than CURR_MAX_BINS bins."""
    n = [int(v) for v in cur.n]
    for a, v in enumerate(n):
        if not 1 <= v <= CURR_MAX_AXIS:
            raise OdkError(f"curriculum: n[{a}] = {v} (1 .. {CURR_MAX_AXIS} bins per axis)")
    if n[0] * n[1] * n[2] > CURR_MAX_BINS:
        raise OdkError(f"curriculum: nbins = {n[0] * n[1] * n[2]} (at most {CURR_MAX_BINS})")
    return n[0] * n[1] * n[2]


def log_row(nu: int) -> int:
    """ODK_LOG_ROW(nu): the floats of a row of the replay table."""
    return 15 + 3 * int(nu)


def log_offsets(nu: int) -> Dict[str, int]:
    """Where the fields of a table row start (include/odk.h "Log replay")."""
    nu = int(nu)
    return {"command": LOG_COMMAND, "action": LOG_ACTION, "pos": 7 + nu, "vel": 7 + 2 * nu, "gyro": 7 + 3 * nu, "accel": 10 + 3 * nu,
            "contact": 13 + 3 * nu}


def check_log_table(name: str, log, nu: int, device: int) -> int:
    """The table argument of `Batch.log_apply` / `Batch.replay_accumulate`: a contiguous float32 [nrow >= 1, log_row(nu)] tensor on
    cuda:`device`; OdkError otherwise.  Returns nrow."""
    _check_tensor(f"{name}: log", log, "float32", device, f"(nrow >= 1, {log_row(nu)})", lambda s: len(s) == 2 and s[0] >= 1 and s[1] == log_row(nu))
    return int(log.shape[0])


def sensor_rotation(roll_deg: float, pitch_deg: float, yaw_deg: float) -> np.ndarray:
    """The float32 [3, 3] mounting rotation of an IMU tilted by roll (about x), pitch (about y) and yaw (about z), in degrees:
    R = Rx(roll)^T Ry(pitch)^T Rz(yaw)^T = (Rz Ry Rx)^T, the matrix that takes a base-frame vector into the frame of a sensor whose axes are
    the base's turned by Rz Ry Rx.  Computed in float64 and rounded once; all zeros give the exact identity (a nominal row's)."""
    r, p, y = (np.deg2rad(float(a)) for a in (roll_deg, pitch_deg, yaw_deg))
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return (rz @ ry @ rx).T.astype(np.float32)


def check_pushes(push, nenv: int, device: int) -> None:
    """What `Batch.bind_pushes` accepts: a contiguous float32 [nenv, >= 2] tensor on cuda:`device`; raises OdkError otherwise."""
    _check_tensor("pushes", push, "float32", device, f"({nenv}, >= 2)", lambda s: len(s) == 2 and s[0] == int(nenv) and s[1] >= 2, " or None")


ACTION_DELAY_ROWS = 3      # the action-history ring: delay 0 (the action just given), 1, 2; a negative device row means "sample"


def check_action_delays(delays, nenv: int, device: int) -> None:
    """What `Batch.bind_action_delays` accepts: an int32 tensor on cuda:`device` with at least `nenv` rows -- [rows] or [rows, k], env e's
    delay the first entry of row e -- and a row stride (in elements) of at least 1; raises ValueError (an OdkError too) otherwise, before
    anything is launched.  The values are not read here: the kernel clamps them (include/odk.h)."""
    import torch
    if not torch.is_tensor(delays):
        raise OdkValueError(f"action delays: expected a torch tensor or None, got {type(delays).__name__}")
    if delays.dtype != torch.int32:
        raise OdkValueError(f"action delays: dtype must be torch.int32, got {delays.dtype}")
    if delays.device.type != "cuda" or delays.device.index != int(device):
        raise OdkValueError(f"action delays: the tensor must live on cuda:{device} (the env's device), got {delays.device}")
    if delays.dim() not in (1, 2) or int(delays.shape[0]) < int(nenv) or (delays.dim() == 2 and int(delays.shape[1]) < 1):
        raise OdkValueError(f"action delays: shape must be (>= {nenv},) or (>= {nenv}, >= 1), got {tuple(delays.shape)}")
    if int(delays.stride(0)) < 1:
        raise OdkValueError(f"action delays: the row stride must be >= 1 element (one row per env), got {int(delays.stride(0))}")


def check_accumulator(name: str, acc, nenv: int, ncol: int, device: int) -> None:
    """An accumulator argument of one of `Batch`'s `*_accumulate` methods: a contiguous float32 [nenv, ncol] tensor on cuda:`device`; OdkError
    otherwise."""
    _check_tensor(name, acc, "float32", device, f"({nenv}, {ncol})", lambda s: s == (int(nenv), int(ncol)))


def _check_report(batch, name: str, acc, ncol: int, track_acc) -> None:
    """A report's `acc` ([nenv, ncol]) and `track_acc`, as every `Batch.*_accumulate` checks them first."""
    check_accumulator(f"{name}: acc", acc, batch.nenv, ncol, batch.device)
    check_accumulator(f"{name}: track_acc", track_acc, batch.nenv, TRACK_NACC, batch.device)


def _report_ptrs(batch, track_acc):
    """What every odk_*_accumulate starts with behind the batch: priv, done, truncation, track_acc."""
    return tuple(_ptr(t) for t in (batch.priv, batch.done, batch.truncation, track_acc))


def _check_torque_limit(batch, name: str, t):
    """`torque_limit` of `gait_accumulate` / `fall_accumulate`: None or float32 [nu] on the batch's device; returns the pointer argument."""
    if t is None:
        return None
    if not hasattr(t, "dim") or t.dim() != 1:
        raise OdkError(f"{name}: torque_limit: expected a 1-D torch tensor or None, got {type(t).__name__}")
    check_accumulator(f"{name}: torque_limit", t.unsqueeze(0), 1, batch.model.nu, batch.device)      # as one row of [1, nu]
    return _ptr(t)


def _check_table_and_map(name: str, what: str, table, of_env, nenv: int, device: int, want: str, shape_ok) -> tuple:
    """A float32 table, argument `what`, then the int32 [nenv] map `<what>_of_env` that gives every env a row of it; returns the table's shape."""
    _check_tensor(f"{name}: {what}", table, "float32", device, want, shape_ok)
    _check_tensor(f"{name}: {what}_of_env", of_env, "int32", device, f"({nenv},)", lambda s: s == (int(nenv),))
    return tuple(int(n) for n in table.shape)


def check_schedule(name: str, sched, sched_of_env, nenv: int, device: int):
    """The schedule arguments of `Batch.command_schedule_apply` / `Batch.response_accumulate`: `sched` a contiguous float32
    [nsched >= 1, 1 .. SCHED_MAX_SEGMENTS, SCHED_SEG_FLOATS] tensor and `sched_of_env` a contiguous int32 [nenv] tensor, both on cuda:`device`;
    OdkError otherwise.  Returns (nsched, nseg).  The contents (segment 0 at step 0, increasing starts, map entries in range) are the
    builder's to check: track.schedule_table / track.schedule_blocks."""
    return _check_table_and_map(name, "sched", sched, sched_of_env, nenv, device, f"(nsched >= 1, 1 .. {SCHED_MAX_SEGMENTS}, {SCHED_SEG_FLOATS})",
                                lambda s: len(s) == 3 and s[0] >= 1 and 1 <= s[1] <= SCHED_MAX_SEGMENTS and s[2] == SCHED_SEG_FLOATS)[:2]


def check_courses(name: str, course, course_of_env, nenv: int, device: int) -> int:
    """The course arguments of `Batch.path_accumulate` / `Batch.waypoint_command_apply`: `course` a contiguous float32
    [ncourse >= 1, PATH_COURSE_FLOATS] tensor and `course_of_env` a contiguous int32 [nenv] tensor, both on cuda:`device`; OdkError otherwise.
    Returns ncourse.  The contents (a count of 1 .. PATH_MAX_WAYPOINTS, finite points, map entries in range) are the builder's to check:
    track.course_table / track.schedule_blocks; the kernels clamp what they index with."""
    return _check_table_and_map(name, "course", course, course_of_env, nenv, device, f"(ncourse >= 1, {PATH_COURSE_FLOATS})",
                                lambda s: len(s) == 2 and s[0] >= 1 and s[1] == PATH_COURSE_FLOATS)[0]


def check_path_parameter(name: str, what: str, value, positive: bool = False) -> float:
    """A controller setting of the path launches: a finite number >= 0 (`positive`: > 0); OdkError otherwise.  Returns it as a float."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise OdkError(f"{name}: {what} = {value!r} is not a number")
    if not np.isfinite(v) or v < 0 or (positive and v == 0):
        raise OdkError(f"{name}: {what} = {value!r} (a finite number {'> 0' if positive else '>= 0'})")
    return v


def _chk(rc: int):
    if rc != 0:
        raise OdkError(f"odk error {rc}: {load_library().odk_last_error().decode()}")


def default_config(standing: bool = False) -> EnvConfig:
    cfg = EnvConfig()
    L = load_library()
    (L.odk_default_config_standing if standing else L.odk_default_config)(C.byref(cfg))
    return cfg


def obs_sizes(env_kind: int):
    """(nobs, npriv) row strides of the observation outputs for an env kind (0 Joystick, 1 Standing) -- of the duck (14 actuators)."""
    a, b = C.c_int(0), C.c_int(0)
    load_library().odk_obs_sizes(int(env_kind), C.byref(a), C.byref(b))
    return a.value, b.value


@contextlib.contextmanager
def _loaded_model(model: Model):
    """(L, handle) of `model` loaded into the library for a host-only query, freed on the way out."""
    L = load_library()
    blob = model.blob()
    h = C.c_void_p()
    _chk(L.odk_model_load(blob, len(blob), C.byref(h)))
    try:
        yield L, h
    finally:
        L.odk_model_free(h)


def model_obs_sizes(model: Model, env_kind: int = 0):
    """(nobs, npriv) of `model`'s env kernels (`odk_model_obs_sizes`): the reference's layout with the robot's actuator count; host-only."""
    with _loaded_model(model) as (L, h):
        a, b = C.c_int(0), C.c_int(0)
        _chk(L.odk_model_obs_sizes(h, int(env_kind), C.byref(a), C.byref(b)))
        return a.value, b.value


def model_reduction(model: Model) -> Dict:
    """The twin-dof reduction the kernels use for `model` (odk_model_reduced) + its LDS footprint; host-only, no GPU."""
    with _loaded_model(model) as (L, h):
        ints = [C.c_int(0) for _ in range(4)]
        main, twin = (C.c_int * 32)(), (C.c_int * 32)()
        _chk(L.odk_model_reduced(h, *[C.byref(i) for i in ints], main, twin))
        nvr = ints[1].value
        return dict(paired=ints[0].value, nvr=nvr, nMr=ints[2].value, nHr=ints[3].value, main=list(main)[:nvr], twin=list(twin)[:nvr],
                    env_lds_floats=L.odk_model_env_lds_floats(h))


HOT_FIELD_NAMES = ("foot_body0", "foot_body1", "foot_nvert0", "foot_nvert1", "foot_rchain_first0", "foot_rchain_first1", "foot_rchain_len0", "foot_rchain_len1",
                   "ls_iterations", "max_nonpath_level", "np_count", "foot_prim")


def model_hot_words(model: Model) -> Dict:
    """The packed words the plane-floor step kernel reads the model's launch-invariant small integers from, and the values they were
    packed from (odk_model_hot_words); host-only, no GPU."""
    with _loaded_model(model) as (L, h):
        packed, fields = (C.c_int * 3)(), (C.c_int * 12)()
        _chk(L.odk_model_hot_words(h, packed, fields))
        return dict(packed=[v & 0xFFFFFFFF for v in packed], fields=dict(zip(HOT_FIELD_NAMES, list(fields))))


def model_body_lanes(model: Model, lanes_per_env: int) -> List[int]:
    """Body id of each of an env's `lanes_per_env` lanes in the kinematics / inertia sweeps, -1 for a lane without a body
    (odk_model_body_lanes); host-only, no GPU."""
    with _loaded_model(model) as (L, h):
        out = (C.c_int * lanes_per_env)()
        _chk(L.odk_model_body_lanes(h, int(lanes_per_env), out, lanes_per_env))
        return list(out)


def load_prm() -> Dict[str, np.ndarray]:
    z = np.load(asset_path("prm_table.npz"))
    return {k: z[k] for k in z.files}


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _stream(t):
    """torch's current stream on `t.device`; `t`: a tensor or a `Batch`."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _f32c(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype.is_floating_point and t.element_size() == 4):
            raise OdkError("learner kernels take contiguous float32 CUDA tensors")


def gae(truncation, termination, rewards, values, bootstrap, lambda_: float, discount: float, vs=None, adv=None, stats=None):
    """compute_gae on the device ([B, T] contiguous float32 CUDA tensors) -> (vs, advantages); one HIP launch.
    `truncation` / `termination` are flags: 0 = clear, anything else = set.
    `stats` (2 floats, optional) receives the advantage mean and 1/(std + 1e-8)."""
    import torch
    B, T = rewards.shape
    vs = torch.empty_like(rewards) if vs is None else vs
    adv = torch.empty_like(rewards) if adv is None else adv
    _f32c(truncation, termination, rewards, values, bootstrap, vs, adv, stats)
    _chk(load_library().odk_gae(_ptr(truncation), _ptr(termination), _ptr(rewards), _ptr(values), _ptr(bootstrap), _ptr(vs), _ptr(adv),
                                _ptr(stats), B, T, lambda_, discount, _stream(rewards)))
    return vs, adv


def ppo_head(logits, raw_action, old_log_prob, adv, stats, vs, baseline, noise, dlogits, dbaseline, losses, clipping_epsilon: float,
             entropy_cost: float, grad_scale: float = 1.0):
    """Fused PPO loss head (forward + gradients w.r.t. logits and baseline); `losses` must be zeroed by the caller."""
    n, a2 = logits.shape
    _f32c(logits, raw_action, old_log_prob, adv, stats, vs, baseline, noise, dlogits, dbaseline, losses)
    _chk(load_library().odk_ppo_head(_ptr(logits), _ptr(raw_action), _ptr(old_log_prob), _ptr(adv), _ptr(stats), _ptr(vs), _ptr(baseline),
                                     _ptr(noise), _ptr(dlogits), _ptr(dbaseline), _ptr(losses), n, a2 // 2, clipping_epsilon, entropy_cost,
                                     grad_scale, _stream(logits)))


def adam_clip(params, grads, m, v, acc, lr: float, max_grad_norm: float = 0.0, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8):
    """optax clip_by_global_norm + adam on flat float32 buffers; acc = ADAM_ACC_FLOATS scratch (acc[1] = step count)."""
    _f32c(params, grads, m, v, acc)
    if acc.numel() < ADAM_ACC_FLOATS:
        raise OdkError("adam_clip: acc needs ADAM_ACC_FLOATS floats")
    _chk(load_library().odk_adam_clip(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(acc), params.numel(), lr, b1, b2, eps,
                                      max_grad_norm or 0.0, _stream(params)))


def policy_sample(logits, noise, out=None):
    """(raw_action, action, log_prob) of the tanh-normal policy for logits [n, 2A] and standard-normal noise [n, A];
    `out`: the three result tensors to write into (contiguous [n, A], [n, A], [n]) instead of fresh ones."""
    import torch
    n, A = noise.shape
    _f32c(logits, noise)
    if out is not None:
        raw, act, logp = out
        _f32c(raw, act, logp)
        if raw.numel() != n * A or act.numel() != n * A or logp.numel() != n:
            raise OdkError("policy_sample: out tensors of the wrong size")
    else:
        raw, act, logp = torch.empty_like(noise), torch.empty_like(noise), torch.empty(n, device=noise.device)
    _chk(load_library().odk_policy_sample(_ptr(logits), _ptr(noise), _ptr(raw), _ptr(act), _ptr(logp), n, A, _stream(noise)))
    return raw, act, logp


def silu_bwd_colsum(dh, z, dz, colsum, partial):
    """dz = dh * silu'(z) ([n, w]) and colsum = dz.sum(0) in one pass; partial: scratch of ceil(n / 64) * w floats.
    colsum=None leaves the per-tile sums in `partial` for a later `ColsumFinalize` (one launch for several layers)."""
    n, w = z.shape
    _f32c(dh, z, dz, colsum, partial)
    if partial.numel() < ((n + 63) // 64) * w:
        raise OdkError("silu_bwd_colsum: partial scratch too small")
    _chk(load_library().odk_silu_bwd_colsum(_ptr(dh), _ptr(z), _ptr(dz), _ptr(colsum), _ptr(partial), n, w, _stream(z)))


def colsum_partial(x, partial):
    """Tile sums of x ([n, w]) for a later `ColsumFinalize` (partial: ceil(n / 64) * w floats)."""
    n, w = x.shape
    _f32c(x, partial)
    if partial.numel() < ((n + 63) // 64) * w:
        raise OdkError("colsum_partial: partial scratch too small")
    _chk(load_library().odk_colsum_partial(_ptr(x), _ptr(partial), n, w, _stream(x)))


class ColsumFinalize:
    """colsum[f] = fold of partial[f] for a fixed set of layers in one launch (`odk_colsum_finalize`); `n` = rows of dz."""

    def __init__(self, pairs, n: int):
        k = len(pairs)
        self.k, self.n, self.keep = k, int(n), pairs
        for p_, o_ in pairs:
            _f32c(p_, o_)
            if p_.numel() < ((n + 63) // 64) * o_.numel():
                raise OdkError("ColsumFinalize: partial scratch too small")
        self.partial = (C.c_void_p * k)(*[p_.data_ptr() for p_, _ in pairs])
        self.out = (C.c_void_p * k)(*[o_.data_ptr() for _, o_ in pairs])
        self.w = (C.c_int * k)(*[int(o_.numel()) for _, o_ in pairs])

    def __call__(self):
        _chk(load_library().odk_colsum_finalize(self.partial, self.out, self.w, self.k, self.n, _stream(self.keep[0][0])))


def quad_rows(n: int) -> int:
    """Rows of a quad-row buffer for n samples: n rounded up to whole 16-sample tiles (a multiple of 8, as odk_dw_gemm wants)."""
    return (int(n) + MLP_TILE - 1) // MLP_TILE * MLP_TILE


def quad_pack(t):
    """[n, width] -> the quad-row layout [np / 4][width][4] the fused network / weight-gradient kernels use (flat tensor, rows
    past n zero).  Plain torch ops: tests and tools."""
    import torch
    n, w = t.shape
    full = torch.zeros(quad_rows(n), w, device=t.device, dtype=t.dtype)
    full[:n] = t
    return full.view(-1, 4, w).permute(0, 2, 1).contiguous().reshape(-1)


def quad_unpack(buf, n: int, width: int):
    """Inverse of `quad_pack`: the first n rows as [n, width]."""
    return buf.view(-1, width, 4).permute(0, 2, 1).reshape(-1, width)[:n]


class DwGemm:
    """Weight gradients out[off_l : off_l + n_out n_in] = dz_l^T h_l of up to 8 layers in one launch (`odk_dw_gemm`, f32
    matrix cores, split over `kslices` row slices folded in a fixed order).  `layers`: [(dz, h, n_out, n_in, offset in
    `flat_out`)] with dz / h flat QUAD-ROW buffers ([np / 4][width][4], `quad_pack`; np a multiple of 8, >= 8 * kslices);
    `workspace`: kslices * workspace_stride(flat_out.numel()) floats.
    `bias`: [(tile sums [nblk, width], bias gradient [width], nblk)] folded by the same finishing launch (what `ColsumFold` does);
    `acc`: the Adam scratch -- the finishing launch then also leaves the partial sums of the squared gradient norm in acc[2:] and
    advances the step count acc[1]; `norm_blocks` is what `adam_clip_packed` wants to hear about it."""

    def __init__(self, layers, flat_out, workspace, kslices: int = 8, bias=(), acc=None):
        k = len(layers)
        _f32c(flat_out, workspace, *[t for dz, h, _, _, _ in layers for t in (dz, h)])
        if k > 8 or kslices % 8 != 0:
            raise OdkError("DwGemm: at most 8 layers, kslices a multiple of 8")
        rows = []
        for dz, h, no, ni, o in layers:
            np_ = dz.numel() // int(no)
            if dz.numel() != np_ * no or h.numel() != np_ * ni or np_ % 8 or np_ // 8 < 2 * kslices:
                raise OdkError("DwGemm: dz / h must be quad-row buffers of the same row count (a multiple of 8, >= 16 * kslices)")
            if int(o) % 4 or (int(no) * int(ni)) % 4:
                raise OdkError("DwGemm: offsets and element counts must be multiples of 4")
            rows.append(np_)
        stride = self.workspace_stride(flat_out.numel())
        if workspace.numel() < kslices * stride:
            raise OdkError("DwGemm: workspace too small (kslices * workspace_stride(flat_out.numel()) floats)")
        self.keep = (layers, flat_out, workspace)
        self.k, self.kslices, self.stride = k, int(kslices), stride
        self.n = (C.c_int * k)(*rows)
        self.dz = (C.c_void_p * k)(*[l[0].data_ptr() for l in layers])
        self.h = (C.c_void_p * k)(*[l[1].data_ptr() for l in layers])
        self.n_out = (C.c_int * k)(*[int(l[2]) for l in layers])
        self.n_in = (C.c_int * k)(*[int(l[3]) for l in layers])
        self.off = (C.c_longlong * k)(*[int(l[4]) for l in layers])
        self.finish, self.norm_blocks = None, 0
        if bias or acc is not None:
            if len(bias) > 8:
                raise OdkError("DwGemm: at most 8 bias gradients")
            f = GradFinish()
            f.nbias = len(bias)
            for i, (part, grad, nblk) in enumerate(bias):
                _f32c(part, grad)
                if part.numel() < int(nblk) * grad.numel():
                    raise OdkError("DwGemm: bias tile sums too small")
                f.bias_partial[i], f.bias_grad[i], f.width[i], f.nblk[i] = part.data_ptr(), grad.data_ptr(), int(grad.numel()), int(nblk)
            if acc is not None:
                _f32c(acc)
                if acc.numel() < ADAM_ACC_FLOATS:
                    raise OdkError("DwGemm: acc needs ADAM_ACC_FLOATS floats")
                f.sq_partials_dev, f.step_counter_dev = acc.data_ptr() + 8, acc.data_ptr() + 4
            self.finish, self.keep_finish = f, (bias, acc)

    @staticmethod
    def workspace_stride(numel: int) -> int:
        return (int(numel) + 3) // 4 * 4

    def __call__(self):
        _, flat_out, ws = self.keep
        _chk(load_library().odk_dw_gemm(self.dz, self.h, self.n_out, self.n_in, self.off, self.k, self.n, self.kslices, _ptr(ws), self.stride,
                                        _ptr(flat_out), C.byref(self.finish) if self.finish is not None else None, _stream(flat_out)))
        if self.finish is not None and self.finish.sq_partials_dev:
            self.norm_blocks = int(self.finish.nblocks)


def _pad16(k: int) -> int:
    return (int(k) + 15) // 16 * 16


class WeightTable:
    """Where the weight matrices sit inside a flat parameter buffer -- [(float offset, rows = n_out, cols = n_in, backward copy?)],
    at most 8 -- and inside the two packed buffers the fused network kernels read (layouts: include/odk.h, odk_mlp_desc).
    `fwd_size` / `bwd_size`: floats to allocate (zero-initialised) for the packed buffers."""

    def __init__(self, entries):
        if len(entries) > 8:
            raise OdkError("WeightTable: at most 8 weights")
        self.entries = [(int(o), int(r), int(c), bool(bw)) for o, r, c, bw in entries]
        t = WeightTableC()
        t.count = len(entries)
        fo = bo = 0
        self.fwd, self.bwd = [], []
        for k, (o, r, c, bw) in enumerate(self.entries):
            t.off[k], t.rows[k], t.cols[k] = o, r, c
            t.fwd_off[k] = fo; self.fwd.append((fo, _pad16(c) * r)); fo += _pad16(c) * r
            if bw:
                t.bwd_off[k] = bo; self.bwd.append((bo, _pad16(r) * c)); bo += _pad16(r) * c
            else:
                t.bwd_off[k] = -1; self.bwd.append(None)
        self.c, self.fwd_size, self.bwd_size = t, fo, max(bo, 4)

    def fwd_view(self, buf, k):
        o, n = self.fwd[k]
        return buf[o:o + n]

    def bwd_view(self, buf, k):
        if self.bwd[k] is None:
            return None
        o, n = self.bwd[k]
        return buf[o:o + n]


def pack_weights(params, fwd_packed, bwd_packed, table: WeightTable):
    """(Re)builds the packed weight copies from the flat parameter buffer (`odk_pack_weights`); padding is left untouched."""
    _f32c(params, fwd_packed, bwd_packed)
    if fwd_packed.numel() < table.fwd_size or bwd_packed.numel() < table.bwd_size:
        raise OdkError("pack_weights: packed buffers too small")
    _chk(load_library().odk_pack_weights(_ptr(params), params.numel(), _ptr(fwd_packed), fwd_packed.numel(), _ptr(bwd_packed), bwd_packed.numel(),
                                         C.byref(table.c), _stream(params)))


def adam_clip_packed(params, grads, m, v, acc, fwd_packed, bwd_packed, table: WeightTable, lr: float, max_grad_norm: float = 0.0, b1: float = 0.9,
                     b2: float = 0.999, eps: float = 1e-8, norm_blocks: int = 0, cursor=None, loss_partials=None, losses=None):
    """`adam_clip` that also writes every updated weight to its places in the packed copies (`odk_adam_clip_packed`).
    `norm_blocks` > 0: the gradient's finishing launch (`DwGemm(..., acc=acc)`) already left that many partial sums of the
    squared norm in acc[2:] and advanced the step count: no norm launch here.  End-of-step duties of the same launch
    (`odk_adam_clip_packed_tail`, all optional): `cursor` (int32 CUDA tensor of one element) -- the minibatch cursor of the learner's
    schedule, advanced by one; `loss_partials` ([w, 4], what `GaeHead` leaves) folded into `losses` ([4], +=) in workgroup order."""
    _f32c(params, grads, m, v, acc, fwd_packed, bwd_packed)
    if acc.numel() < ADAM_ACC_FLOATS or fwd_packed.numel() < table.fwd_size or bwd_packed.numel() < table.bwd_size:
        raise OdkError("adam_clip_packed: acc needs ADAM_ACC_FLOATS floats, the packed buffers table.fwd_size / bwd_size")
    if cursor is not None and not (cursor.is_cuda and cursor.numel() == 1 and cursor.element_size() == 4 and not cursor.dtype.is_floating_point):
        raise OdkError("adam_clip_packed: cursor must be a one-element int32 CUDA tensor")
    tail = None
    if cursor is not None or loss_partials is not None:
        _f32c(loss_partials, losses)
        if loss_partials is not None and (losses is None or losses.numel() < 4 or loss_partials.numel() % 4):
            raise OdkError("adam_clip_packed: loss_partials [w, 4] need losses [4]")
        tail = StepTail(None if cursor is None else cursor.data_ptr(), None if loss_partials is None else loss_partials.data_ptr(),
                        0 if loss_partials is None else loss_partials.numel() // 4, None if losses is None else losses.data_ptr())
    _chk(load_library().odk_adam_clip_packed_tail(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(acc), params.numel(), lr, b1, b2, eps,
                                                  max_grad_norm or 0.0, _ptr(fwd_packed), fwd_packed.numel(), _ptr(bwd_packed), bwd_packed.numel(),
                                                  C.byref(table.c), int(norm_blocks), C.byref(tail) if tail is not None else None, _stream(params)))


def col_moments(x, slices: int = 1024):
    """(column sums, column sums of squares) of a contiguous float32 CUDA matrix x [rows, w], float64, in one pass (`odk_col_moments` + a
    fixed-order fold of its row slices): the observation normaliser's batch statistics."""
    import torch
    _f32c(x)
    rows, w = x.shape
    slices = max(1, min(int(slices), 1024, int(rows)))
    part = torch.empty(slices, 2, w, dtype=torch.float64, device=x.device)
    _chk(load_library().odk_col_moments(_ptr(x), int(rows), int(w), slices, _ptr(part), _stream(x)))
    tot = part.sum(0)
    return tot[0], tot[1]


def running_stats_update(x, count, mean, summed_variance, std, std_min: float, std_max: float, slices: int = 1024):
    """brax running_statistics.update of (count float64 [], mean / summed_variance / std float32 [w]) with the batch x [rows, w] (contiguous float32
    CUDA), in place, three launches and no host arithmetic (`odk_col_moments` + `odk_moments_update`)."""
    import torch
    _f32c(x, mean, summed_variance, std)
    rows, w = x.shape
    if not (count.is_cuda and count.dtype == torch.float64 and count.numel() == 1):
        raise OdkError("running_stats_update: count must be a float64 CUDA scalar")
    slices = max(1, min(int(slices), 1024, int(rows)))
    part = torch.empty(slices, 2, w, dtype=torch.float64, device=x.device)
    L = load_library()
    _chk(L.odk_col_moments(_ptr(x), int(rows), int(w), slices, _ptr(part), _stream(x)))
    _chk(L.odk_moments_update(_ptr(part), slices, int(w), int(rows), _ptr(count), _ptr(mean), _ptr(summed_variance), _ptr(std),
                              float(std_min), float(std_max), _stream(x)))


class GaeHead:
    """GAE + advantage statistics + PPO loss head of a minibatch in ONE launch, the rollout read through the schedule's trajectory
    indices (`odk_ppo_gae_head`; include/odk.h names every argument).  Built once over fixed tensors:
      logits [n, 2A], values [n + B], rollout tensors raw_action [n_traj, T, A], log_prob / reward / termination / truncation
      [n_traj, T], noise [steps, n, A], schedule int64 [steps * B], cursor int32 [1], dlogits [n, 2A], dvalues [>= n], losses [4];
      optional adv / vs [n] and stats [2] (copies of the intermediate results); `loss_partials` ([ceil(n / 32), 4]): the per-workgroup loss
      sums go there instead of float atomics on `losses` (`adam_clip_packed(loss_partials=..., losses=...)` folds them)."""

    def __init__(self, logits, values, rollout: dict, noise, schedule, cursor, dlogits, dvalues, losses, B: int, T: int, cfg: dict, grad_scale: float = 1.0,
                 adv=None, vs=None, stats=None, loss_partials=None):
        import torch
        n, A = B * T, logits.shape[1] // 2
        fl = [logits, values, noise, dlogits, dvalues, losses] + [rollout[k] for k in ("raw_action", "log_prob", "reward", "termination", "truncation")]
        _f32c(*fl, adv, vs, stats, loss_partials)
        if loss_partials is not None and loss_partials.numel() < 4 * ((n + GAE_HEAD_SAMPLES - 1) // GAE_HEAD_SAMPLES):
            raise OdkError("GaeHead: loss_partials needs 4 floats per 32 samples")
        n_traj = int(rollout["reward"].shape[0])
        if tuple(logits.shape) != (n, 2 * A) or values.numel() < n + B or dlogits.numel() != n * 2 * A or dvalues.numel() < n or losses.numel() < 4:
            raise OdkError("GaeHead: logits [B T, 2 A], values [B T + B], dlogits like logits, dvalues [>= B T], losses [4]")
        if any(int(rollout[k].shape[0]) != n_traj or int(rollout[k][0].numel()) != T * (A if k == "raw_action" else 1)
               for k in ("raw_action", "log_prob", "reward", "termination", "truncation")):
            raise OdkError("GaeHead: rollout tensors must be [n_traj, T(, A)]")
        if not (schedule.is_cuda and schedule.dtype == torch.int64 and schedule.is_contiguous() and schedule.numel() % B == 0):
            raise OdkError("GaeHead: schedule must be a contiguous int64 CUDA tensor of steps * B entries")
        if not (cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1):
            raise OdkError("GaeHead: cursor must be a one-element int32 CUDA tensor")
        if noise.numel() < (schedule.numel() // B) * n * A:
            raise OdkError("GaeHead: the noise pool needs one [n, A] slot per schedule step")
        if n > 5120 or B > 1024:
            raise OdkError("GaeHead: B * T <= 5120, B <= 1024")
        a = GaeHeadArgs()
        a.logits, a.values, a.noise, a.dlogits, a.dvalues, a.losses = (t.data_ptr() for t in (logits, values, noise, dlogits, dvalues, losses))
        a.raw_action, a.old_log_prob, a.reward, a.termination, a.truncation = (rollout[k].data_ptr() for k in ("raw_action", "log_prob", "reward", "termination", "truncation"))
        a.row_idx, a.cursor = schedule.data_ptr(), cursor.data_ptr()
        a.adv_out, a.vs_out, a.stats_out, a.loss_partials = (None if t is None else t.data_ptr() for t in (adv, vs, stats, loss_partials))
        a.B, a.T, a.action_size, a.n_traj, a.normalize_advantage = int(B), int(T), int(A), n_traj, int(bool(cfg["normalize_advantage"]))
        a.gae_lambda, a.discount, a.clipping_epsilon, a.entropy_cost, a.grad_scale = (float(cfg["gae_lambda"]), float(cfg["discounting"]), float(cfg["clipping_epsilon"]),
                                                                                       float(cfg["entropy_cost"]), float(grad_scale))
        self.a, self.keep = a, (fl, rollout, schedule, cursor, adv, vs, stats, loss_partials)

    def __call__(self):
        _chk(load_library().odk_ppo_gae_head(C.byref(self.a), _stream(self.keep[0][0])))


class ColsumFold:
    """colsum[f] = sum over the nblk[f] tile rows of partial[f] ([nblk[f], width]) for up to 8 layers in one launch (`odk_colsum_fold`)."""

    def __init__(self, pairs, nblk):
        k = len(pairs)
        self.k, self.keep = k, pairs
        nblk = [int(nblk)] * k if isinstance(nblk, int) else [int(b) for b in nblk]
        for (p_, o_), nb in zip(pairs, nblk):
            _f32c(p_, o_)
            if p_.numel() < nb * o_.numel():
                raise OdkError("ColsumFold: partial buffer too small")
        self.nblk = (C.c_int * k)(*nblk)
        self.partial = (C.c_void_p * k)(*[p_.data_ptr() for p_, _ in pairs])
        self.out = (C.c_void_p * k)(*[o_.data_ptr() for _, o_ in pairs])
        self.w = (C.c_int * k)(*[int(o_.numel()) for _, o_ in pairs])

    def __call__(self):
        _chk(load_library().odk_colsum_fold(self.partial, self.out, self.w, self.nblk, self.k, _stream(self.keep[0][0])))


class FusedMLP:
    """One or two swish MLPs (n_in -> 512 -> 256 -> 128 -> n_out) whose forward pass is ONE launch and whose backward-data chain is
    ONE launch (`odk_mlp_forward` / `odk_mlp_backward`, csrc/odk_mlp.hip).  Each net is a dict of tensors:
      x [n, n_in], wf[4] (forward-packed weights: `WeightTable.fwd_view`), b[4], out [n, n_out], optionally in_mean / in_std [n_in]
      (the input is normalised on load); for training also wb[4]
      (backward-packed, wb[0] may be None), dout [n, n_out], bias_partial[4] ([ceil(n / 16), width]) and the flat QUAD-ROW
      buffers (`quad_rows(n)` x width floats, layout of `quad_pack`) xp (copy of x), h[3], g[3] (activations, swish'), dz[3],
      doutp (copy of dout) -- `train_buffers` allocates them."""

    @staticmethod
    def train_buffers(n: int, n_in: int, n_out: int, device):
        import torch
        np_, tiles = quad_rows(n), quad_rows(n) // MLP_TILE
        E = lambda k: torch.empty(k, device=device)
        return dict(xp=E(np_ * n_in), h=[E(np_ * w) for w in MLP_HIDDEN], g=[E(np_ * w) for w in MLP_HIDDEN], dz=[E(np_ * w) for w in MLP_HIDDEN],
                    doutp=E(np_ * n_out), bias_partial=[E(tiles * w) for w in MLP_HIDDEN + (n_out,)])

    def __init__(self, nets):
        if not 1 <= len(nets) <= 2:
            raise OdkError("FusedMLP: one or two networks")
        self.k = len(nets)
        self.keep = nets
        self.desc = (MlpDesc * self.k)()
        self.train = []
        for d, nt in zip(self.desc, nets):
            x, out = nt["x"], nt["out"]
            n, n_in = out.shape[0], x.shape[1]      # (with row sources x is the whole rollout: the row count is the output's)
            n_out = out.shape[1]
            widths = (n_in,) + MLP_HIDDEN + (n_out,)
            if n_in > MLP_MAX_IN or n_out > MLP_MAX_OUT or (nt.get("row_idx") is None and x.shape[0] != n):
                raise OdkError("FusedMLP: n_in <= 224, n_out <= 32")
            _f32c(x, out, *nt["wf"], *nt["b"])
            for l in range(4):
                if nt["wf"][l].numel() != _pad16(widths[l]) * widths[l + 1] or nt["b"][l].numel() != widths[l + 1]:
                    raise OdkError(f"FusedMLP: layer {l} is not {widths[l]} -> {widths[l + 1]} (hidden widths are fixed at {MLP_HIDDEN})")
            d.x, d.out, d.n, d.n_in, d.n_out = x.data_ptr(), out.data_ptr(), int(n), int(n_in), int(n_out)
            if nt.get("row_idx") is not None:      # rows through the minibatch schedule (odk_mlp_desc.row_idx): x is the whole rollout
                import torch
                ri, cur = nt["row_idx"], nt["cursor"]
                if not (ri.is_cuda and ri.dtype == torch.int64 and ri.is_contiguous() and cur.is_cuda and cur.dtype == torch.int32 and cur.numel() == 1):
                    raise OdkError("FusedMLP: row_idx int64 / cursor int32[1] CUDA tensors")
                d.row_idx, d.cursor = ri.data_ptr(), cur.data_ptr()
                d.traj_len, d.n_main, d.n_traj = int(nt["traj_len"]), int(nt["n_main"]), int(nt["n_traj"])
                if nt.get("x_tail") is not None:
                    _f32c(nt["x_tail"])
                    d.x_tail = nt["x_tail"].data_ptr()
            if nt.get("in_mean") is not None:      # normalise the input on load: (x - in_mean) / in_std
                _f32c(nt["in_mean"], nt["in_std"])
                if nt["in_mean"].numel() != n_in or nt["in_std"].numel() != n_in:
                    raise OdkError("FusedMLP: in_mean / in_std must have n_in entries")
                d.in_mean, d.in_std = nt["in_mean"].data_ptr(), nt["in_std"].data_ptr()
            for l in range(4):
                d.wf[l], d.b[l] = nt["wf"][l].data_ptr(), nt["b"][l].data_ptr()
            train = "h" in nt
            self.train.append(train)
            if train:
                tiles, np_ = (n + MLP_TILE - 1) // MLP_TILE, quad_rows(n)
                _f32c(nt["dout"], nt["xp"], nt["doutp"], *nt["h"], *nt["g"], *nt["dz"], *nt["bias_partial"], *nt["wb"][1:])
                if nt["xp"].numel() != np_ * n_in or nt["doutp"].numel() != np_ * n_out:
                    raise OdkError("FusedMLP: xp / doutp must be quad-row buffers of quad_rows(n) rows")
                d.xp, d.doutp = nt["xp"].data_ptr(), nt["doutp"].data_ptr()
                for l in range(1, 4):
                    if nt["wb"][l].numel() != _pad16(widths[l + 1]) * widths[l]:
                        raise OdkError(f"FusedMLP: backward-packed weight {l} has the wrong size")
                    d.wb[l] = nt["wb"][l].data_ptr()
                for l in range(3):
                    for key in ("h", "g", "dz"):
                        if nt[key][l].numel() != np_ * MLP_HIDDEN[l]:
                            raise OdkError(f"FusedMLP: {key}[{l}] must be a quad-row buffer of {np_} x {MLP_HIDDEN[l]} floats")
                    d.h[l], d.g[l], d.dz[l] = nt["h"][l].data_ptr(), nt["g"][l].data_ptr(), nt["dz"][l].data_ptr()
                if tuple(nt["dout"].shape) != (n, n_out):
                    raise OdkError("FusedMLP: dout must match out")
                d.dout = nt["dout"].data_ptr()
                for l in range(4):
                    if nt["bias_partial"][l].numel() < tiles * widths[l + 1]:
                        raise OdkError("FusedMLP: bias_partial too small")
                    d.bias_partial[l] = nt["bias_partial"][l].data_ptr()

    def forward(self):
        _chk(load_library().odk_mlp_forward(self.desc, self.k, _stream(self.keep[0]["x"])))

    def backward(self):
        if not all(self.train):
            raise OdkError("FusedMLP.backward: built without training buffers")
        _chk(load_library().odk_mlp_backward(self.desc, self.k, _stream(self.keep[0]["x"])))


class MultiCopy:
    """dst[f] <- src[f] for up to 10 (src, dst) pairs of equally sized contiguous float32 CUDA tensors in ONE launch (the block
    copy mode of `odk_gather_rows`): e.g. the five per-step snapshots of a rollout."""

    def __init__(self, pairs):
        import torch
        n = len(pairs)
        if not 1 <= n <= 10:
            raise OdkError("MultiCopy: 1..10 pairs")
        for s_, d_ in pairs:
            _f32c(s_, d_)
            if s_.numel() != d_.numel():
                raise OdkError("MultiCopy: sizes differ")
        self.n, self.keep = n, pairs
        self.src = (C.c_void_p * n)(*[s_.data_ptr() for s_, _ in pairs])
        self.dst = (C.c_void_p * n)(*[d_.data_ptr() for _, d_ in pairs])
        self.rows = (C.c_int * n)(*[int(s_.numel()) for s_, _ in pairs])
        self.base = (C.c_longlong * n)(*([0] * n))
        self.idx = torch.zeros(1, dtype=torch.int64, device=pairs[0][0].device)   # (unused: every field is a block copy)

    def __call__(self):
        _chk(load_library().odk_gather_rows(self.src, self.dst, self.rows, self.base, self.n, _ptr(self.idx), 1, 1, _stream(self.keep[0][0])))


class RowGather:
    """dst[f][b] = src[f][idx[b]] for a fixed set of (src, dst) float32 tensors in one launch (`odk_gather_rows`).
    `direct`: further (src, dst) pairs copied as plain blocks, dst[b] = src[base + b] with `base` given per call (the
    learner's slice of its noise pool rides along with the minibatch gather instead of being a launch of its own)."""

    def __init__(self, pairs, direct=()):
        allp = list(pairs) + list(direct)
        n = len(allp)
        if n > 10:
            raise OdkError("RowGather: at most 10 fields")
        self.n, self.nidx = n, len(pairs)
        self.keep = allp
        for s_, d_ in allp:
            _f32c(s_, d_)
        self.src = (C.c_void_p * n)(*[s_.data_ptr() for s_, _ in allp])
        self.dst = (C.c_void_p * n)(*[d_.data_ptr() for _, d_ in allp])
        self.rows = (C.c_int * n)(*[int(s_[0].numel()) for s_, _ in allp])
        self.base = (C.c_longlong * n)(*([-1] * n))
        self.nrows = int(pairs[0][1].shape[0])
        self.src_rows = int(pairs[0][0].shape[0])
        for s_, d_ in pairs:
            if int(s_.shape[0]) != self.src_rows or int(d_.shape[0]) != self.nrows or s_[0].numel() != d_[0].numel():
                raise OdkError("RowGather: every source needs the same row count, every destination the same row count, and "
                               "matching row lengths")
        for s_, d_ in direct:
            if int(d_.shape[0]) != self.nrows or s_[0].numel() != d_[0].numel():
                raise OdkError("RowGather: a direct field needs the destinations' row count and matching row lengths")

    def __call__(self, idx, direct_base=()):
        """`idx`: contiguous int64 CUDA tensor of `nrows` source-row numbers (values outside the source are not read: those
        destination rows become NaN); `direct_base`: first source row of every direct field."""
        import torch
        if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == self.nrows):
            raise OdkError(f"RowGather: idx must be a contiguous int64 CUDA tensor of {self.nrows} entries "
                           f"(got {idx.dtype}, {idx.device}, contiguous={idx.is_contiguous()}, {idx.numel()} entries)")
        if len(direct_base) != self.n - self.nidx:
            raise OdkError("RowGather: one base row per direct field")
        for k, b in enumerate(direct_base):
            s_ = self.keep[self.nidx + k][0]
            if b < 0 or b + self.nrows > int(s_.shape[0]):
                raise OdkError("RowGather: direct block out of range")
            self.base[self.nidx + k] = int(b)
        _chk(load_library().odk_gather_rows(self.src, self.dst, self.rows, self.base, self.n, _ptr(idx), self.nrows, self.src_rows, _stream(idx)))


class Batch:
    """`nenv` environments resident on one GPU.  Thin: every method is one C-ABI call."""

    def __init__(self, model: Model, nenv: int, cfg: Optional[EnvConfig] = None, device: int = 0, prm: Optional[dict] = None):
        import torch

        if not torch.cuda.is_available():
            raise OdkError("no HIP device visible: the env engine has no CPU path")
        self.L = load_library()
        self.torch = torch
        self.model, self.nenv, self.device = model, int(nenv), int(device)
        self.cfg = cfg if cfg is not None else default_config()
        blob = model.blob()
        self._m = C.c_void_p()
        _chk(self.L.odk_model_load(blob, len(blob), C.byref(self._m)))
        prm = prm if prm is not None else load_prm()
        self._table = np.ascontiguousarray(prm["table"], np.float32)
        dxs, dys, dths = (np.ascontiguousarray(prm[k], np.float64) for k in ("dxs", "dys", "dthetas"))
        ranges = np.ascontiguousarray(np.concatenate([prm["dx_range"], prm["dy_range"], prm["dtheta_range"]]), np.float64)
        self._b = C.c_void_p()
        _chk(self.L.odk_batch_create(self._m, C.byref(self.cfg), self.nenv, self.device, _fp(self._table), _dp(dxs), len(dxs), _dp(dys),
                                     len(dys), _dp(dths), len(dths), _dp(ranges), int(prm["nb_steps_in_period"][0]), C.byref(self._b)))
        dev = torch.device("cuda", self.device)
        f32 = dict(dtype=torch.float32, device=dev)
        a_, b_ = C.c_int(0), C.c_int(0)
        _chk(self.L.odk_model_obs_sizes(self._m, int(self.cfg.env_kind), C.byref(a_), C.byref(b_)))
        self.nobs, self.npriv = a_.value, b_.value
        self.lanes_per_env = int(self.L.odk_batch_lanes(self._b))      # what the kernels run (cfg.lanes_per_env is a hint)
        self.obs = torch.zeros(self.nenv, self.nobs, **f32)
        self.priv = torch.zeros(self.nenv, self.npriv, **f32)
        self.reward = torch.zeros(self.nenv, **f32)
        self.done = torch.zeros(self.nenv, **f32)
        self.truncation = torch.zeros(self.nenv, **f32)
        self.metrics = torch.zeros(self.nenv, NMETRIC, **f32)
        self._outs = Outputs(self.obs.data_ptr(), self.priv.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                             self.truncation.data_ptr(), self.metrics.data_ptr())
        self.commands = None         # the tensor bound by bind_commands (kept alive while bound)
        self.pushes = None           # the tensor bound by bind_pushes (kept alive while bound)
        self.action_delays = None    # the tensor bound by bind_action_delays (kept alive while bound)
        self.xmetrics = None         # [nenv, NXTERM] reward-library metrics, allocated by the first set_reward_terms that turns a term on
        self.reward_terms_on = False
        self.generation = 0          # advanced by every call that rewrites the per-env records (reset / step / set_records): `State.info` checks it

    # -- streams: calls are ordered on torch's current stream (the module's `_stream`, as a method: it reads `self.device`)
    _stream = _stream

    def set_config(self, cfg: EnvConfig):
        self.cfg = cfg
        _chk(self.L.odk_batch_set_config(self._b, C.byref(cfg)))

    def set_param(self, param: int, values: np.ndarray):
        v = np.ascontiguousarray(values, np.float32).reshape(self.nenv, -1)
        _chk(self.L.odk_batch_set_param(self._b, param, _fp(v), v.shape[1]))

    def reset(self, seed: int, env_id_offset: int = 0):
        self.generation += 1
        _chk(self.L.odk_reset(self._b, seed & 0xFFFFFFFF, env_id_offset, C.byref(self._outs), self._stream()))

    def step(self, action):
        assert action.is_cuda and action.dtype == self.torch.float32 and action.is_contiguous() and tuple(action.shape) == (self.nenv, self.model.nu)
        self.generation += 1
        _chk(self.L.odk_step(self._b, _ptr(action), C.byref(self._outs), self._stream()))

    def bind_commands(self, cmd):
        """Drive every env with the caller's command (`odk_batch_bind_commands`): `cmd` is a contiguous float32 [nenv, 7] tensor on
        this batch's device, row e = env e's command (include/odk.h); None returns to sampled commands.  The batch keeps a reference
        to the tensor while it is bound.  Write into it (stream-ordered) to change the command of the next step; a captured graph
        keeps the buffer it was captured with, so rebind only before capturing."""
        if cmd is None:
            _chk(self.L.odk_batch_bind_commands(self._b, None, 0))
            self.commands = None
            return
        check_commands(cmd, self.nenv, self.device)
        _chk(self.L.odk_batch_bind_commands(self._b, _ptr(cmd), NCOMMAND))
        self.commands = cmd

    def bind_pushes(self, push):
        """Push every env with the caller's kick (`odk_batch_bind_pushes`): `push` is a contiguous float32 [nenv, >= 2] tensor on this
        batch's device, row e = the world-frame velocity kick (dvx, dvy) in m/s that env e's next step adds to qvel[0:2] (include/odk.h);
        None returns to the sampled push.  A row left non-zero is applied by every step: write it (stream-ordered) for the step that is to
        be pushed and zero it afterwards.  The batch keeps a reference to the tensor while it is bound; a captured graph keeps the buffer
        it was captured with, so rebind only before capturing."""
        if push is None:
            _chk(self.L.odk_batch_bind_pushes(self._b, None, 0))
            self.pushes = None
            return
        check_pushes(push, self.nenv, self.device)
        _chk(self.L.odk_batch_bind_pushes(self._b, _ptr(push), int(push.shape[1])))
        self.pushes = push

    def bind_action_delays(self, delays):
        """Fix every env's action delay (`odk_batch_bind_action_delays`): `delays` is an int32 tensor on this batch's device with at least
        nenv rows ([rows] or [rows, k]; `check_action_delays`), row e = the action-history row 0, 1 or 2 that env e's next step turns into
        motor targets (0: the action just given), a negative value = the sampled delay for that env; None returns every env to the sampler.
        The kernel clamps a value above 2 to 2.  The random streams stay those of an unbound run.  The batch keeps a reference to the tensor
        while it is bound; write into it (stream-ordered) to change the delays; a captured graph keeps the buffer it was captured with, so
        rebind only before capturing."""
        if delays is None:
            _chk(self.L.odk_batch_bind_action_delays(self._b, None, 0))
            self.action_delays = None
            return
        check_action_delays(delays, self.nenv, self.device)
        _chk(self.L.odk_batch_bind_action_delays(self._b, _ptr(delays), int(delays.stride(0))))
        self.action_delays = delays

    def set_reward_terms(self, terms: Optional[RewardTerms]):
        """Reward-library terms of the step kernel (`odk_batch_set_reward_terms`): None or all scales 0 turns them off.  While some
        term is on every step writes `xmetrics` ([nenv, NXTERM], column = XTERM_NAMES index, 0 for a term that is off).  Synchronous;
        a graph captured while a term was on follows later calls."""
        on = terms is not None and any(float(terms.scale[i]) != 0.0 for i in range(NXTERM))
        if on and self.xmetrics is None:
            self.xmetrics = self.torch.zeros(self.nenv, NXTERM, dtype=self.torch.float32, device=self.torch.device("cuda", self.device))
            _chk(self.L.odk_batch_bind_reward_metrics(self._b, _ptr(self.xmetrics)))
        _chk(self.L.odk_batch_set_reward_terms(self._b, C.byref(terms) if terms is not None else None))
        self.reward_terms_on = on

    def set_imitation_joints(self, seq):
        """Joint map of the imitation reward (`odk_batch_set_imitation_joints`): entry u is the reference-motion frame joint actuator u is
        compared with, -1 for an actuator the reward leaves out (reference_motion.imitation_joint_map makes one).  Synchronous; a graph
        captured earlier follows it.  OdkError for a map of the wrong length, an entry outside [-1, 15] or a frame joint used twice."""
        m = np.ascontiguousarray(np.asarray(seq).reshape(-1), np.int32)
        _chk(self.L.odk_batch_set_imitation_joints(self._b, m.ctypes.data_as(C.POINTER(C.c_int32)), len(m)))

    def set_head_joints(self, seq):
        """Head joints of the Standing task (`odk_batch_set_head_joints`): entry k is the actuator that posture command k tracks (neck_pitch,
        head_pitch, head_yaw, head_roll), -1 for a slot with no joint (standing.head_joint_map makes one).  Synchronous; a graph captured earlier
        follows it.  OdkError for a map that is not 4 entries long, an entry outside [-1, nu - 1] or an actuator used twice."""
        m = np.ascontiguousarray(np.asarray(seq).reshape(-1), np.int32)
        _chk(self.L.odk_batch_set_head_joints(self._b, m.ctypes.data_as(C.POINTER(C.c_int32)), len(m)))

    def tracking_accumulate(self, acc):
        """One `odk_tracking_accumulate` launch over this step's outputs into `acc` ([nenv, TRACK_NACC] float32, zeroed before
        the first step); needs bound commands."""
        torch = self.torch
        assert acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous() and tuple(acc.shape) == (self.nenv, TRACK_NACC)
        if self.commands is None:
            raise OdkError("tracking_accumulate: no commands bound (bind_commands)")
        _chk(self.L.odk_tracking_accumulate(self._b, _ptr(self.priv), _ptr(self.reward), _ptr(self.done), _ptr(self.truncation), _ptr(acc), self._stream()))

    def push_accumulate(self, acc, track_acc, lin_tol: float, ang_tol: float):
        """One `odk_push_accumulate` launch over this step's outputs into `acc` ([nenv, PUSH_NACC] float32, zeroed before the first
        step), issued after `step` and BEFORE `tracking_accumulate(track_acc)`; needs bound commands and bound pushes."""
        _check_report(self, "push_accumulate", acc, PUSH_NACC, track_acc)
        if self.commands is None:
            raise OdkError("push_accumulate: no commands bound (bind_commands)")
        if self.pushes is None:
            raise OdkError("push_accumulate: no pushes bound (bind_pushes)")
        _chk(self.L.odk_push_accumulate(self._b, *_report_ptrs(self, track_acc), float(lin_tol), float(ang_tol), _ptr(acc), self._stream()))

    def gait_accumulate(self, acc, track_acc, torque_limit=None):
        """One `odk_gait_accumulate` launch over this step's outputs into `acc` ([nenv, GAIT_NACC] float32, zeroed before the first step),
        issued after `step` and BEFORE `tracking_accumulate(track_acc)`.  `torque_limit`: float32 [nu] on the batch's device (an entry <= 0:
        that actuator never counts as saturated) or None (nobody does).  Needs neither bound commands nor bound pushes."""
        _check_report(self, "gait_accumulate", acc, GAIT_NACC, track_acc)
        limit = _check_torque_limit(self, "gait_accumulate", torque_limit)
        _chk(self.L.odk_gait_accumulate(self._b, *_report_ptrs(self, track_acc), limit, _ptr(acc), self._stream()))

    def posture_accumulate(self, acc, track_acc, tol: float):
        """One `odk_posture_accumulate` launch over this step's outputs into `acc` ([nenv, POSTURE_NACC] float32, zeroed before the first
        step), issued after `step` and BEFORE `tracking_accumulate(track_acc)`.  `tol`: the head error in radians above which a sample counts
        as not settled (finite, >= 0).  Needs bound commands and a head-joint map (the duck has one; `set_head_joints` otherwise)."""
        _check_report(self, "posture_accumulate", acc, POSTURE_NACC, track_acc)
        if self.commands is None:
            raise OdkError("posture_accumulate: no commands bound (bind_commands)")
        _chk(self.L.odk_posture_accumulate(self._b, *_report_ptrs(self, track_acc), float(tol), _ptr(acc), self._stream()))

    def imitation_accumulate(self, acc, track_acc, period_steps: int):
        """One `odk_imitation_accumulate` launch over this step's outputs into `acc` ([nenv, IMIT_NACC] float32, zeroed before the first
        step), issued after `step` and BEFORE `tracking_accumulate(track_acc)`.  `period_steps`: the reference motion's nb_steps_in_period
        (touchdown lags past half of it count as early for the next cycle), or 0 for lags that are not folded.  A Joystick batch that runs
        the imitation reward with a joint map (the duck has one; `set_imitation_joints` otherwise); needs no bound commands."""
        _check_report(self, "imitation_accumulate", acc, IMIT_NACC, track_acc)
        if int(period_steps) != period_steps:
            raise OdkError(f"imitation_accumulate: period_steps = {period_steps!r} (a whole number of steps)")
        _chk(self.L.odk_imitation_accumulate(self._b, *_report_ptrs(self, track_acc), int(period_steps), _ptr(acc), self._stream()))

    def command_schedule_apply(self, sched, sched_of_env, track_acc):
        """One `odk_command_schedule_apply` launch, issued BEFORE `step`: env e's row of the bound command tensor becomes the command of the
        segment of schedule `sched_of_env[e]` in force at the first-episode step about to run (`track_acc`'s STEPS slot is the clock; a zeroed
        `track_acc` gives segment 0, what `reset` must find).  `sched`: float32 [nsched, nseg <= SCHED_MAX_SEGMENTS, SCHED_SEG_FLOATS] (start_step
        and the 7 command entries per segment, padded with SCHED_NEVER starts); `sched_of_env`: int32 [nenv].  Needs bound commands."""
        nsched, nseg = check_schedule("command_schedule_apply", sched, sched_of_env, self.nenv, self.device)
        check_accumulator("command_schedule_apply: track_acc", track_acc, self.nenv, TRACK_NACC, self.device)
        if self.commands is None:
            raise OdkError("command_schedule_apply: no commands bound (bind_commands)")
        _chk(self.L.odk_command_schedule_apply(self._b, _ptr(sched), nsched, nseg, _ptr(sched_of_env), _ptr(track_acc), self._stream()))

    def response_accumulate(self, acc, track_acc, sched, sched_of_env, lin_tol: float, ang_tol: float, tail_after: int):
        """One `odk_response_accumulate` launch over this step's outputs into `acc` ([nenv, RESP_NACC] float32, zeroed before the first step:
        one block of RESP_STRIDE floats per segment), issued after `step` and BEFORE `tracking_accumulate(track_acc)`, with the schedule that
        `command_schedule_apply` wrote this step's commands from.  `lin_tol` / `ang_tol`: the planar velocity error (m/s) and yaw-rate error
        (rad/s) up to which a sample counts as following the command (finite, >= 0); `tail_after`: the samples past this many steps of a
        segment are its steady state.  Needs bound commands."""
        _check_report(self, "response_accumulate", acc, RESP_NACC, track_acc)
        nsched, nseg = check_schedule("response_accumulate", sched, sched_of_env, self.nenv, self.device)
        if int(tail_after) != tail_after:
            raise OdkError(f"response_accumulate: tail_after = {tail_after!r} (a whole number of steps)")
        if self.commands is None:
            raise OdkError("response_accumulate: no commands bound (bind_commands)")
        _chk(self.L.odk_response_accumulate(self._b, *_report_ptrs(self, track_acc), _ptr(sched), nsched, nseg, _ptr(sched_of_env),
                                            float(lin_tol), float(ang_tol), int(tail_after), _ptr(acc), self._stream()))

    def fall_row_floats(self, ring: int) -> int:
        """Floats of one env's row of the fall recorder with a ring of `ring` samples (`odk_fall_row_floats`): FALL_HEAD + ring * (FALL_SAMPLE +
        nq).  OdkError for a ring outside 1 .. FALL_MAX_RING."""
        if isinstance(ring, bool) or int(ring) != ring or not 1 <= int(ring) <= FALL_MAX_RING:
            raise OdkError(f"fall_row_floats: ring = {ring!r} (a whole number of samples, 1 .. {FALL_MAX_RING})")
        n = int(self.L.odk_fall_row_floats(self._b, int(ring)))
        if n < 0:
            raise OdkError(f"fall_row_floats: ring = {ring!r} refused")
        return n

    def fall_accumulate(self, acc, track_acc, tilt_tol: float, ring: int, torque_limit=None):
        """One `odk_fall_accumulate` launch over this step's outputs into `acc` (float32 [nenv, row_stride] with row_stride >=
        `fall_row_floats(ring)`, zeroed before the first step: per env a head and a ring of its last `ring` samples, frozen when its first
        episode ends), issued after `step` and BEFORE `tracking_accumulate(track_acc)`.  `tilt_tol`: the sine of the lean up to which a sample
        counts as upright (finite, >= 0); `torque_limit` as `gait_accumulate`'s.  Needs bound commands."""
        nfl = self.fall_row_floats(ring)
        if not hasattr(acc, "dim") or acc.dim() != 2 or int(acc.shape[1]) < nfl:
            raise OdkError(f"fall_accumulate: acc: expected a torch tensor [{self.nenv}, >= {nfl}] (fall_row_floats({int(ring)})), got "
                           f"{tuple(acc.shape) if hasattr(acc, 'shape') else type(acc).__name__}")
        _check_report(self, "fall_accumulate", acc, int(acc.shape[1]), track_acc)
        limit = _check_torque_limit(self, "fall_accumulate", torque_limit)
        if self.commands is None:
            raise OdkError("fall_accumulate: no commands bound (bind_commands)")
        _chk(self.L.odk_fall_accumulate(self._b, *_report_ptrs(self, track_acc), limit, float(tilt_tol), int(ring), _ptr(acc), int(acc.shape[1]),
                                        self._stream()))

    def path_begin(self, acc):
        """One `odk_path_begin` launch, issued after `reset`: env e's row of `acc` ([nenv, PATH_NACC] float32) is zeroed and takes the base
        pose the reset left as its start pose (PATH_START_*) and as its last sample (PATH_X ..): every later pose quantity is in that frame."""
        check_accumulator("path_begin: acc", acc, self.nenv, PATH_NACC, self.device)
        _chk(self.L.odk_path_begin(self._b, _ptr(acc), self._stream()))

    def path_accumulate(self, acc, track_acc, course=None, course_of_env=None, radius: float = 0.0):
        """One `odk_path_accumulate` launch over this step's state into `acc` ([nenv, PATH_NACC] float32, begun by `path_begin`), issued
        after `step` and BEFORE `tracking_accumulate(track_acc)`: path length, heading change and the last pose of every env in its first
        episode.  `course` (float32 [ncourse, PATH_COURSE_FLOATS]: count, then the points in start-frame metres) with `course_of_env` (int32
        [nenv]) adds the course progress: the waypoint reached within `radius` metres (finite, >= 0), the cross-track distance and the
        distance to the goal.  Without a course it is the plain odometry.  Needs no bound commands."""
        _check_report(self, "path_accumulate", acc, PATH_NACC, track_acc)
        if course is None and course_of_env is not None:
            raise OdkError("path_accumulate: course_of_env without a course")
        ncourse = 0 if course is None else check_courses("path_accumulate", course, course_of_env, self.nenv, self.device)
        radius = check_path_parameter("path_accumulate", "radius", radius)
        _chk(self.L.odk_path_accumulate(self._b, _ptr(self.done), _ptr(self.truncation), _ptr(track_acc), _ptr(course), ncourse,
                                        _ptr(course_of_env), radius, _ptr(acc), self._stream()))

    def waypoint_command_apply(self, course, course_of_env, track_acc, path_acc, v_cruise: float, turn_rate: float, heading_gain: float,
                               slow_dist: float):
        """One `odk_waypoint_command_apply` launch, issued BEFORE `step`: entries 0..2 (vx, vy, wz) of env e's row of the bound command
        tensor steer it towards waypoint PATH_WP_INDEX of its course -- forward at `v_cruise` (m/s, >= 0) times the cosine of the heading
        error, turning at `heading_gain` (> 0) times its sine, clamped to `turn_rate` (rad/s, >= 0), slowing down inside `slow_dist`
        (metres, > 0) of the last waypoint; zeros once the course is finished.  `track_acc`'s STEPS slot is the clock: a zeroed one takes the
        start pose as the pose, what the launch before `reset` needs.  `path_acc`: `path_accumulate`'s.  Needs bound commands."""
        ncourse = check_courses("waypoint_command_apply", course, course_of_env, self.nenv, self.device)
        check_accumulator("waypoint_command_apply: track_acc", track_acc, self.nenv, TRACK_NACC, self.device)
        check_accumulator("waypoint_command_apply: path_acc", path_acc, self.nenv, PATH_NACC, self.device)
        fn = "waypoint_command_apply"
        args = (check_path_parameter(fn, "v_cruise", v_cruise), check_path_parameter(fn, "turn_rate", turn_rate),
                check_path_parameter(fn, "heading_gain", heading_gain, True), check_path_parameter(fn, "slow_dist", slow_dist, True))
        if self.commands is None:
            raise OdkError("waypoint_command_apply: no commands bound (bind_commands)")
        _chk(self.L.odk_waypoint_command_apply(self._b, _ptr(course), ncourse, _ptr(course_of_env), _ptr(track_acc), _ptr(path_acc), *args,
                                               self._stream()))

    def _apply_stage(self, fn: str, src_name: str, src_what: str, src, ncol: int, done, fault, nprm: int, state, nstate: int, out):
        """The out-of-place stages `sensor_apply` / `action_apply`: `out` <- `src` (both [nenv, ncol]) under `fault` ([nenv, nprm]) with `state`
        ([nenv, nstate]) and `done` ([nenv] or None), refused in this order, then the one `odk_<fn>` launch."""
        import torch
        for what, t, n in ((src_name, src, ncol), ("out", out, ncol), ("fault", fault, nprm), ("state", state, nstate)):
            check_accumulator(f"{fn}: {what}", t, self.nenv, n, self.device)
        if done is not None:
            if not torch.is_tensor(done) or tuple(done.shape) != (self.nenv,):
                raise OdkError(f"{fn}: done: expected a torch tensor of shape ({self.nenv},) or None, got "
                               f"{tuple(done.shape) if hasattr(done, 'shape') else type(done).__name__}")
            _check_placement(f"{fn}: done", done, torch.float32, self.device)
        lo, hi = src.data_ptr(), src.data_ptr() + src.numel() * 4
        if out is src or (out.data_ptr() < hi and lo < out.data_ptr() + out.numel() * 4):
            raise OdkError(f"{fn}: out shares memory with {src_name} (the stage is out of place: {src_what} is only read)")
        if self.model.nu > 16:
            raise OdkError(f"{fn}: the model has {self.model.nu} actuators, a row holds 16")
        _chk(getattr(self.L, "odk_" + fn)(self._b, _ptr(src), _ptr(done), _ptr(fault), _ptr(state), _ptr(out), self._stream()))

    @staticmethod
    def sensor_fault_rows(n: int) -> np.ndarray:
        """`sensor_fault_rows(n)`: [n, SENSOR_NPRM] float32 all-nominal fault rows to fill in."""
        return sensor_fault_rows(n)

    def sensor_apply(self, obs, done, fault, state, out):
        """One `odk_sensor_apply` launch: `out` ([nenv, nobs] float32) <- `obs` (the step's observation, only read) as env e's faulty sensors
        would deliver it -- `fault` ([nenv, SENSOR_NPRM], `sensor_fault_rows` to fill in) names the fault, `state` ([nenv, SENSOR_NSTATE], zeroed
        before an episode's first call) holds the ring of raw samples the delays read, `done` ([nenv], or None) refills it.  Gyro,
        accelerometer, joint positions and velocities and the two contacts are touched, every other column is copied bit for bit, and an
        all-nominal `fault` copies the whole row bit for bit.  `out` must not share memory with `obs`."""
        self._apply_stage("sensor_apply", "obs", "the step's observation", obs, self.nobs, done, fault, SENSOR_NPRM, state, SENSOR_NSTATE, out)

    @staticmethod
    def action_fault_rows(n: int) -> np.ndarray:
        """`action_fault_rows(n)`: [n, ACT_NPRM] float32 all-nominal fault rows to fill in."""
        return action_fault_rows(n)

    def action_apply(self, act, done, fault, state, out):
        """One `odk_action_apply` launch: `out` ([nenv, nu] float32, what `step` is then given) <- `act` (the policy's action, only read) as
        env e's link to its servos would deliver it -- `fault` ([nenv, ACT_NPRM], `action_fault_rows` to fill in; action units) names the
        fault, `state` ([nenv, ACT_NSTATE], zeroed before an episode's first call) holds the step and episode counts, the loss run, the
        filter's state and the action last delivered, `done` ([nenv], or None) starts a new episode.  An all-nominal `fault` copies every
        bit.  `out` must not share memory with `act`."""
        self._apply_stage("action_apply", "act", "the policy's action", act, int(self.model.nu), done, fault, ACT_NPRM, state, ACT_NSTATE, out)

    def fault_resample(self, done, spec, seed: int, env_id_offset: int, state, sensor_fault, act_fault):
        """One `odk_fault_resample` launch, issued BEFORE `sensor_apply` and `action_apply` of the same step with the same `done`: every env
        whose `state` row ([nenv, FAULT_NSTATE], zeroed before an episode's first call) has HEAD 0 or whose `done` ([nenv], or None) is set
        gets its rows of `sensor_fault` ([nenv, SENSOR_NPRM]) and `act_fault` ([nenv, ACT_NPRM]) redrawn from `spec` ([3, FAULT_NSLOT]: lo,
        hi, kind = FAULT_FIXED / FAULT_UNIFORM / FAULT_WHOLE per slot); the other envs' rows keep their bits.  The draws are a stateless
        hash of (`seed`, `env_id_offset` + e, the env's redraw count, the slot): both are whole numbers below 2^32."""
        import torch
        fn = "fault_resample"
        for what, t, n in (("state", state, FAULT_NSTATE), ("sensor_fault", sensor_fault, SENSOR_NPRM), ("act_fault", act_fault, ACT_NPRM)):
            check_accumulator(f"{fn}: {what}", t, self.nenv, n, self.device)
        _check_tensor(f"{fn}: spec", spec, "float32", self.device, f"(3, {FAULT_NSLOT})", lambda s: s == (3, FAULT_NSLOT))
        if done is not None:
            if not torch.is_tensor(done) or tuple(done.shape) != (self.nenv,):
                raise OdkError(f"{fn}: done: expected a torch tensor of shape ({self.nenv},) or None, got "
                               f"{tuple(done.shape) if hasattr(done, 'shape') else type(done).__name__}")
            _check_placement(f"{fn}: done", done, torch.float32, self.device)
        for name, v in (("seed", seed), ("env_id_offset", env_id_offset)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 1 << 32:
                raise OdkError(f"{fn}: {name} = {v!r} (a whole number, 0 .. 2^32 - 1)")
        _chk(self.L.odk_fault_resample(self._b, _ptr(done), _ptr(spec), int(seed), int(env_id_offset), _ptr(state), _ptr(sensor_fault),
                                       _ptr(act_fault), self._stream()))

    def _curriculum_ints(self, fn: str, cur, **arrays) -> int:
        """The checks the two curriculum launches share: `cur` a `Curriculum` with a grid in range, every array a contiguous int32 tensor of
        its shape on the batch's device.  Returns nbins."""
        if not isinstance(cur, Curriculum):
            raise OdkError(f"{fn}: curriculum: expected an engine.Curriculum, got {type(cur).__name__}")
        try:
            nbins = curriculum_nbins(cur)
        except OdkError as e:
            raise OdkError(f"{fn}: {e}")
        shapes = dict(levels=(nbins,), cdf=(nbins,), counts=(nbins, 2), stats=(4,))
        for what, t in arrays.items():
            _check_tensor(f"{fn}: {what}", t, "int32", self.device, str(shapes[what]), lambda s, w=shapes[what]: s == w)
        return nbins

    def curriculum_step(self, cur, priv, done, truncation, cdf, counts, state, cmd, obs=None, patch_priv: bool = True):
        """One `odk_curriculum_step` launch, issued AFTER `step`: per env the velocity sample of the step against the command it ran under,
        the judgement of a stint that ends (integer atomics on `counts` [nbins, 2]) and the draw of the next command from `cdf` ([nbins]
        int32) into `cmd` -- which must be the tensor bound with `bind_commands` -- and into floats 6 .. 12 of `obs` ([nenv, nobs] or
        None) and, with `patch_priv`, of `priv` ([nenv, npriv]: the step's privileged observation, whose noise-free velocities are read).
        `state`: [nenv, CURR_NSTATE], zeroed before the first call, on which every env draws.  `done` / `truncation`: [nenv], or both None
        (no stint ends but by `period`)."""
        import torch
        fn = "curriculum_step"
        self._curriculum_ints(fn, cur, cdf=cdf, counts=counts)
        check_accumulator(f"{fn}: state", state, self.nenv, CURR_NSTATE, self.device)
        check_accumulator(f"{fn}: priv", priv, self.nenv, self.npriv, self.device)
        if obs is not None:
            check_accumulator(f"{fn}: obs", obs, self.nenv, self.nobs, self.device)
        _check_tensor(f"{fn}: cmd", cmd, "float32", self.device, f"({self.nenv}, {NCOMMAND})", lambda s: s == (self.nenv, NCOMMAND))
        if self.commands is None or cmd.data_ptr() != self.commands.data_ptr():
            raise OdkError(f"{fn}: cmd is not the tensor bound to the batch (bind_commands)")
        if (done is None) != (truncation is None):
            raise OdkError(f"{fn}: done and truncation come together: both tensors or both None")
        for what, t in (("done", done), ("truncation", truncation)):
            if t is not None:
                _check_tensor(f"{fn}: {what}", t, "float32", self.device, f"({self.nenv},)", lambda s: s == (self.nenv,), " or None")
        for name, lo in (("period", 1), ("skip", 0), ("min_samples", 0)):
            if int(getattr(cur, name)) < lo:
                raise OdkError(f"{fn}: {name} = {int(getattr(cur, name))} (at least {lo})")
        _chk(self.L.odk_curriculum_step(self._b, C.byref(cur), _ptr(priv), _ptr(done), _ptr(truncation), _ptr(cdf), _ptr(counts), _ptr(state),
                                        _ptr(cmd), _ptr(obs), _ptr(priv) if patch_priv else None, self._stream()))

    def curriculum_update(self, cur, levels, cdf, counts, stats):
        """One `odk_curriculum_update` launch (one wave): judges every bin of `counts` with `min_tries` tries, raises `levels` ([nbins] int32)
        by the promoted bins among a bin and its axis neighbours up to CURR_LMAX, zeroes the judged counters, rebuilds `cdf` as the
        inclusive prefix sums and advances `stats` ([4] int32)."""
        fn = "curriculum_update"
        self._curriculum_ints(fn, cur, levels=levels, cdf=cdf, counts=counts, stats=stats)
        if int(cur.min_tries) < 1:
            raise OdkError(f"{fn}: min_tries = {int(cur.min_tries)} (at least 1)")
        _chk(self.L.odk_curriculum_update(self._b, C.byref(cur), _ptr(levels), _ptr(cdf), _ptr(counts), _ptr(stats), self._stream()))

    def log_apply(self, log, track_acc, action):
        """One `odk_log_apply` launch, issued BEFORE `step`: `action` ([nenv, nu] float32, what `step` is then given) and entries 0..6 of the
        bound command tensor become the action and the command of row min(k, nrow - 1) of `log` ([nrow, log_row(nu)] float32), k the
        first-episode step about to run (`track_acc`'s STEPS slot, `command_schedule_apply`'s clock).  Needs bound commands."""
        nrow = check_log_table("log_apply", log, self.model.nu, self.device)
        check_accumulator("log_apply: track_acc", track_acc, self.nenv, TRACK_NACC, self.device)
        check_accumulator("log_apply: action", action, self.nenv, self.model.nu, self.device)
        if self.commands is None:
            raise OdkError("log_apply: no commands bound (bind_commands)")
        _chk(self.L.odk_log_apply(self._b, _ptr(log), nrow, _ptr(track_acc), _ptr(action), self._stream()))

    def replay_accumulate(self, acc, track_acc, log):
        """One `odk_replay_accumulate` launch over this step's outputs into `acc` ([nenv, 16, REPLAY_NSLOT] float32, zeroed before the first
        step), issued after `step` and BEFORE `tracking_accumulate(track_acc)`: the residuals of the step that just ran against its row of
        `log`, the table `log_apply` took the step's action from.  Needs no bound commands."""
        _check_tensor("replay_accumulate: acc", acc, "float32", self.device, f"({self.nenv}, 16, {REPLAY_NSLOT})",
                      lambda s: s == (self.nenv, 16, REPLAY_NSLOT))
        check_accumulator("replay_accumulate: track_acc", track_acc, self.nenv, TRACK_NACC, self.device)
        nrow = check_log_table("replay_accumulate", log, self.model.nu, self.device)
        _chk(self.L.odk_replay_accumulate(self._b, *_report_ptrs(self, track_acc), _ptr(log), nrow, _ptr(acc), self._stream()))

    def physics_step(self, ctrl, n_substeps: int = 10):
        assert ctrl.is_cuda and ctrl.dtype == self.torch.float32 and ctrl.is_contiguous() and tuple(ctrl.shape) == (self.nenv, self.model.nu)
        _chk(self.L.odk_physics_step(self._b, _ptr(ctrl), n_substeps, self._stream()))

    # -- synchronous host access (tests, checkpoints)
    def get_state(self):
        qpos = np.zeros((self.nenv, self.model.nq), np.float32); qvel = np.zeros((self.nenv, self.model.nv), np.float32)
        warm = np.zeros((self.nenv, self.model.nv), np.float32)
        _chk(self.L.odk_batch_get_state(self._b, _fp(qpos), _fp(qvel), _fp(warm)))
        return qpos, qvel, warm

    def set_state(self, qpos=None, qvel=None, warm=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (qpos, qvel, warm)]
        _chk(self.L.odk_batch_set_state(self._b, *[None if a is None else _fp(a) for a in arrs]))

    def get_debug(self):
        s = np.zeros((self.nenv, 46), np.float32); a = np.zeros((self.nenv, self.model.nu), np.float32)
        c = np.zeros((self.nenv, 12), np.float32); q = np.zeros((self.nenv, self.model.nv), np.float32)
        _chk(self.L.odk_batch_get_debug(self._b, _fp(s), _fp(a), _fp(c), _fp(q)))
        return dict(sensordata=s, actuator_force=a, contact_dist=c, qacc=q)

    def lds_image(self) -> np.ndarray:
        n = self.L.odk_batch_lds_size(self._b)
        img = np.zeros((self.nenv, n), np.float32)
        _chk(self.L.odk_batch_get_lds(self._b, _fp(img)))
        return img

    def lds_offset(self, name: str) -> int:
        off = self.L.odk_lds_offset(self._b, name.encode())
        if off < 0:
            raise KeyError(name)
        return off

    def records(self) -> np.ndarray:
        n = self.L.odk_batch_record_size(self._b)
        r = np.zeros((self.nenv, n), np.float32)
        _chk(self.L.odk_batch_get_records(self._b, _fp(r)))
        return r

    def set_records(self, records: np.ndarray):
        r = np.ascontiguousarray(records, np.float32)
        assert r.shape == (self.nenv, self.L.odk_batch_record_size(self._b))
        self.generation += 1
        _chk(self.L.odk_batch_set_records(self._b, _fp(r)))

    INFO_FIELDS = ("rng", "step", "command", "last_act", "last_last_act", "last_last_last_act", "motor_targets", "feet_air_time", "last_contact",
                   "swing_peak", "push", "push_step", "push_interval_steps", "action_history", "imu_history", "imitation_i",
                   "steps", "truncation", "episode_done", "episode_metrics/sum_reward", "episode_metrics/length", "episode_metrics/reward_terms")

    def record_field(self, name: str):
        """(offset, count, kind) of a named field inside a record (`odk_record_field`; kind 0 float32, 1 int32, 2 bit mask)."""
        o, n, k = C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(self.L.odk_record_field(self._b, name.encode(), C.byref(o), C.byref(n), C.byref(k)))
        return o.value, n.value, k.value

    def info(self, records: np.ndarray = None) -> dict:
        """The carried `info` dict of the reference's State (joystick.py:278-302 + the wrapper's additions), one [nenv, ...] array per
        key, as VIEWS over a host copy of the records (`records()` when none is passed): write through a view, then hand the
        same array to `set_records` to preset a field.  int32 fields come as int32 views; `last_contact` as the packed mask
        (bit f = foot f), with `last_contact_bool(info)` for the reference's bool[2]."""
        r = self.records() if records is None else records
        ri = r.view(np.int32)
        out = {"_records": r}
        for name in self.INFO_FIELDS:
            o, n, k = self.record_field(name)
            v = (r if k == 0 else ri)[:, o:o + n]
            out[name] = v[:, 0] if n == 1 else v
        return out

    @staticmethod
    def last_contact_bool(info: dict) -> np.ndarray:
        m = info["last_contact"]
        return np.stack([(m & 1) != 0, (m & 2) != 0], axis=1)

    def timing(self, enable):
        """Average kernel milliseconds of the timed launches since the last call; `enable`: False / 0 = off, True / 1 = time every
        launch from now on, n = every n-th launch (`odk_batch_timing`)."""
        ms, n = C.c_float(0), C.c_int(0)
        _chk(self.L.odk_batch_timing(self._b, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if getattr(self, "_b", None):
            self.L.odk_batch_destroy(self._b); self._b = None
        if getattr(self, "_m", None):
            self.L.odk_model_free(self._m); self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
