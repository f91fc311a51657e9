"""Env configurations away from `odk_default_config()`, shared by tests/test_env_config_host.py (oracle alone) and
tests/test_gpu_env_config.py (env kernels against the oracle).  Plain module: no fixtures, no GPU.

A case is a dict from field name to value in the vocabulary of `odk_env_config` (include/odk.h).  `apply_engine` writes it into an
`engine.EnvConfig`, `apply_oracle` into an `OracleEnv.cfg`; the two writers share nothing but the dict -- every array is written out on each
side in that side's own layout, so a layout slip on one side is not mirrored on the other.  Values travel as float32 on both sides (the
format of `odk_env_config`): the oracle computes in float64 from the same float32 numbers the kernels read.

What a case has to satisfy is checked by `check_case` / `check_case_set` (run by the host tests):
  * no two float values of a case are equal and none equals its default -- except `ctrl_dt` of a 10-substep case (it must equal
    n_substeps * sim_dt = 0.02, the default), `push_enable` (a switch: 1.0) and the first three `cmd_range` rows of a Standing case (zero, as
    `odk_default_config_standing` sets them: the Standing task has no move command);
  * all 16 `qpos_noise_scale` slots distinct and non-zero; all seven `cmd_range` rows asymmetric (Standing: the last four);
  * `ctrl_dt == n_substeps * SIM_DT`; `push_interval_range[0] / ctrl_dt >= 1` (neither side may ever take `% 0`);
  * magnitudes within about a factor 2 of the defaults (the push interval apart: it is short ON PURPOSE, so that the built-in push fires many
    times inside a 36-step run -- at the defaults it fires every 250..500 steps and no parity run ever sees it);
  * over the set: n_substeps 4, 7 and 10; the motor speed limit off (with a non-zero max_motor_velocity) and on; autoreset off and on; a noise
    level strictly inside (0, 1); every reward slot once positive and once negative."""
import numpy as np

SIM_DT = 0.002          # the models' <option timestep>: ctrl_dt = n_substeps * SIM_DT
EPISODE_LENGTH = 17     # two truncations per env inside a 36-step run

FLOAT_SCALARS = ("ctrl_dt", "action_scale", "dof_vel_scale", "max_motor_velocity", "noise_level", "noise_gyro", "noise_accelerometer", "noise_gravity",
                 "noise_joint_vel", "tracking_sigma", "push_enable", "reset_base_qvel")
FLOAT_ARRAYS = {"qpos_noise_scale": 16, "reward_scales": 7, "push_interval_range": 2, "push_magnitude_range": 2, "cmd_range": 14}
INT_FIELDS = ("use_imitation", "use_motor_speed_limits", "autoreset", "episode_length", "n_substeps")

# odk_default_config / odk_default_config_standing, written out (tests/test_capi_and_model.py holds the library to the same numbers)
DEFAULTS = dict(
    ctrl_dt=0.02, action_scale=0.25, dof_vel_scale=0.05, max_motor_velocity=5.24, noise_level=1.0, noise_gyro=0.1, noise_accelerometer=0.05,
    noise_gravity=0.1, noise_joint_vel=2.5, qpos_noise_scale=[0.03, 0.03, 0.03, 0.05, 0.08, 0.03, 0.03, 0.03, 0.05, 0.08, 0, 0, 0, 0, 0, 0],
    reward_scales=[2.5, 6.0, -1.0e-3, -0.5, -0.2, 20.0, 1.0], tracking_sigma=0.01, push_enable=1.0, push_interval_range=[5.0, 10.0],
    push_magnitude_range=[0.1, 1.0], cmd_range=[[-0.15, 0.15], [-0.2, 0.2], [-1.0, 1.0], [-0.34, 1.1], [-0.78, 0.78], [-1.5, 1.5], [-0.5, 0.5]],
    use_imitation=1, use_motor_speed_limits=1, autoreset=1, episode_length=1000, n_substeps=10, reset_base_qvel=0.05)
DEFAULTS_STANDING = dict(
    DEFAULTS, max_motor_velocity=0.0, noise_gyro=0.05, noise_accelerometer=0.005, reward_scales=[-0.5, -2.0, -1.0e-3, -0.375, -0.3, 20.0, 0.0],
    cmd_range=[[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [-0.34, 1.1], [-0.78, 0.78], [-2.7, 2.7], [-0.5, 0.5]],
    use_imitation=0, use_motor_speed_limits=0, reset_base_qvel=0.5)

CASES = {
    # 10 substeps, motor speed limit on, noise level 0.6.  Reward signs + - + - + + +.
    "s10": dict(
        ctrl_dt=0.02, n_substeps=10, action_scale=0.41, dof_vel_scale=0.072, max_motor_velocity=3.1, noise_level=0.6, noise_gyro=0.13,
        noise_accelerometer=0.097, noise_gravity=0.17, noise_joint_vel=1.9,
        qpos_noise_scale=[0.018, 0.023, 0.038, 0.043, 0.048, 0.053, 0.058, 0.063, 0.068, 0.073, 0.078, 0.083, 0.088, 0.093, 0.098, 0.103],
        reward_scales=[1.7, -4.0, 2.0e-3, -0.33, 0.35, 12.0, 0.55], tracking_sigma=0.024, push_enable=1.0, push_interval_range=[0.05, 0.21],
        push_magnitude_range=[0.22, 0.7],
        cmd_range=[[-0.06, 0.2], [-0.31, 0.1], [-0.4, 1.3], [-0.22, 0.9], [-0.5, 0.85], [-1.1, 0.62], [-0.72, 0.25]],
        use_imitation=1, use_motor_speed_limits=1, autoreset=1, episode_length=EPISODE_LENGTH, reset_base_qvel=0.11),
    # 4 substeps, motor speed limit OFF beside a non-zero max_motor_velocity, noise level 0.5.  Reward signs - + - + - + -.
    "s4": dict(
        ctrl_dt=0.008, n_substeps=4, action_scale=0.17, dof_vel_scale=0.086, max_motor_velocity=7.3, noise_level=0.5, noise_gyro=0.075,
        noise_accelerometer=0.092, noise_gravity=0.14, noise_joint_vel=3.6,
        qpos_noise_scale=[0.077, 0.065, 0.071, 0.089, 0.101, 0.041, 0.023, 0.059, 0.035, 0.095, 0.017, 0.107, 0.029, 0.083, 0.047, 0.053],
        reward_scales=[-1.3, 3.5, -1.8e-3, 0.8, -0.37, 27.0, -1.7], tracking_sigma=0.006, push_enable=1.0, push_interval_range=[0.03, 0.1],
        push_magnitude_range=[0.15, 1.45],
        cmd_range=[[-0.2, 0.07], [-0.12, 0.33], [-1.6, 0.52], [-0.6, 0.47], [-0.95, 0.42], [-0.8, 2.1], [-0.28, 0.74]],
        use_imitation=1, use_motor_speed_limits=0, autoreset=1, episode_length=EPISODE_LENGTH, reset_base_qvel=0.031),
    # 7 substeps, motor speed limit on, noise level 0.8.  Reward signs + + - - + - + (a negative `alive`).
    "s7": dict(
        ctrl_dt=0.014, n_substeps=7, action_scale=0.32, dof_vel_scale=0.036, max_motor_velocity=8.4, noise_level=0.8, noise_gyro=0.19,
        noise_accelerometer=0.09, noise_gravity=0.055, noise_joint_vel=4.4,
        qpos_noise_scale=[0.02, 0.041, 0.062, 0.035, 0.056, 0.026, 0.05, 0.023, 0.044, 0.065, 0.038, 0.059, 0.032, 0.053, 0.029, 0.047],
        reward_scales=[3.9, 8.5, -6.0e-4, -0.9, 0.13, -14.0, 1.9], tracking_sigma=0.016, push_enable=1.0, push_interval_range=[0.033, 0.095],
        push_magnitude_range=[0.18, 0.52],
        cmd_range=[[-0.27, 0.11], [-0.09, 0.38], [-0.7, 1.95], [-0.5, 0.66], [-1.4, 0.46], [-2.2, 0.97], [-0.3, 0.82]],
        use_imitation=1, use_motor_speed_limits=1, autoreset=1, episode_length=EPISODE_LENGTH, reset_base_qvel=0.078),
    # the Standing kind (reward slots: orientation, head_pos, torques, action_rate, stand_still, alive, unused); signs + - + - + +
    "standing": dict(
        ctrl_dt=0.02, n_substeps=10, action_scale=0.36, dof_vel_scale=0.064, max_motor_velocity=2.9, noise_level=0.7, noise_gyro=0.085,
        noise_accelerometer=0.028, noise_gravity=0.15, noise_joint_vel=1.4,
        qpos_noise_scale=[0.016, 0.0207, 0.0354, 0.0401, 0.0448, 0.0495, 0.0542, 0.0589, 0.0636, 0.0683, 0.073, 0.0777, 0.0824, 0.0871, 0.0918, 0.0965],
        reward_scales=[0.9, -3.1, 1.6e-3, -0.6, 0.45, 13.0, -0.8], tracking_sigma=0.019, push_enable=1.0, push_interval_range=[0.06, 0.19],
        push_magnitude_range=[0.24, 0.63],
        cmd_range=[[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [-0.25, 0.81], [-0.55, 0.97], [-1.9, 3.3], [-0.75, 0.34]],
        use_imitation=0, use_motor_speed_limits=0, autoreset=1, episode_length=EPISODE_LENGTH, reset_base_qvel=0.33),
}
# 2 substeps (a 250 Hz policy): the 4-substep case with its control step halved, for the robots with box feet (GPU_CASES)
CASES["s2"] = dict(CASES["s4"], ctrl_dt=0.004, n_substeps=2, push_interval_range=[0.013, 0.046])
# the 10-substep case without auto-reset: done envs keep stepping
CASES["s10_no_autoreset"] = dict(CASES["s10"], autoreset=0)
STANDING_CASES = ("standing",)


def is_standing(name):
    return name in STANDING_CASES


def defaults_of(name):
    return DEFAULTS_STANDING if is_standing(name) else DEFAULTS


def apply_engine(cfg, case):
    """writes `case` into an engine.EnvConfig (ctypes mirror of odk_env_config): every field by name, arrays element by element"""
    cfg.ctrl_dt = case["ctrl_dt"]
    cfg.action_scale = case["action_scale"]
    cfg.dof_vel_scale = case["dof_vel_scale"]
    cfg.max_motor_velocity = case["max_motor_velocity"]
    cfg.noise_level = case["noise_level"]
    cfg.noise_gyro = case["noise_gyro"]
    cfg.noise_accelerometer = case["noise_accelerometer"]
    cfg.noise_gravity = case["noise_gravity"]
    cfg.noise_joint_vel = case["noise_joint_vel"]
    for slot in range(16):
        cfg.qpos_noise_scale[slot] = case["qpos_noise_scale"][slot]
    for slot in range(7):
        cfg.reward_scales[slot] = case["reward_scales"][slot]
    cfg.tracking_sigma = case["tracking_sigma"]
    cfg.push_enable = case["push_enable"]
    cfg.push_interval_range[0], cfg.push_interval_range[1] = case["push_interval_range"]
    cfg.push_magnitude_range[0], cfg.push_magnitude_range[1] = case["push_magnitude_range"]
    for row in range(7):
        lo, hi = case["cmd_range"][row]
        cfg.cmd_range[row][0] = lo
        cfg.cmd_range[row][1] = hi
    cfg.use_imitation = case["use_imitation"]
    cfg.use_motor_speed_limits = case["use_motor_speed_limits"]
    cfg.autoreset = case["autoreset"]
    cfg.episode_length = case["episode_length"]
    cfg.n_substeps = case["n_substeps"]
    cfg.reset_base_qvel = case["reset_base_qvel"]
    return cfg


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def apply_oracle(env, case):
    """writes `case` into an OracleEnv's config (`odko_env_cfg`: every field a `real`, cmd_range flat [7 * 2]) -- the float32 value of every
    number, which is what the kernels are given"""
    c = env.cfg
    c["ctrl_dt"][0] = _f32(case["ctrl_dt"]); c["n_substeps"][0] = case["n_substeps"]
    c["action_scale"][0] = _f32(case["action_scale"]); c["dof_vel_scale"][0] = _f32(case["dof_vel_scale"])
    c["max_motor_velocity"][0] = _f32(case["max_motor_velocity"]); c["use_motor_speed_limits"][0] = case["use_motor_speed_limits"]
    c["noise_level"][0] = _f32(case["noise_level"])
    c["noise_gyro"][0] = _f32(case["noise_gyro"]); c["noise_gravity"][0] = _f32(case["noise_gravity"])
    c["noise_accelerometer"][0] = _f32(case["noise_accelerometer"]); c["noise_joint_vel"][0] = _f32(case["noise_joint_vel"])
    q = c["qpos_noise_scale"]
    assert len(q) == 16
    q[:] = _f32(case["qpos_noise_scale"])
    r = c["reward_scales"]
    assert len(r) == 7
    r[:] = _f32(case["reward_scales"])
    c["tracking_sigma"][0] = _f32(case["tracking_sigma"])
    c["push_enable"][0] = _f32(case["push_enable"])
    c["push_interval_range"][:] = _f32(case["push_interval_range"])
    c["push_magnitude_range"][:] = _f32(case["push_magnitude_range"])
    rng = c["cmd_range"]
    assert len(rng) == 14
    rng[0::2] = _f32([row[0] for row in case["cmd_range"]])      # lower ends
    rng[1::2] = _f32([row[1] for row in case["cmd_range"]])      # upper ends
    c["use_imitation"][0] = case["use_imitation"]; c["autoreset"][0] = case["autoreset"]; c["episode_length"][0] = case["episode_length"]
    c["reset_base_qvel"][0] = _f32(case["reset_base_qvel"])
    return env


def float_values(case):
    """[(label, value)] of every float of a case, arrays flattened"""
    out = [(k, float(case[k])) for k in FLOAT_SCALARS]
    for k, n in FLOAT_ARRAYS.items():
        flat = np.asarray(case[k], np.float64).reshape(-1)
        assert len(flat) == n, k
        out += [(f"{k}[{i}]", float(v)) for i, v in enumerate(flat)]
    return out


def check_case(name):
    """the conditions on one case (module docstring); AssertionError names the field"""
    case, dflt, standing = CASES[name], defaults_of(name), is_standing(name)
    assert set(case) == set(FLOAT_SCALARS) | set(FLOAT_ARRAYS) | set(INT_FIELDS), name
    vals, dvals = float_values(case), dict(float_values(dflt))
    allowed_same = {"push_enable"} | ({"ctrl_dt"} if case["n_substeps"] == 10 else set()) | ({f"cmd_range[{i}]" for i in range(6)} if standing else set())
    seen = {}
    for label, v in vals:
        if label in allowed_same:
            continue
        assert np.float32(v) != np.float32(dvals[label]), f"{name}: {label} holds its default {v}"
        assert np.float32(v) not in seen, f"{name}: {label} and {seen[np.float32(v)]} hold the same value {v}"
        seen[np.float32(v)] = label
    assert all(v != 0 for v in case["qpos_noise_scale"]) and len(set(case["qpos_noise_scale"])) == 16
    for i, (lo, hi) in enumerate(case["cmd_range"]):
        if standing and i < 3:
            assert lo == hi == 0.0
        else:
            assert lo < hi and abs(lo + hi) > 0.05 * (hi - lo), f"{name}: cmd_range row {i} is symmetric"
    assert len(set(case["reward_scales"])) == 7
    assert abs(case["ctrl_dt"] - case["n_substeps"] * SIM_DT) < 1e-12, name
    assert case["push_interval_range"][0] / case["ctrl_dt"] >= 1.0 and case["push_interval_range"][0] < case["push_interval_range"][1]
    assert case["push_magnitude_range"][0] < case["push_magnitude_range"][1]
    # the longest interval still fires at least three times in 36 steps
    assert case["push_interval_range"][1] / case["ctrl_dt"] <= 12.5
    for label, v in vals:      # within about a factor 2 of the default (2.5 with the rounding of hand-picked numbers); the push interval apart
        d = dvals[label]
        if label.startswith("push_interval_range") or label in allowed_same or d == 0.0 or label == "ctrl_dt":      # (ctrl_dt follows n_substeps)
            continue
        if standing and label == "noise_accelerometer":
            # Standing's default 0.005 is so small against the accelerometer bound (1e-3 relative to readings of O(1..10) m/s^2) that no value
            # within a factor 2 of it has teeth (tests/test_env_config_host.py); the case stays below the Joystick default 0.05 instead
            assert d < v <= DEFAULTS["noise_accelerometer"]
            continue
        assert 0.39 <= abs(v) / abs(d) <= 2.6, f"{name}: {label} = {v} is not within about a factor 2 of its default {d}"
    for k in ("qpos_noise_scale",):      # slots whose default is 0: inside the range of the non-zero defaults, times 2
        assert all(0.015 <= v <= 0.16 for v in case[k])
    if standing:
        assert 0 < abs(case["max_motor_velocity"]) <= 2 * 5.24 and 0.4 <= abs(case["reward_scales"][6]) <= 2.0


def check_case_set():
    """the coverage the set as a whole has to give"""
    for name in CASES:
        check_case(name)
    J = [c for n, c in CASES.items() if not is_standing(n)]
    assert {c["n_substeps"] for c in CASES.values()} >= {4, 7, 10}
    assert any(c["use_motor_speed_limits"] == 0 and c["max_motor_velocity"] != 0 for c in J) and any(c["use_motor_speed_limits"] == 1 for c in J)
    assert {c["autoreset"] for c in CASES.values()} == {0, 1}
    assert all(0 < c["noise_level"] < 1 for c in CASES.values())
    for slot in range(7):
        signs = {np.sign(c["reward_scales"][slot]) for c in J}
        assert signs == {-1.0, 1.0}, f"reward slot {slot} never changes sign over the Joystick cases"


# ---------------------------------------------------------------------------------------------------------------------------------
# The run both test files make with a case: N_ENVS envs, a reset, then N_STEPS env steps with actions uniform in [-1, 1].
N_ENVS, N_STEPS = 16, 36
# RESET_SEED: of the duck's 16 envs three draw the all-zero command (probability 0.1 each) -- `stand_still` is a cost of a robot that is told to
# stand, so without such an env its reward scale moves nothing (the host tests assert that the run has one)
RESET_SEED, ACTION_SEED = 21, 5
# (task or robot file under tests/assets/, lanes per env asked of the engine, case).  A robot that is not the duck runs without the imitation
# reward (`robot_case`); tail_biped.xml takes its `qpos_noise_scale` from `TAIL_BIPED_QPOS_NOISE`.
GPU_CASES = [
    ("flat_terrain", 32, "s10"),
    ("flat_terrain", 64, "s4"),
    ("flat_terrain_backlash", 32, "s7"),
    ("flat_terrain", 32, "standing"),
    ("rough_terrain_backlash", 32, "s4"),
    # (box feet lying flat tie in the manifold's arg-max steps by construction -- SET_ASIDE_BOX in test_gpu_env.py: at the defaults 9 .. 13 % of
    # these robots' env steps are ill-conditioned.  The fewer substeps an env step has, the fewer such branch points it crosses: measured with the
    # oracle alone 7.1 % at 10 substeps, 4.7 % at 4; the robots run the 2-substep case, which keeps them inside half the duck's cap)
    ("tail_biped.xml", 32, "s2"),
    ("biped_arms.xml", 32, "s2"),
    ("flat_terrain", 32, "s10_no_autoreset"),
]
# tail_biped.xml: actuators 0..4 the left leg (hip yaw / roll / pitch, knee, ankle), 5..9 the tail, 10..14 the right leg.  What
# `joystick.to_engine_config` has to produce from the reference's keys hip_pos / knee_pos / ankle_pos below: each leg joint's scale in its
# ACTUATOR's slot, 0 for the tail.
TAIL_BIPED_NOISE_KEYS = dict(hip_pos=0.026, knee_pos=0.047, ankle_pos=0.069)
TAIL_BIPED_QPOS_NOISE = [0.026, 0.026, 0.026, 0.047, 0.069, 0.0, 0.0, 0.0, 0.0, 0.0, 0.026, 0.026, 0.026, 0.047, 0.069, 0.0]


def robot_case(task, name):
    """the case as a robot file runs it: no imitation reward (no reference motion), and for tail_biped.xml the noise scales by actuator"""
    case = dict(CASES[name])
    if task.endswith(".xml"):
        case["use_imitation"] = 0
    if task == "tail_biped.xml":
        case["qpos_noise_scale"] = list(TAIL_BIPED_QPOS_NOISE)
    return case


# Terminations: an episode of 17 control steps (0.14 .. 0.34 s) is too short for a robot to fall over by itself, so after the reset these envs are
# tipped on the oracle side -- rolled by TIP_ANGLE about the base's x axis with a roll rate of TIP_RATE -- and the re-synchronisation before every
# step carries that state to the GPU: their up-vector crosses the horizontal within a few control steps, the env terminates, and auto-reset hands
# back the first state and observation that each side stored at ITS reset.
TIPPED_ENVS = (3, 11)
TIP_ANGLE, TIP_RATE = 1.45, 6.0


def tip(envs):
    """tips TIPPED_ENVS of a list of freshly reset oracle envs (free joint: qpos[3:7] = w, x, y, z; qvel[3:6] = the local angular velocity)"""
    for i in TIPPED_ENVS:
        d = envs[i].data
        w, x, y, z = (float(v) for v in d["qpos"][3:7])
        c, s = np.cos(0.5 * TIP_ANGLE), np.sin(0.5 * TIP_ANGLE)
        d["qpos"][3:7] = [w * c - x * s, w * s + x * c, y * c + z * s, z * c - y * s]      # q * (c, s, 0, 0)
        d["qvel"][3] = TIP_RATE


def case_key(task, lanes, name):
    """the parity_log key of a GPU case"""
    return f"env_config/{name}/{task}" + ("/lanes64" if lanes == 64 else "")
