"""Joystick task for Open Duck Mini V2 -- batched, device-resident mirror of the reference env.

Same surface as reference playground/open_duck_mini_v2/joystick.py (`Joystick`, `default_config`,
`reset`, `step`, `action_size`, `observation_size`, `dt`, `sim_dt`, `n_substeps`) and base.py
(`mj_model`, `xml_path`), but *batched and stateful on the GPU*: `reset(seed)` / `step(state, action)`
operate on all `num_envs` envs at once and every tensor in `State` is a torch device tensor.  The
brax Vmap / Episode / AutoReset wrappers (reference common/runner.py:117) are fused into the same
kernel launch (config keys `episode_length`, `autoreset`).  All arithmetic happens in csrc/ (HIP).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import numpy as np

from . import constants, engine

USE_IMITATION_REWARD = True       # reference joystick.py:45
USE_MOTOR_SPEED_LIMITS = True     # reference joystick.py:46


class ConfigDict(dict):
    """Tiny ml_collections.ConfigDict stand-in: attribute + item access, nested."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def __deepcopy__(self, memo):
        return ConfigDict({k: copy.deepcopy(v, memo) for k, v in self.items()})


def default_config() -> ConfigDict:
    """reference joystick.py:49-102, key for key."""
    C = ConfigDict
    return C(
        ctrl_dt=0.02, sim_dt=0.002, episode_length=1000, action_repeat=1, action_scale=0.25, dof_vel_scale=0.05, history_len=0,
        soft_joint_pos_limit_factor=0.95, max_motor_velocity=5.24,
        noise_config=C(level=1.0, action_min_delay=0, action_max_delay=3, imu_min_delay=0, imu_max_delay=3,
                       scales=C(hip_pos=0.03, knee_pos=0.05, ankle_pos=0.08, joint_vel=2.5, gravity=0.1, linvel=0.1, gyro=0.1, accelerometer=0.05)),
        reward_config=C(scales=C(tracking_lin_vel=2.5, tracking_ang_vel=6.0, torques=-1.0e-3, action_rate=-0.5, stand_still=-0.2, alive=20.0, imitation=1.0),
                        tracking_sigma=0.01),
        push_config=C(enable=True, interval_range=[5.0, 10.0], magnitude_range=[0.1, 1.0]),
        lin_vel_x=[-0.15, 0.15], lin_vel_y=[-0.2, 0.2], ang_vel_yaw=[-1.0, 1.0], neck_pitch_range=[-0.34, 1.1], head_pitch_range=[-0.78, 0.78],
        head_yaw_range=[-1.5, 1.5], head_roll_range=[-0.5, 0.5], head_range_factor=1.0,
    )


def _merge(cfg: ConfigDict, overrides: Optional[Dict[str, Any]]) -> ConfigDict:
    cfg = copy.deepcopy(cfg)
    for k, v in (overrides or {}).items():
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


REWARD_SLOTS = ("tracking_lin_vel", "tracking_ang_vel", "torques", "action_rate", "stand_still", "alive", "imitation")


def to_engine_config(cfg: ConfigDict, autoreset: bool = True, lanes_per_env: int = 0, standing: bool = False,
                     reward_slots=REWARD_SLOTS, use_imitation: bool = USE_IMITATION_REWARD,
                     use_motor_speed_limits: bool = USE_MOTOR_SPEED_LIMITS, joints_order_no_head=None, leg_actuators=None) -> engine.EnvConfig:
    """reference config -> odk_env_config (include/odk.h).  `joints_order_no_head`: the robot's leg joints in actuator order (what a new robot's
    constants.py sets, reference README.md:74-85); default: the duck's.  `leg_actuators` (constants.Robot.leg_actuators): the actuator index of
    each of those joints -- the kernels index `qpos_noise_scale` by actuator, so a robot whose leg actuators are not the first ones (a tail between
    the legs) needs it; None keeps the reference's index-by-position (the duck, BUG-COMPAT below)."""
    c = engine.default_config(standing)
    c.ctrl_dt, c.action_scale, c.dof_vel_scale = cfg.ctrl_dt, cfg.action_scale, cfg.dof_vel_scale
    c.max_motor_velocity = cfg.get("max_motor_velocity", 0.0)
    n = cfg.noise_config
    if (n.action_min_delay, n.action_max_delay, n.imu_min_delay, n.imu_max_delay) != (0, 3, 0, 3):
        raise ValueError("the kernels implement the reference's delay ring of depth 3")
    c.noise_level, c.noise_gyro, c.noise_accelerometer = n.level, n.scales.gyro, n.scales.accelerometer
    c.noise_gravity, c.noise_joint_vel = n.scales.gravity, n.scales.joint_vel
    # BUG-COMPAT (joystick.py:184-200): indices taken on the 10-entry JOINTS_ORDER_NO_HEAD, written into the 14-entry array
    # A robot that is not the duck: each leg joint's scale goes to that joint's ACTUATOR slot, every other actuator gets 0 (DESIGN, BUG-COMPAT list)
    scale = np.zeros(16, np.float32)
    legs = list(constants.JOINTS_ORDER_NO_HEAD if joints_order_no_head is None else joints_order_no_head)
    slots = list(range(len(legs))) if leg_actuators is None else [int(u) for u in leg_actuators]
    if len(slots) != len(legs):
        raise ValueError(f"leg_actuators has {len(slots)} entries for {len(legs)} leg joints")
    for idx, j in zip(slots, legs):
        if not 0 <= idx < 16:
            continue
        scale[idx] = n.scales.hip_pos if "_hip" in j else (n.scales.knee_pos if "_knee" in j else n.scales.ankle_pos)
    for i in range(16):
        c.qpos_noise_scale[i] = float(scale[i])
    s = cfg.reward_config.scales
    for i, k in enumerate(reward_slots):
        c.reward_scales[i] = float(s[k]) if k is not None else 0.0
    c.tracking_sigma = cfg.reward_config.tracking_sigma
    c.push_enable = 1.0 if cfg.push_config.enable else 0.0
    for i in range(2):
        c.push_interval_range[i] = cfg.push_config.interval_range[i]
        c.push_magnitude_range[i] = cfg.push_config.magnitude_range[i]
    f = cfg.head_range_factor
    zero = [0.0, 0.0]   # Standing has no move command (standing.py:652-654)
    ranges = [cfg.get("lin_vel_x", zero), cfg.get("lin_vel_y", zero), cfg.get("ang_vel_yaw", zero), [cfg.neck_pitch_range[0] * f, cfg.neck_pitch_range[1] * f],
              [cfg.head_pitch_range[0] * f, cfg.head_pitch_range[1] * f], [cfg.head_yaw_range[0] * f, cfg.head_yaw_range[1] * f],
              [cfg.head_roll_range[0] * f, cfg.head_roll_range[1] * f]]
    for i, r in enumerate(ranges):
        c.cmd_range[i][0], c.cmd_range[i][1] = float(r[0]), float(r[1])
    c.use_imitation = int(use_imitation)
    c.use_motor_speed_limits = int(use_motor_speed_limits)
    c.autoreset = int(autoreset)
    c.episode_length = int(cfg.episode_length)
    c.n_substeps = int(round(cfg.ctrl_dt / cfg.sim_dt))
    c.lanes_per_env = lanes_per_env
    # additive key (not in the reference's config): on a height-field floor, prism contacts count only when their normal points up
    c.hfield_up_normals_only = int(bool(cfg.get("hfield_up_normals_only", False)))
    return c


LIBRARY_TERMS = engine.XTERM_NAMES
# parameters of the library terms: keys of reward_config (soft_joint_pos_limit_factor is a top-level key, joystick.py:57); no defaults
# are invented except the one the reference's function signature carries (reward_feet_air_time's thresholds 0.1, 0.5)
REWARD_PARAMS = ("base_height_target", "max_foot_height", "air_time_range", "pose_weights", "soft_joint_pos_limit_factor")
AIR_TIME_RANGE_DEFAULT = (0.1, 0.5)


def active_reward_terms(cfg: ConfigDict, reward_slots=REWARD_SLOTS):
    """The library terms a config turns on: keys of reward_config.scales with a non-zero scale that are library names and not one of
    the env's native slots (those keep their native meaning, e.g. Standing's `orientation`).  Other keys are ignored, as in the reference."""
    s = cfg.reward_config.scales
    native = {k for k in reward_slots if k is not None}
    return [k for k in LIBRARY_TERMS if k not in native and float(s.get(k, 0.0)) != 0.0]


def to_reward_terms(cfg: ConfigDict, nu: int, reward_slots=REWARD_SLOTS) -> Optional[engine.RewardTerms]:
    """reference config -> odk_reward_terms (include/odk.h), or None when no library term is on.  ValueError names a parameter that an
    enabled term needs and the config does not carry (base_height_target, max_foot_height, pose_weights with one weight per actuator,
    soft_joint_pos_limit_factor)."""
    active = active_reward_terms(cfg, reward_slots)
    if not active:
        return None
    rc, s = cfg.reward_config, cfg.reward_config.scales
    t = engine.RewardTerms()
    for i, k in enumerate(LIBRARY_TERMS):
        t.scale[i] = float(s[k]) if k in active else 0.0

    def need(key, *terms, where=rc):
        on = [k for k in terms if k in active]
        if on and where.get(key, None) is None:
            raise ValueError(f"reward term {on[0]} is on but the config has no {key}")
        return bool(on)

    if need("base_height_target", "base_height"):
        t.base_height_target = float(rc.base_height_target)
    if need("max_foot_height", "feet_clearance", "feet_height"):
        t.max_foot_height = float(rc.max_foot_height)
    if "feet_air_time" in active:
        lo, hi = rc.get("air_time_range", None) or AIR_TIME_RANGE_DEFAULT
        t.air_time_range[0], t.air_time_range[1] = float(lo), float(hi)
    if need("soft_joint_pos_limit_factor", "joint_pos_limits", where=cfg):
        t.soft_joint_pos_limit_factor = float(cfg.soft_joint_pos_limit_factor)
    if need("pose_weights", "pose"):
        w = [float(x) for x in rc.pose_weights]
        if len(w) != int(nu):
            raise ValueError(f"reward term pose: pose_weights has {len(w)} entries, the robot has {nu} actuators")
        for i, x in enumerate(w):
            t.pose_weight[i] = x
    return t


def reward_metric_name(key: str, scale: float) -> str:
    """State.metrics key of a library term: reward/<k> or cost/<k> by the sign of its scale."""
    return ("reward/" if float(scale) > 0 else "cost/") + key


@dataclass
class State:
    """mjx_env.State counterpart (reference joystick.py:321): tensors are views of the engine's output buffers,
    valid until the next reset/step call."""
    data: Any                       # the engine Batch (physics state lives on the device)
    obs: Dict[str, Any]             # {"state": [N,101], "privileged_state": [N,212]}
    reward: Any                     # [N]
    done: Any                       # [N]
    metrics: Dict[str, Any]         # reward/* cost/* swing_peak, each [N]
    info: Dict[str, Any] = field(default_factory=dict)   # {"truncation": [N]} + every other key of the reference's info, fetched on first use (_Info)


class _Info(dict):
    """`State.info` (reference joystick.py:278-302 + the wrappers' additions): "truncation" is the engine's output tensor; every
    other key of the reference's dict -- rng, step, command, last_act, last_last_act, last_last_last_act, motor_targets,
    feet_air_time, last_contact, swing_peak, push, push_step, push_interval_steps, action_history, imu_history, imitation_i, and
    steps / episode_done / episode_metrics/* -- lives in the engine's per-env record on the device and is copied out ON FIRST USE
    (one synchronous read of the records per State, `Batch.info()` -> `odk_record_field`): reading `info["command"]` works like
    in the reference, it is just not free.  Every way of reading a dict triggers that fetch: `[]`, `get`, `in`, iteration, `keys` /
    `values` / `items`, `len`, `dict(info)`, `copy`.  Values are tensors on the env's device, [N, ...]; `last_contact` is bool [N, 2].

    The reference's info is an immutable snapshot; the engine is stateful and keeps ONE set of records.  A State whose info has not
    been fetched yet when the env moves on (a later `reset` / `step` / `set_records`) can no longer produce its own step's values:
    reading it then raises `RuntimeError` instead of silently returning the newer step's (fetch what you need before stepping on).
    Writing goes through `Batch.info()` / `set_records` (the reference's functional update has no counterpart on a stateful engine)."""

    def __init__(self, batch, truncation):
        super().__init__(truncation=truncation)
        self._batch = batch
        self._generation = batch.generation
        self._fetched = False

    def _fetch(self):
        if self._fetched:
            return
        if self._batch.generation != self._generation:
            raise RuntimeError("State.info: the env has been stepped / reset since this State was made and its info was never read; "
                               "the engine holds only the current records (read info before the next step)")
        import torch
        I = self._batch.info()
        dev = dict.__getitem__(self, "truncation").device
        for k in self._batch.INFO_FIELDS:
            if k == "truncation":
                continue
            v = self._batch.last_contact_bool(I) if k == "last_contact" else I[k]
            dict.__setitem__(self, k, torch.from_numpy(np.ascontiguousarray(v)).to(dev))
        self._fetched = True

    def __missing__(self, key):
        if key in self._batch.INFO_FIELDS:
            self._fetch()
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._batch.INFO_FIELDS

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def __iter__(self):
        self._fetch()
        return dict.__iter__(self)

    def __len__(self):
        self._fetch()
        return dict.__len__(self)

    def keys(self):
        self._fetch()
        return dict.keys(self)

    def values(self):
        self._fetch()
        return dict.values(self)

    def items(self):
        self._fetch()
        return dict.items(self)

    def copy(self):
        self._fetch()
        return dict(dict.items(self))


class Joystick:
    """Track a joystick command (reference joystick.py:105)."""

    METRIC_NAMES = engine.METRIC_NAMES

    def __init__(self, task: str = "flat_terrain", config: Optional[ConfigDict] = None, config_overrides: Optional[Dict[str, Any]] = None,
                 num_envs: int = 8192, device: int = 0, autoreset: bool = True, lanes_per_env: int = 0, env_id_offset: int = 0,
                 xml_path: Optional[str] = None, model=None):
        """`xml_path` / `model` (additive): a robot of one's own instead of a shipped task -- the MJCF (compiled by mjcf.py) or a compiled `Model`.
        The reference's recipe for a new robot (README.md:74-85) copies base.py / constants.py / joystick.py and edits names; here the names the
        reference looks up (constants.py: sites `imu`, `left_foot`, `right_foot`; geoms `left_foot_bottom_tpu`, `right_foot_bottom_tpu`, `floor`;
        the 15 sensors; keyframe `home`) are what the XML must carry, and the index tables of base.py:63-125 / joystick.py:121-200 come out of the
        compiled model.

        Imitation reward (BUILD-DEFINED config keys; they travel in `config_overrides` and the evaluation sibling inherits them):
        `reference_motion` -- a `polynomial_coefficients.pkl` (reference_motion.ReferenceMotion.from_pickle) -- turns the imitation reward on
        for any robot, with that table; `imitation_joints` names the motion's frame joints in frame order and `imitation_ignore` the frame
        joints to leave out (reference_motion.imitation_joint_map: the defaults are the duck's frame and custom_rewards.py:80-88's joints for
        the duck, the actuated joints for another robot).  Without `reference_motion` the duck trains on the shipped table
        (assets/prm_table.npz) and another robot without the imitation reward."""
        self._config = _merge(config if config is not None else self._default_config(), config_overrides)
        if model is not None:
            self._model = model
        elif xml_path is not None:
            from .model import Model
            self._model = Model.from_xml(xml_path, sim_dt=float(self._config.sim_dt))
        else:
            self._model = constants.task_to_model(task)      # KeyError for unknown task names
        self._robot = constants.robot_of(self._model)
        self._motion = self._load_reference_motion()
        self._head_map = self._load_head_joints()
        cone = self._config.get("cone", None)
        if cone is not None:      # BUILD-DEFINED switch (the reference edits the XML's <option cone=...>): "pyramidal" | "elliptic", optional "impratio"
            if cone not in ("pyramidal", "elliptic"):
                raise ValueError(f"config cone = {cone!r}: 'pyramidal' or 'elliptic'")
            import numpy as _np
            from .model import Model
            edit = {"opt_cone": _np.array([1 if cone == "elliptic" else 0], _np.int32)}
            if self._config.get("impratio", None) is not None:
                edit["opt_impratio"] = _np.array([float(self._config.get("impratio"))], _np.float64)
            self._model = Model({**self._model.a, **edit}, xml_path=self._model.xml_path)
        # (lanes_per_env is a hint: a model with elliptic cones -- from this switch or from its own XML --, a height field or a robot that is not the
        # duck runs 32 lanes per env whatever is asked here; `batch.lanes_per_env` reports it)
        self._task = task
        self.num_envs = int(num_envs)
        self._env_id_offset = int(env_id_offset)
        self._batch = engine.Batch(self._model, self.num_envs, self._engine_config(autoreset, lanes_per_env), device=device,
                                   prm=self._motion.prm() if self._motion is not None else None)
        if self._motion is not None:
            self._batch.set_imitation_joints(self._imitation_map)
        if self._head_map is not None:
            self._batch.set_head_joints(self._head_map)
        self._batch.set_reward_terms(to_reward_terms(self._config, self._model.nu, self._reward_slots()))
        scales = self._config.reward_config.scales
        # State.metrics names of the Batch.xmetrics columns (None: the term is off)
        self.XMETRIC_NAMES = tuple(reward_metric_name(k, scales[k]) if k in self.reward_terms() else None for k in LIBRARY_TERMS)

    def _default_config(self) -> ConfigDict:
        return default_config()

    def _load_reference_motion(self):
        """The `reference_motion` config key's table and joint map, or None (keys: Joystick.__init__)."""
        path = self._config.get("reference_motion", None)
        if path is None:
            for k in ("imitation_joints", "imitation_ignore"):
                if self._config.get(k, None) is not None:
                    raise ValueError(f"config {k} is set without reference_motion (the joint map belongs to a reference motion)")
            return None
        from .reference_motion import ReferenceMotion, imitation_joint_map
        motion = ReferenceMotion.from_pickle(str(path))
        self._imitation_map = imitation_joint_map(self._model, motion, self._config.get("imitation_joints", None),
                                                  self._config.get("imitation_ignore", None))
        return motion

    def _load_head_joints(self):
        """The Standing task's `head_joints` map (Standing.__init__), or None: the Joystick task has no posture cost (ignore_head=False)."""
        if self._config.get("head_joints", None) is not None:
            raise ValueError("config head_joints: the Joystick task has no head-joint map (cost_stand_still(ignore_head=False)); it is the Standing task's")
        return None

    @property
    def head_joints(self):
        """The Standing task's head-joint map set on the batch (actuator per posture-command slot, -1: none), or None (the model's default)."""
        return self._head_map

    @property
    def reference_motion(self):
        """The ReferenceMotion loaded from the `reference_motion` config key, or None (the duck's shipped table / no imitation)."""
        return self._motion

    @property
    def imitation_joints(self):
        """The imitation joint map the batch compares with (frame joint per actuator, -1: not compared): the `reference_motion` key's, the
        duck's own (custom_rewards.py:80-88) on the shipped table, or None for a robot that runs without the imitation reward."""
        if self._motion is not None:
            return [int(j) for j in self._imitation_map]
        if not self._robot.is_open_duck:
            return None
        return [u if u < 5 else (u + 2 if u >= 9 else -1) for u in range(self._model.nu)]      # odk_batch_create's default

    def _engine_config(self, autoreset: bool, lanes_per_env: int) -> engine.EnvConfig:
        imitation = USE_IMITATION_REWARD and (self._robot.is_open_duck or self._motion is not None)
        return to_engine_config(self._config, autoreset, lanes_per_env, use_imitation=imitation,
                                joints_order_no_head=self._robot.joints_order_no_head, leg_actuators=self._robot.leg_actuators)

    def _reward_slots(self):
        return REWARD_SLOTS

    def reward_terms(self):
        """The reward-library terms this env computes (keys of reward_config.scales; include/odk.h odk_xterm), in column order."""
        return active_reward_terms(self._config, self._reward_slots())

    # ---- reference accessors (base.py:277-291, MjxEnv)
    @property
    def xml_path(self) -> str: return self._model.xml_path
    @property
    def action_size(self) -> int: return self._model.nu
    @property
    def mj_model(self): return self._model
    @property
    def mjx_model(self): return self._batch
    @property
    def observation_size(self): return {"state": (self._batch.nobs,), "privileged_state": (self._batch.npriv,)}
    @property
    def dt(self) -> float: return self._config.ctrl_dt
    @property
    def sim_dt(self) -> float: return self._config.sim_dt
    @property
    def n_substeps(self) -> int: return int(round(self._config.ctrl_dt / self._config.sim_dt))
    @property
    def unwrapped(self): return self
    @property
    def batch(self) -> "engine.Batch": return self._batch
    @property
    def env_id_offset(self) -> int: return self._env_id_offset      # env e is env env_id_offset + e of the run (a rank's first env)

    def make_eval_env(self, num_envs: int = 128):
        """Sibling env for the Evaluator (brax wraps `eval_env or environment` a second time with num_eval_envs)."""
        # a few hundred envs leave most SIMDs empty, so an evaluation of 1000 sequential steps is bound by ONE wave's latency:
        # 64 lanes per env (one env per wave) finish a step 7 % sooner than two envs sharing a wave (0.194 vs 0.209 ms at 128 envs)
        return type(self)(task=self._task, config=self._config, num_envs=num_envs, device=self._batch.device, autoreset=True,
                          lanes_per_env=64 if num_envs <= 1024 else 0, env_id_offset=1 << 24, model=self._model)

    def randomize(self, rng: np.random.Generator):
        """randomization_fn hook of brax ppo.train (reference runner.py:26, common/runner.py:108)."""
        from . import randomize
        fields, _ = randomize.domain_randomize(self._model, rng, self.num_envs)
        randomize.apply(self._batch, fields)
        return fields

    def _state(self) -> State:
        b = self._batch
        metrics = {name: b.metrics[:, i] for i, name in enumerate(self.METRIC_NAMES) if name is not None}
        if b.reward_terms_on:
            metrics.update({name: b.xmetrics[:, i] for i, name in enumerate(self.XMETRIC_NAMES) if name is not None})
        return State(data=b, obs={"state": b.obs, "privileged_state": b.priv}, reward=b.reward, done=b.done, metrics=metrics,
                     info=_Info(b, b.truncation))

    def reset(self, rng: int) -> State:
        """reference joystick.py:206: `rng` is an integer seed; env e draws from key(seed, env_id_offset + e)."""
        self._batch.reset(int(rng), self._env_id_offset)
        return self._state()

    def set_commands(self, cmd) -> None:
        """Drive the envs with caller-given commands instead of sampled ones (what mujoco_infer.py's keyboard `self.commands` does for
        one CPU env): `cmd` is a contiguous float32 [num_envs, 7] tensor on the env's device -- lin_vel_x, lin_vel_y, ang_vel_yaw,
        neck_pitch, head_pitch, head_yaw, head_roll per env -- or None to return to sampled commands.  Every step, reset and auto-reset
        uses env e's row as it is when that launch runs; the random streams stay those of an unbound run.  The env holds a reference to
        the tensor while it is bound; write into it to change the commands (`Batch.bind_commands`)."""
        self._batch.bind_commands(cmd)

    @property
    def commands(self):
        """The tensor bound by `set_commands`, or None."""
        return self._batch.commands

    def set_pushes(self, push) -> None:
        """Push the envs with caller-given kicks instead of the sampled training push (what grabbing the robot with the mouse does in
        mujoco_infer.py's viewer): `push` is a contiguous float32 [num_envs, >= 2] tensor on the env's device -- the world-frame
        velocity kick (dvx, dvy) in m/s that env e's next step adds to qvel[0:2] -- or None to return to `push_config`.  Every step
        applies env e's row as it is when that launch runs (zero it after the pushed step); `info["push"]` holds the kick's unit
        direction; the random streams stay those of an unbound run.  The env holds a reference to the tensor while it is bound
        (`Batch.bind_pushes`).  Standing inherits this."""
        self._batch.bind_pushes(push)

    @property
    def pushes(self):
        """The tensor bound by `set_pushes`, or None."""
        return self._batch.pushes

    def set_action_delays(self, delays) -> None:
        """Fix the envs' action delay instead of drawing it every step (joystick.py:357-376 draws 0..2 control steps): `delays` is an
        int32 tensor on the env's device with at least num_envs rows -- env e's delay in control steps, 0, 1 or 2; a negative value keeps
        the sampled delay for that env -- or None to return every env to the sampler.  Every step reads env e's row as it is when that
        launch runs; the random streams stay those of an unbound run.  The env holds a reference to the tensor while it is bound
        (`Batch.bind_action_delays`).  Standing inherits this."""
        self._batch.bind_action_delays(delays)

    @property
    def action_delays(self):
        """The tensor bound by `set_action_delays`, or None."""
        return self._batch.action_delays

    def step(self, state: State, action) -> State:
        """reference joystick.py:323 (+ Episode/AutoReset wrappers): one fused kernel launch."""
        self._batch.step(action)
        return self._state()
