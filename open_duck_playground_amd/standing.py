"""Standing task for Open Duck Mini V2 -- batched, device-resident mirror of reference
playground/open_duck_mini_v2/standing.py (`Standing`:103, `default_config`:44-100).

Same fused kernel as `Joystick` with `env_kind = ODK_ENV_STANDING`: no imitation reward / phase, no motor speed
limit (standing.py:42,377-380), observation without motor targets (85 floats, :524-540; privileged 153, :548-565),
rewards orientation / torques / action_rate / alive / stand_still(ignore_head) / head_pos (:585-606), no move
command (:652-654), base-velocity reset noise +-0.5 (:247).
"""
from __future__ import annotations

import numpy as np

from . import constants, engine
from .joystick import ConfigDict, Joystick, State, to_engine_config  # noqa: F401

USE_IMITATION_REWARD = False      # reference standing.py:42

# reward slot order of the engine for this env kind (include/odk.h: odk_env_config.reward_scales)
REWARD_SLOTS = ("orientation", "head_pos", "torques", "action_rate", "stand_still", "alive", None)
METRIC_NAMES = ("cost/orientation", "cost/head_pos", "cost/torques", "cost/action_rate", "cost/stand_still", "reward/alive", None, "swing_peak")


def default_config() -> ConfigDict:
    """reference standing.py:44-100, key for key."""
    C = ConfigDict
    return C(
        ctrl_dt=0.02, sim_dt=0.002, episode_length=1000, action_repeat=1, action_scale=0.25, dof_vel_scale=0.05, history_len=0,
        soft_joint_pos_limit_factor=0.95,
        noise_config=C(level=1.0, action_min_delay=0, action_max_delay=3, imu_min_delay=0, imu_max_delay=3,
                       scales=C(hip_pos=0.03, knee_pos=0.05, ankle_pos=0.08, joint_vel=2.5, gravity=0.1, linvel=0.1, gyro=0.05, accelerometer=0.005)),
        reward_config=C(scales=C(orientation=-0.5, torques=-1.0e-3, action_rate=-0.375, stand_still=-0.3, alive=20.0, head_pos=-2.0),
                        tracking_sigma=0.01),
        push_config=C(enable=True, interval_range=[5.0, 10.0], magnitude_range=[0.1, 1.0]),
        neck_pitch_range=[-0.34, 1.1], head_pitch_range=[-0.78, 0.78], head_yaw_range=[-2.7, 2.7], head_roll_range=[-0.5, 0.5],
        head_range_factor=1.0,
    )


def head_joint_map(model, head_joints):
    """The `head_joints` config key -> odk_batch_set_head_joints' map: for each slot of constants.HEAD_SLOTS (neck_pitch, head_pitch,
    head_yaw, head_roll) the actuator of the joint named for it, -1 for a slot without one ({} -> a robot without head joints).
    ValueError names an unknown slot, a name that is not a joint, a joint no actuator drives, a joint that more than one actuator drives (the
    map holds one actuator per slot: the others would stay in cost_stand_still), a joint used twice and a leg joint
    (constants.robot_of(model).joints_order_no_head: cost_stand_still(ignore_head=True) leaves only head joints out)."""
    if not isinstance(head_joints, dict):
        raise ValueError(f"config head_joints = {head_joints!r}: a dict from head slot ({', '.join(constants.HEAD_SLOTS)}) to joint name")
    a = model.a
    jn = [str(n) for n in a["names_jnt"]]
    trn = [int(j) for j in np.asarray(a["actuator_trnid"]).reshape(model.nu, -1)[:, 0]]
    legs = set(constants.robot_of(model).joints_order_no_head)
    out, used = [-1] * len(constants.HEAD_SLOTS), {}
    for slot, joint in head_joints.items():
        if slot not in constants.HEAD_SLOTS:
            raise ValueError(f"head_joints: unknown slot {slot!r} (slots: {', '.join(constants.HEAD_SLOTS)})")
        joint = str(joint)
        if joint not in jn:
            raise ValueError(f"head_joints {slot}={joint}: the robot has no joint {joint!r}")
        drivers = [u for u, j in enumerate(trn) if j == jn.index(joint)]
        if not drivers:
            raise ValueError(f"head_joints {slot}={joint}: no actuator drives joint {joint!r}")
        if len(drivers) > 1:
            raise ValueError(f"head_joints {slot}={joint}: joint {joint!r} is driven by {len(drivers)} actuators ({', '.join(map(str, drivers))}); "
                             "the map takes one actuator per slot")
        if joint in used:
            raise ValueError(f"head_joints {slot}={joint}: joint {joint!r} is used twice ({used[joint]} and {slot})")
        if joint in legs:
            raise ValueError(f"head_joints {slot}={joint}: {joint!r} is a leg joint (cost_stand_still(ignore_head=True) counts every leg joint)")
        used[joint] = slot
        out[constants.HEAD_SLOTS.index(slot)] = drivers[0]
    return out


def to_standing_engine_config(cfg: ConfigDict, autoreset: bool = True, lanes_per_env: int = 0, head_map=None, joints_order_no_head=None,
                              leg_actuators=None) -> engine.EnvConfig:
    """reference config -> odk_env_config for the Standing task; `head_map` (head_joint_map, or None: the model's default): a posture
    command that no joint tracks keeps its draw, from the range [0, 0].  `joints_order_no_head` / `leg_actuators`: as in `to_engine_config`
    (the qpos noise scales of a robot that is not the duck, by actuator)."""
    c = to_engine_config(cfg, autoreset, lanes_per_env, standing=True, reward_slots=REWARD_SLOTS,
                         use_imitation=USE_IMITATION_REWARD, use_motor_speed_limits=False, joints_order_no_head=joints_order_no_head,
                         leg_actuators=leg_actuators)
    for k, u in enumerate(head_map or ()):
        if u < 0:
            c.cmd_range[3 + k][0] = c.cmd_range[3 + k][1] = 0.0
    return c


def describe_head_joint_map(model, hmap) -> str:
    """One line: each slot with its joint and actuator, `-` for a slot without one."""
    act = [str(n) for n in model.a["names_actuator"]]
    jn = [str(n) for n in model.a["names_jnt"]]
    trn = [int(j) for j in np.asarray(model.a["actuator_trnid"]).reshape(model.nu, -1)[:, 0]]
    parts = [f"{slot}={jn[trn[u]]} (actuator {u} {act[u]})" if u >= 0 else f"{slot}=-" for slot, u in zip(constants.HEAD_SLOTS, hmap)]
    return "head joints: " + ", ".join(parts)


class Standing(Joystick):
    """Standing policy (reference standing.py:103).

    Head joints (BUILD-DEFINED config key `head_joints`, not in default_config(); it travels in `config_overrides` and the evaluation
    sibling inherits it): a dict from posture-command slot (neck_pitch, head_pitch, head_yaw, head_roll) to the joint that tracks it,
    e.g. {"neck_pitch": "neck_a", "head_yaw": "neck_b"}; {} for a robot without head joints.  cost_head_pos compares the mapped joints
    with their commands, cost_stand_still(ignore_head=True) leaves them out, and a slot without a joint samples the range [0, 0] (same
    draws).  Without the key the duck keeps its own head (actuators 5..8) and another robot is refused."""

    METRIC_NAMES = METRIC_NAMES

    def _default_config(self) -> ConfigDict:
        return default_config()

    def _reward_slots(self):
        return REWARD_SLOTS   # `orientation` is native here: the library's copy of it is the Joystick's

    def _load_reference_motion(self):
        for k in ("reference_motion", "imitation_joints", "imitation_ignore"):
            if self._config.get(k, None) is not None:
                raise ValueError(f"config {k}: the Standing task has no imitation reward (standing.py:42)")
        return None

    @property
    def imitation_joints(self):
        return None      # no imitation reward, no frame in the privileged row

    def _load_head_joints(self):
        spec = self._config.get("head_joints", None)
        return None if spec is None else head_joint_map(self._model, spec)

    def _engine_config(self, autoreset: bool, lanes_per_env: int) -> engine.EnvConfig:
        return to_standing_engine_config(self._config, autoreset, lanes_per_env, self._head_map,
                                         joints_order_no_head=self._robot.joints_order_no_head, leg_actuators=self._robot.leg_actuators)

    def describe_head_joints(self) -> str:
        """The head-joint map in use, one line."""
        if self._head_map is None:
            return "head joints: the duck's (actuators 5..8)" if self._robot.is_open_duck else "head joints: none set"
        return describe_head_joint_map(self._model, self._head_map)
