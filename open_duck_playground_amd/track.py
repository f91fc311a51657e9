"""Velocity tracking of a trained policy under given commands (what the reference answers with
playground/open_duck_mini_v2/mujoco_infer.py -- one CPU env, commands from the keyboard, observations saved to
mujoco_saved_obs.pkl for playground/common/plot_saved_obs.py -- batched on the GPU and measured).

    python -m open_duck_playground_amd.track --checkpoint checkpoints/<run>.pt --command 0 0 0 --command 0.15 0 0 --command 0 0 0.5
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --grid vx=-0.15:0.15:3,wz=-1:1:5 --envs_per_command 128 --output report.json

Every command gets a block of `--envs_per_command` envs, bound with `set_commands` (commands are not resampled), and the
deterministic policy (action = tanh(loc), as `Evaluator` and the ONNX export) drives them for `--episode_length` steps.  One
evaluation step -- the policy (the whole-network inference launch where the architecture allows), the fused env step and the
tracking accumulator (`odk_tracking_accumulate`) -- is captured once as a HIP graph and replayed; only the final sums come to the
host.  Each env counts over its first episode (Evaluator semantics).  The report is one JSON document: per command the mean achieved
local linear velocity x / y and yaw rate, the RMS error per axis against the command, the fall rate (episodes that ended with done and
no truncation), the mean episode reward and the step counts, plus the run's settings.

Pushes (what grabbing the robot with the mouse answers in that viewer: does the policy stay on its feet, and how long until it walks
straight again?):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --push_grid magnitude=0:1.5:6,direction=0:315:8 --push_at 200

`--push DVX DVY` (repeatable) and `--push_grid magnitude=a:b:n,direction=c:d:m` (degrees, world frame, 0 = +x) give world-frame velocity
kicks in m/s; every (command, push) cell gets `--envs_per_command` envs, command blocks outermost.  The kick is added once, to the step of
the first episode that `--push_at` names, through `set_pushes`: the push buffer is written inside the captured step from a device step
counter, so the run stays one graph replay per step.  `odk_push_accumulate` follows each env until its first episode ends; every command
row of the report gains "pushes" (per push: fall rate after the push, steps to the fall, recovery time -- the last step at which the
velocity error exceeded `--push_tolerance` -- and the error peaks) and "max_push_survived" (per direction).  Without push flags the
report, the graph and the JSON keys are exactly those above.

Gait and actuator load (how does it walk, and what does that cost the motors?):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --gait

`--gait` adds one launch (`odk_gait_accumulate`) to the captured step, before the tracking accumulator; it reads the noise-free privileged
observation the step wrote and touches nothing else.  Every command row (and, with pushes, every cell too) gains a "gait" object: duty
factor, double support and flight, step frequency, swing time and foot slip per foot, root height, trunk wobble, action rate, mechanical
power and cost of transport, and per actuator the torque RMS and peak against its force range, the saturation share, the speed peak, the
power and the joint range used (`reduce_gait`).  Without `--gait` nothing changes.

Posture and stillness (does the head go where the posture commands send it, and does the rest of the robot keep still? -- the Standing
task's whole purpose, and the four command entries the figures above never read):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --env standing --grid head_yaw=-1:1:5 --posture

`--posture` adds one launch (`odk_posture_accumulate`) to the captured step, before the tracking accumulator, with gait's contract.  Every
command row (and, with pushes, every cell too) gains a "posture" object: per mapped head slot the joint, the command, the mean angle, the
RMS and peak error against the command, the settle time (the last sample whose error exceeded `--posture_tolerance`: the episode starts at
the home pose, so the run is a step response) and the share of envs that ended inside the tolerance; the mean of cost_head_pos; and under
"stillness" the planar drift speed, yaw and roll/pitch rate RMS, lean, root height and the two parts of cost_stand_still over the joints
that are not the head's (`reduce_posture`).  The head-joint map is the env's: the duck's own, or `--env standing --head_joints` for another
robot.  Without `--posture` nothing changes.

Imitation fidelity (does the policy walk the reference gait? -- the question behind `imitation=` and a `polynomial_coefficients.pkl` of one's
own, which the reference answers with ref_motion_viewer.py and plot_saved_obs.py on one CPU robot, compared by eye):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --imitation_report

`--imitation_report` adds one launch (`odk_imitation_accumulate`) to the captured step, before the tracking accumulator, with gait's
contract.  It compares the step's noise-free privileged observation with the reference-motion frame the reward read in that step, through
the batch's imitation joint map.  Every command row (and, with pushes, every cell too) gains an "imitation" object: per compared joint the
bias, RMS and peak position error, the velocity RMS error and the range used against the reference's; the reward's joint_pos and joint_vel
terms; per foot the contact agreement, stance shares, touchdown counts and the touchdown lag against the reference's touchdown; the
reward's contact term; and the planar speed error (`reduce_imitation`).  The Joystick task with the imitation reward on: the duck, or
another robot with `--reference_motion`.  Without the flag nothing changes.

Command schedules and the step response (walk to stop, forward to turn: how fast does the policy follow a NEW command? -- what changing the
command with the keyboard shows in that viewer while the robot walks):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --sequence "0: 0 0 0 | 150: 0.15 0 0 | 400: 0 0 0.5 | 700: 0 0 0"
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --grid vx=-0.15:0.15:3,wz=-1:1:3 --then 0 0 0 --switch_at 300 --output transitions.json

`--sequence` (repeatable) is one schedule of up to 8 segments, `start_step: command` each, the first at step 0; `--then V...` (repeatable)
with `--switch_at N` crosses every `--command` / `--grid` row with every then-command into two-segment schedules, from-commands outermost:
the transition matrix of a grid.  Every schedule gets `--envs_per_command` envs and one row of the report.  Two launches join the captured
step: `odk_command_schedule_apply` before the env step writes each env's row of the bound command tensor from the schedule table -- its
clock is the tracking accumulator's step count, so there is no other counter -- and `odk_response_accumulate`, before the tracking
accumulator, follows each segment.  A schedule row keeps every key above: `command` is segment 0's, and the velocity statistics are against
the command in force at each step (the tracking accumulator reads the row the step read).  It gains "schedule" (the segments as given)
and "segments": per segment the samples, mean velocities and RMS errors, the fall rate among the envs that entered it, the response time
(the first sample within `--response_tolerance` of the new command), the settle time (the last sample outside it) and the settled share,
the error peaks after the response, the overshoot per axis past the command in the direction of the change, and the steady-state error over
the samples later than `--response_tail_after` steps into the segment (`reduce_response`).  `--gait` and `--imitation_report` combine with
schedules, one object per schedule row; pushes and `--posture` do not (their figures assume one command per episode), and the response
figures cover vx, vy and wz although all seven entries of a segment are applied.  Without `--sequence` / `--then` nothing changes.

Falls (why, when and which way does it go down? -- what watching one robot tip over in that viewer shows, for every env that falls):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.15 0 0 --push_grid magnitude=0:1.5:6,direction=0:315:8 --falls --save_falls falls.npz

`--falls` adds one launch (`odk_fall_accumulate`) to the captured step, before the tracking accumulator.  It is a recorder, not a sum: per
env a ring of the last `--fall_ring` samples of its first episode -- the up vector, gyro, local velocity, root height, contacts, command
errors, the number of saturated actuators and the whole `qpos`, read on the device from the batch's own state -- that freezes when the
episode ends, plus the last sample at which the lean was within `--fall_tilt` and the contacts then.  Nothing comes to the host before the
end of the run.  Every command row (with pushes every cell, with schedules every schedule row) gains a "falls" object: the fall rate and
the fall step's quartiles, the direction of the fall in the base body's frame (forward / backward / left / right shares) and in the
world, the onset (how long before the termination the robot left the upright, and on which foot it stood then), the share of falls with
a saturated actuator in the ring, how close the survivors came, and the mean profile of lean, height, roll/pitch rate, command error and
saturation over the samples before the termination (`reduce_falls`).  `--save_falls PATH` writes the rings of the first
`--save_falls_max` falls of every row (cell) as an .npz of clips that replay like `--save_qpos` (`fall_clips`).  `--falls` combines with
every flag above.  Without it nothing changes.

Plants (how much control latency and model error does it tolerate? -- the reference randomises kp, body masses, friction loss, armature
and a 0..2-step action delay in training, so a trained policy claims robustness to them; here they are controlled axes):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --plant_grid kp=0.7:1.3:4,mass=0.9:1.2:3,delay=0:2:3
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --grid vx=-0.15:0.15:3 --plant kp=0.6,delay=2 --plant kp=1.0 --falls

`--plant KEY=V[,KEY=V...]` (repeatable) and `--plant_grid` (a cross product, `--grid`'s syntax) name plants: `kp`, `mass`, `frictionloss`
and `armature` are scales on the model's values (every actuator's gain, with the bias following; every body's mass, inertias NOT rescaled,
as playground/common/randomize.py; the actuated dofs' friction loss and armature), `delay` is the action delay in control steps, 0, 1, 2 or
`random` (the sampler, the default).  Every (command, plant) cell gets `--envs_per_command` envs, command blocks outermost (`plant_blocks`,
the layout pushes use).  The host hands the engine nominal value times scale per env (`odk_batch_set_param`) and binds an int32 delay per env
(`set_action_delays`, -1 for `random`); the captured step is the plain one.  Every command row gains "plants" -- per cell a whole command
row of its own plus "plant" -- and "robustness": per swept axis, with the other axes at their value nearest nominal, the fall rate,
RMS errors and episode reward against the axis, and "survived_range", the contiguous run of values around nominal whose fall rate stays
within `--robust_fall_rate`.  `--gait`, `--falls`, `--imitation_report`, `--posture`, `--sequence` and `--then` combine with plants (one
object per cell too); `--push` / `--push_grid` do not (a third cell axis).  `--randomize` applies the training-time `domain_randomize` draw
to every env (seeded by `--seed`; a plant's scales multiply it), `--noise_level X` overrides `noise_config.level`.  Without these flags
nothing changes.

Paths and waypoints (where did it end up, and can something steer it? -- every figure above is a velocity, a rate or a joint quantity):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.15 0 0 --path
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --waypoints "0.5,0 | 0.5,0.5 | 0,0.5 | 0,0" --waypoints "1,0" --falls

`--path` adds one launch (`odk_path_accumulate`) to the captured step, before the tracking accumulator, and one (`odk_path_begin`) after the
reset.  They read the base pose from the batch's own state on the device and express it in each env's start frame, the pose right after
the reset (which draws every env's own offset and yaw).  Every row (cell, schedule row) gains a "path" object: forward and lateral
displacement, heading change, path length and straightness as mean and std over the envs, and for a row with one constant command the
dead-reckoned `ideal` pose and the mean distance to it (`reduce_path`).  `--waypoints` (repeatable: one course of 1 to 8 points in
start-frame metres each) makes every course a row of the report: `odk_waypoint_command_apply`, before the env step, steers each env towards
its next waypoint by writing vx and wz of the bound command tensor -- the clock is the tracking accumulator's, the waypoint index the path
accumulator's -- and the row gains "course": the share of envs that reached each waypoint and when, the cross-track error, the distance left
to the goal, the path length against the course's and the falls by leg (`reduce_course`).  `--waypoint_radius`, `--waypoint_speed`,
`--waypoint_turn_rate`, `--waypoint_gain` and `--waypoint_slow_dist` are the follower's settings.  `--waypoints` implies `--path`; it combines
with plants, `--gait`, `--falls` and `--imitation_report`, and not with `--command` / `--grid` (the course is the command), `--sequence` /
`--then` (two writers of the command tensor), pushes or `--posture`.  Without these flags nothing changes.

Sensor faults (what does it tolerate on the sensor side? -- a biased, tilted or late IMU, encoders with a zero error or a coarse step, a
foot switch that sticks: everyday faults of this robot that training never showed the policy, see INTEGRATION.md "Sensor faults"):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --sensor_grid imu_delay=0:7:8,gyro_bias_y=-0.3:0.3:5 --falls
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --grid vx=-0.15:0.15:3 --sensor acc_bias_x=1.3 --sensor contact_left=off --sensor encoder_offset=0.05

`--sensor KEY=V[,KEY=V...]` (repeatable) and `--sensor_grid` (a cross product, `--grid`'s syntax) name sensor settings (`sensors.SENSOR_KEYS`);
every (command, sensor) cell gets `--envs_per_command` envs, command blocks outermost (`sensors.sensor_blocks`, the plants' layout).  One
launch joins the captured step, in front of the policy: `odk_sensor_apply` reads the observation the env step wrote -- which stays what the
policy trained on, the env's own noise included -- and writes what each env's faulty sensors would deliver into a tensor of the Tracker's,
which the policy reads instead.  The env, physics and report kernels are untouched, and every report reads the noise-free privileged
row, so each keeps its meaning: a fault changes what the policy sees, the reports measure what the robot then does.  Every command row
gains "sensors" -- per cell a whole command row of its own plus "sensor", its settings -- and "sensor_robustness": `reduce_robustness` per
swept key with the other keys nearest their nominal, `survived_range` around the key's own nominal (0, 1 for the scales, `ok` for the foot
switches).  `--gait`, `--falls`, `--path`, `--posture`, `--imitation_report`, `--sequence` / `--then`, `--waypoints`, `--randomize` and
`--noise_level` combine with it (one object per cell too); pushes and plants do not (a third cell axis).  `--save_obs` then saves the row
the policy read.  Without these flags nothing changes.

Actuation faults (what does it tolerate between the policy and the servos? -- the runtime's low-pass filter, a lost command packet, the
servo's position step, a mis-indexed horn, a servo that drops off the bus, see INTEGRATION.md "Actuation faults"):

    python -m open_duck_playground_amd.track --checkpoint <ckpt> --command 0.1 0 0 --actuation_grid cutoff=5:40:8,drop=0:0.2:3 --falls
    python -m open_duck_playground_amd.track --checkpoint <ckpt> --grid vx=-0.15:0.15:3 --actuation quant=0.0015 --actuation freeze=left_knee,freeze_at=100

`--actuation KEY=V[,KEY=V...]` (repeatable) and `--actuation_grid` name actuation settings (`actuation.ACTUATION_KEYS`); every (command,
actuation) cell gets `--envs_per_command` envs, command blocks outermost (`actuation.actuation_blocks`).  One launch joins the captured
step, between the policy and the env step: `odk_action_apply` reads the policy's action and writes what each env's link delivers into a
tensor of the Tracker's, which the step takes; the env's action memories and `motor_targets` are therefore the delivered action's
(BUILD-DEFINED, the reference's deployment order).  Every command row gains "actuations" -- per cell a whole command row of its own plus
"actuation", its settings, and "link" (`dropped_share`) -- and "actuation_robustness".  Every report flag, `--sequence` / `--then`,
`--waypoints`, `--randomize` and `--noise_level` combine with it; pushes, plants and sensor faults do not (a third cell axis).  Without
these flags nothing changes.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import pickle
import sys
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .engine import (TRACK_NACC as NACC, TRACK_ENDED as ENDED, TRACK_STEPS as STEPS, TRACK_SAMPLES as SAMPLES, TRACK_FALLS as FALLS,
                     TRACK_REWARD as REWARD, TRACK_SUM as SUM, TRACK_SQERR as SQERR)      # ODK_TRACK_*

from .engine import (PUSH_NACC, PUSH_PUSHED as P_PUSHED, PUSH_PUSH_AT as P_PUSH_AT, PUSH_FELL as P_FELL, PUSH_STEPS_TO_FALL as P_STEPS_TO_FALL,
                     PUSH_LAST_OFF as P_LAST_OFF, PUSH_PEAK_LIN_ERR as P_PEAK_LIN, PUSH_PEAK_ANG_ERR as P_PEAK_ANG, PUSH_PRE_LIN_ERR_SUM as P_PRE_SUM,
                     PUSH_PRE_SAMPLES as P_PRE_SAMPLES, PUSH_PRE_LIN_ERR_LOW as P_PRE_LOW)      # include/odk.h ODK_PUSH_*: one definition, engine.py's

from .engine import (GAIT_NACC, GAIT_SAMPLES as G_SAMPLES, GAIT_SPEED_SUM as G_SPEED, GAIT_ABS_POWER_SUM as G_POWER, GAIT_CONTACT as G_CONTACT,
                     GAIT_DOUBLE as G_DOUBLE, GAIT_FLIGHT as G_FLIGHT, GAIT_TOUCHDOWNS as G_TOUCH, GAIT_SWING_STEPS_SUM as G_SWING, GAIT_SLIP_SUM as G_SLIP,
                     GAIT_HEIGHT_SUM as G_HEIGHT, GAIT_HEIGHT_SQ_SUM as G_HEIGHT_SQ, GAIT_ROLLPITCH_RATE_SQ_SUM as G_WOBBLE,
                     GAIT_ACTION_RATE_SUM as G_ARATE, GAIT_TORQUE_SQ as G_TORQUE_SQ, GAIT_TORQUE_PEAK as G_TORQUE_PEAK, GAIT_VEL_PEAK as G_VEL_PEAK,
                     GAIT_SAT as G_SAT, GAIT_ABS_POWER as G_ABS_POWER, GAIT_RANGE_MIN as G_RANGE_MIN, GAIT_RANGE_MAX as G_RANGE_MAX)      # ODK_GAIT_*

from .engine import (POSTURE_NACC, POSTURE_SAMPLES as S_SAMPLES, POSTURE_DRIFT_SPEED_SUM as S_DRIFT, POSTURE_YAW_RATE_SQ_SUM as S_YAW,
                     POSTURE_ROLLPITCH_RATE_SQ_SUM as S_WOBBLE, POSTURE_TILT_SUM as S_TILT, POSTURE_TILT_PEAK as S_TILT_PEAK, POSTURE_HEIGHT_SUM as S_HEIGHT,
                     POSTURE_LEG_POSE_SUM as S_LEG_POSE, POSTURE_LEG_VEL_SUM as S_LEG_VEL, POSTURE_HEAD_SQERR_SUM as S_HEAD_SQERR,
                     POSTURE_ANGLE_SUM as S_ANGLE, POSTURE_ERR_SQ_SUM as S_ERR_SQ, POSTURE_ERR_PEAK as S_ERR_PEAK,
                     POSTURE_LAST_OFF as S_LAST_OFF)      # ODK_POSTURE_*

from .engine import (IMIT_NACC, IMIT_SAMPLES as I_SAMPLES, IMIT_GATED as I_GATED, IMIT_SPEED_ERR_SQ_SUM as I_SPEED_ERR_SQ, IMIT_REF_SPEED_SUM as I_REF_SPEED,
                     IMIT_JOINT_POS_SQ_SUM as I_JOINT_POS_SQ, IMIT_JOINT_VEL_SQ_SUM as I_JOINT_VEL_SQ, IMIT_BOTH as I_BOTH, IMIT_ROBOT_ONLY as I_ROBOT_ONLY,
                     IMIT_REF_ONLY as I_REF_ONLY, IMIT_REF_TOUCHDOWNS as I_REF_TOUCH, IMIT_TOUCHDOWNS as I_TOUCH, IMIT_LAG_SUM as I_LAG,
                     IMIT_LAG_ABS_SUM as I_LAG_ABS, IMIT_POS_ERR_SUM as I_POS_ERR, IMIT_POS_ERR_SQ as I_POS_ERR_SQ, IMIT_POS_ERR_PEAK as I_POS_ERR_PEAK,
                     IMIT_VEL_ERR_SQ as I_VEL_ERR_SQ, IMIT_RANGE_MIN as I_RANGE_MIN, IMIT_RANGE_MAX as I_RANGE_MAX, IMIT_REF_RANGE_MIN as I_REF_RANGE_MIN,
                     IMIT_REF_RANGE_MAX as I_REF_RANGE_MAX)      # ODK_IMIT_*

from .engine import (SCHED_MAX_SEGMENTS, SCHED_SEG_FLOATS, SCHED_NEVER, RESP_NACC, RESP_STRIDE, RESP_ENTERED as R_ENTERED, RESP_SAMPLES as R_SAMPLES,
                     RESP_FELL as R_FELL, RESP_STEPS_TO_FALL as R_STEPS_TO_FALL, RESP_FIRST_IN as R_FIRST_IN, RESP_LAST_OFF as R_LAST_OFF,
                     RESP_PEAK_LIN_ERR as R_PEAK_LIN, RESP_PEAK_ANG_ERR as R_PEAK_ANG, RESP_SUM as R_SUM, RESP_SQERR as R_SQERR,
                     RESP_OVERSHOOT as R_OVERSHOOT, RESP_TAIL_SAMPLES as R_TAIL_SAMPLES, RESP_TAIL_SUM as R_TAIL_SUM)      # ODK_SCHED_* / ODK_RESP_*

from .engine import (FALL_HEAD, FALL_SAMPLE, FALL_MAX_RING, FALL_SAMPLES as F_SAMPLES, FALL_FELL as F_FELL, FALL_STEP as F_STEP,
                     FALL_LAST_UPRIGHT as F_LAST_UPRIGHT, FALL_UPRIGHT_CONTACT as F_UPRIGHT_CONTACT, FALL_TILT_PEAK as F_TILT_PEAK,
                     FALL_S_STEP as FS_STEP, FALL_S_UP as FS_UP, FALL_S_GYRO as FS_GYRO, FALL_S_HEIGHT as FS_HEIGHT, FALL_S_LIN_ERR as FS_LIN_ERR,
                     FALL_S_SAT as FS_SAT)      # ODK_FALL_*

from .engine import (PATH_NACC, PATH_MAX_WAYPOINTS, PATH_COURSE_FLOATS, PATH_START_X as W_START_X, PATH_START_Y as W_START_Y,
                     PATH_START_HX as W_START_HX, PATH_START_HY as W_START_HY, PATH_X as W_X, PATH_Y as W_Y, PATH_LENGTH as W_LENGTH,
                     PATH_TURN as W_TURN, PATH_SAMPLES as W_SAMPLES, PATH_FELL as W_FELL, PATH_FELL_LEG as W_FELL_LEG, PATH_WP_INDEX as W_WP_INDEX,
                     PATH_XTRACK_SAMPLES as W_XTRACK_SAMPLES, PATH_XTRACK_SQ as W_XTRACK_SQ, PATH_XTRACK_PEAK as W_XTRACK_PEAK,
                     PATH_GOAL_DIST as W_GOAL_DIST, PATH_REACHED as W_REACHED)      # ODK_PATH_*

from .engine import SENSOR_NPRM, SENSOR_NSTATE      # ODK_SENSOR_*
from .sensors import nominal_sensor, sensor_order, sensors_from_args, sensor_blocks      # --sensor / --sensor_grid: the settings and their per-env fault rows
from .engine import ACT_NPRM, ACT_NSTATE      # ODK_ACT_*
from .actuation import nominal_actuation, actuation_order, actuations_from_args, actuation_blocks, reduce_link      # --actuation / --actuation_grid
from .sweeps import parse_axis_grid, grid_rows, parse_key_values, cell_rows      # the syntaxes and the env layout every sweep flag shares

COMMAND_KEYS = ("vx", "vy", "wz", "neck_pitch", "head_pitch", "head_yaw", "head_roll")   # the order of cmd_range (include/odk.h)


def command_row(values: Sequence[float]) -> List[float]:
    """`--command vx vy wz [neck_pitch head_pitch head_yaw head_roll]` -> the 7 floats of a command row (head entries default to 0)."""
    v = [float(x) for x in values]
    if len(v) not in (3, 4, 5, 6, 7):
        raise ValueError(f"a command is vx vy wz [neck_pitch head_pitch head_yaw head_roll]: 3 to 7 numbers, got {len(v)}")
    return v + [0.0] * (7 - len(v))


def parse_grid(spec: str) -> List[List[float]]:
    """`vx=a:b:n,wz=c:d:m` -> the command rows of the grid: each named axis takes n values from a to b (numpy.linspace, ends included),
    axes not named stay 0, rows in itertools.product order of the axes as written (the last axis varies fastest)."""
    axes = parse_axis_grid("--grid", spec, COMMAND_KEYS)
    return [[float(row[k]) for k in COMMAND_KEYS] for row in grid_rows(axes, dict.fromkeys(COMMAND_KEYS, 0.0))]


def command_blocks(commands: Sequence[Sequence[float]], envs_per_command: int) -> np.ndarray:
    """[len(commands) * envs_per_command, 7] float32: command c drives envs c * envs_per_command .. (c + 1) * envs_per_command - 1."""
    return np.repeat(np.asarray(commands, np.float32).reshape(-1, 7), int(envs_per_command), axis=0)


PUSH_AXES = ("magnitude", "direction")
# BUILD-DEFINED defaults (the reference has no such measure): a velocity sample is "off" while its planar velocity error exceeds 0.05 m/s
# (a third of the duck's top commanded speed) or its yaw-rate error 0.2 rad/s (a fifth of the top commanded yaw rate)
DEFAULT_PUSH_TOLERANCE = (0.05, 0.2)
DEFAULT_PUSH_AT = 200


def push_entry(magnitude: float, direction_deg: float) -> Dict:
    """One push of the sweep: the world-frame kick of `magnitude` m/s towards `direction_deg` (0 = +x, 90 = +y)."""
    th = np.deg2rad(float(direction_deg))
    return dict(push=[float(magnitude * np.cos(th)), float(magnitude * np.sin(th))], magnitude=float(magnitude), direction_deg=float(direction_deg))


def push_row(values: Sequence[float]) -> Dict:
    """`--push DVX DVY` -> the push with that kick; its magnitude and direction (degrees in [0, 360), 0 for a zero kick) are derived."""
    v = [float(x) for x in values]
    if len(v) != 2:
        raise ValueError(f"a push is DVX DVY: 2 numbers, got {len(v)}")
    mag = float(np.hypot(v[0], v[1]))
    return dict(push=v, magnitude=mag, direction_deg=float(np.rad2deg(np.arctan2(v[1], v[0])) % 360.0) if mag > 0 else 0.0)


def parse_push_grid(spec: str) -> List[Dict]:
    """`magnitude=a:b:n,direction=c:d:m` -> the pushes of the grid, with `--grid`'s conventions: each axis takes n values from a to b
    (numpy.linspace, ends included), rows in itertools.product order of the axes as written (the last axis varies fastest).  Magnitude in
    m/s (required), direction in degrees (0 when not named)."""
    def check(name, part, lo, hi):
        if name == "magnitude" and min(lo, hi) < 0:
            raise ValueError(f"--push_grid: {part!r}: a magnitude is >= 0 (turn the direction instead)")
    axes = parse_axis_grid("--push_grid", spec, PUSH_AXES, check=check, required="magnitude")
    return [push_entry(cell["magnitude"], cell["direction"]) for cell in grid_rows(axes, {"magnitude": 0.0, "direction": 0.0})]


def cell_blocks(commands: Sequence[Sequence[float]], pushes: Sequence[Dict], envs_per_cell: int):
    """(cmd [n, 7], kicks [n, 2]) float32 with n = len(commands) * len(pushes) * envs_per_cell: cell (c, p) drives envs
    (c * len(pushes) + p) * envs_per_cell onwards (`sweeps.cell_rows`) -- command blocks outermost, so command c's envs stay one block of
    len(pushes) * envs_per_cell (what `reduce_tracking` pools)."""
    cmd = command_blocks(commands, len(pushes) * int(envs_per_cell))
    return cmd, cell_rows(np.asarray([p["push"] for p in pushes], np.float32).reshape(-1, 2), len(commands), envs_per_cell)


PLANT_SCALE_AXES = ("kp", "mass", "frictionloss", "armature")      # scales on the model's values (randomize.SCALED_FIELDS)
PLANT_AXES = PLANT_SCALE_AXES + ("delay",)
DELAY_RANDOM = "random"      # the sampled action delay: a device row of -1 (include/odk.h odk_batch_bind_action_delays)
DELAY_VALUES = (0, 1, 2)
DEFAULT_ROBUST_FALL_RATE = 0.05      # a REPORTING threshold the user sets (--robust_fall_rate), not a measured constant


def nominal_plant() -> Dict:
    """The plant the XML describes: every scale 1, the delay sampled."""
    return {"kp": 1.0, "mass": 1.0, "frictionloss": 1.0, "armature": 1.0, "delay": DELAY_RANDOM}


def _plant_value(flag: str, name: str, value) -> object:
    """One axis value as a plant holds it: a finite scale > 0, or for `delay` 0, 1, 2 or "random"; ValueError otherwise."""
    if name not in PLANT_AXES:
        raise ValueError(f"{flag}: unknown axis {name!r} (one of {', '.join(PLANT_AXES)})")
    if name == "delay":
        if isinstance(value, str) and value.strip().lower() == DELAY_RANDOM:
            return DELAY_RANDOM
        try:
            v = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{flag}: delay={value!r} is not 0, 1, 2 or {DELAY_RANDOM}")
        if not np.isfinite(v) or v != round(v):
            raise ValueError(f"{flag}: delay={value} is not a whole number of control steps (0, 1, 2 or {DELAY_RANDOM})")
        if int(v) not in DELAY_VALUES:
            raise ValueError(f"{flag}: delay={int(v)} is outside the action-history ring: 0, 1, 2 or {DELAY_RANDOM}")
        return int(v)
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{flag}: {name}={value!r} is not a number")
    if not np.isfinite(v) or v <= 0:
        raise ValueError(f"{flag}: {name}={value} is not a finite scale > 0 (1 = the model's own value)")
    return v


def parse_plant(spec: str) -> Dict:
    """`--plant kp=0.6,delay=2` -> a plant: `nominal_plant()` with the named axes replaced.  ValueError for an unknown axis, an axis given
    twice, a scale that is not a finite number > 0, and a delay that is not 0, 1, 2 or `random`."""
    return parse_key_values("--plant", spec, nominal_plant(), "axis", _plant_value)


def parse_plant_grid(spec: str) -> List[Dict]:
    """`kp=0.7:1.3:4,mass=0.9:1.2:3,delay=0:2:3` -> the plants of the grid, with `--grid`'s conventions: each axis takes n values from a to
    b (numpy.linspace, ends included), plants in itertools.product order of the axes as written (the last axis varies fastest), axes not
    named stay nominal.  A `delay` axis must come out as whole numbers within 0..2."""
    return grid_rows(parse_axis_grid("--plant_grid", spec, PLANT_AXES, value=_plant_value), nominal_plant())


def plants_from_args(args) -> List[Dict]:
    """The plants the command line asks for (`--plant` in order, then `--plant_grid`'s), [] without a plant flag.  SystemExit with the reason
    for a plant that cannot be parsed, for plants next to `--push` / `--push_grid` (a third cell axis) and for a `--robust_fall_rate`
    outside 0..1 -- host work only, before any batch exists."""
    specs, grid = getattr(args, "plant", None) or [], getattr(args, "plant_grid", None)
    try:
        plants = [parse_plant(s) for s in specs] + (parse_plant_grid(grid) if grid else [])
    except ValueError as err:
        raise SystemExit(str(err))
    if plants and (getattr(args, "push", None) or getattr(args, "push_grid", None)):
        raise SystemExit("--plant / --plant_grid do not combine with --push / --push_grid: (command, push, plant) would be a third cell axis; "
                         "run the push sweep once per plant")
    rate = float(getattr(args, "robust_fall_rate", DEFAULT_ROBUST_FALL_RATE))
    if not (np.isfinite(rate) and 0.0 <= rate <= 1.0):
        raise SystemExit(f"--robust_fall_rate is a fall rate: 0 .. 1, got {rate}")
    return plants


def plant_blocks(commands: Sequence[Sequence[float]], plants: Sequence[Dict], envs_per_cell: int):
    """(cmd [n, 7] float32, scales {axis: [n] float64}, delays [n] int32) with n = len(commands) * len(plants) * envs_per_cell: cell (c, p)
    drives envs (c * len(plants) + p) * envs_per_cell onwards -- `cell_blocks`' layout with plants where the pushes are.  `scales[axis][e]`
    is env e's scale of that axis, `delays[e]` its bound delay row: 0, 1, 2, or -1 for `random`."""
    cmd = command_blocks(commands, len(plants) * int(envs_per_cell))
    tile = lambda per_plant, dtype: cell_rows(np.asarray(per_plant, dtype), len(commands), envs_per_cell)
    scales = {axis: tile([float(p[axis]) for p in plants], np.float64) for axis in PLANT_SCALE_AXES}
    delays = tile([-1 if p["delay"] == DELAY_RANDOM else int(p["delay"]) for p in plants], np.int32)
    return cmd, scales, delays


def plant_fields(model, scales: Dict[str, np.ndarray], fields: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """What `randomize.apply` hands the engine for the envs of `plant_blocks`: the model's nominal values (`randomize.nominal_fields`; or
    `fields`, a `domain_randomize` draw) times env e's scales.  Parameters no axis names stay nominal."""
    from . import randomize
    n = len(next(iter(scales.values())))
    return randomize.scale_fields(fields if fields is not None else randomize.nominal_fields(model, n), scales)


def plant_order(axis: str, value) -> Optional[float]:
    """Where a plant's `value` sits on its axis' line: the number itself, and None for `random`, which is no point among the fixed delays."""
    return None if value == DELAY_RANDOM else float(value)


def survived_range(values: Sequence[float], fall_rates: Sequence[float], threshold: float, nominal: float = 1.0) -> Optional[List[float]]:
    """[lo, hi]: the contiguous run of `values` around the one nearest `nominal` whose fall rate is at most `threshold`, or None when that
    value itself fails (then nothing around nominal was survived).  The values are taken in increasing order; the run starts at the value
    nearest `nominal` (the smaller of two equally near -- nominal need not be in the grid) and grows in both directions until the first
    value whose fall rate exceeds the threshold: a failing value in the middle ends the run there, whatever passes beyond it."""
    order = sorted(range(len(values)), key=lambda i: float(values[i]))
    v = [float(values[i]) for i in order]
    ok = [float(fall_rates[i]) <= float(threshold) for i in order]
    if not v:
        return None
    k = min(range(len(v)), key=lambda i: (abs(v[i] - float(nominal)), v[i]))
    if not ok[k]:
        return None
    lo = hi = k
    while lo > 0 and ok[lo - 1]:
        lo -= 1
    while hi + 1 < len(v) and ok[hi + 1]:
        hi += 1
    return [v[lo], v[hi]]


ROBUSTNESS_POINT_KEYS = ("value", "fall_rate", "rms_error_vx", "rms_error_vy", "rms_error_wz", "mean_episode_reward")


def reduce_robustness(cells: Sequence[Dict], threshold: float, key: str = "plant", nominals: Optional[Dict] = None,
                      order: Optional[Callable] = None) -> Dict:
    """The "robustness" object of one command row from its plant cells (each a command row with "plant").  An axis is swept when the cells
    hold more than one value of it.  Per swept axis, under its name: the cells whose OTHER axes sit at their value nearest nominal (scale
    1; delay `random` if present, else the smallest), in increasing order of the axis (`random` first) -- `value`, `fall_rate`, the three
    RMS errors and `mean_episode_reward` each.  `survived_range`: per swept axis `survived_range()` of those points at `threshold`; for
    `delay` over the fixed delays, starting from the smallest (`random` is not a point on that line).  `robust_fall_rate` is the threshold.
    For cells of another kind (the sensor cells: `key` "sensor"): `nominals`, every axis with its own nominal value, and `order(axis,
    value)`, a value's place on its axis' line as a number (default: the value itself).  Nearest nominal and `survived_range` are then taken
    around the axis's own nominal, and a range's ends are the values of its end points (a name for an axis whose values are names).
    The plants are that with `nominal_plant()` and `plant_order`, whose None says that `random` is on no line: such a value sorts first,
    is nearest only to itself, and as a nominal leaves `survived_range` to start from the smallest point; their ranges' ends are numbers."""
    plants = nominals is None
    nominals = nominal_plant() if plants else nominals
    order = order or (plant_order if plants else (lambda axis, v: float(v)))
    axes = tuple(nominals)
    distinct = {a: [] for a in axes}
    for cell in cells:
        for a in axes:
            if cell[key][a] not in distinct[a]:
                distinct[a].append(cell[key][a])
    swept = [a for a in axes if len(distinct[a]) > 1]

    def far(a, v):      # (how far from the axis' nominal, the place): what is off the line is in front of it, and near only to itself
        o, n = order(a, v), order(a, nominals[a])
        return v != nominals[a], np.inf if None in (o, n) else abs(o - n), -np.inf if o is None else o
    base = {a: min(distinct[a], key=lambda v, a=a: far(a, v)) for a in axes}
    out: Dict = {"robust_fall_rate": float(threshold)}
    ranges: Dict = {}
    for axis in swept:
        line = [c for c in cells if all(c[key][o] == base[o] for o in axes if o != axis)]
        line.sort(key=lambda c: far(axis, c[key][axis])[2])
        out[axis] = [dict(value=c[key][axis], **{k: c[k] for k in ROBUSTNESS_POINT_KEYS[1:]}) for c in line]
        pts = [p for p in out[axis] if order(axis, p["value"]) is not None]
        at, nominal = [order(axis, p["value"]) for p in pts], order(axis, nominals[axis])
        ends = survived_range(at, [p["fall_rate"] for p in pts], threshold, min(at, default=0.0) if nominal is None else nominal)
        ranges[axis] = ends if ends is None or plants else [pts[at.index(x)]["value"] for x in ends]
    out["survived_range"] = ranges
    return out


PLANT_ROW_KEYS = ("plants", "robustness")


def _mean_or_none(x: np.ndarray) -> Optional[float]:
    return float(x.mean()) if x.size else None


DEFAULT_SWITCH_AT = 300
DEFAULT_RESPONSE_TAIL_AFTER = 100      # BUILD-DEFINED default: two seconds into a segment the transient counts as over


def parse_sequence(text: str) -> List[Dict]:
    """`--sequence "0: 0 0 0 | 150: 0.15 0 0 | 400: 0 0 0.5"` -> one schedule: a list of segments {start_step, command}, segments apart
    by `|`, each `start_step: vx vy wz [neck_pitch head_pitch head_yaw head_roll]` with the command padded as `command_row` does.  Syntax
    only (ValueError); what a schedule must satisfy is `check_schedule`'s."""
    segs = []
    for part in str(text).split("|"):
        start, colon, values = part.partition(":")
        if not colon or not start.strip():
            raise ValueError(f"--sequence: {part.strip()!r} is not `start_step: vx vy wz [...]`")
        try:
            at = float(start)
        except ValueError:
            raise ValueError(f"--sequence: the start step {start.strip()!r} of {part.strip()!r} is not a number")
        if not np.isfinite(at) or at != int(at):
            raise ValueError(f"--sequence: the start step {start.strip()!r} of {part.strip()!r} is not a whole number of steps")
        try:
            cmd = command_row(values.split())
        except ValueError as err:
            raise ValueError(f"--sequence: segment {part.strip()!r}: {err}")
        segs.append(dict(start_step=int(at), command=cmd))
    return segs


def check_schedule(schedule: Sequence[Dict], episode_length: Optional[int] = None) -> None:
    """What a schedule must satisfy before it reaches the device (the kernels cannot report it): 1 to 8 segments, the first at step 0,
    starts strictly increasing and below `episode_length` (when given), every command 7 finite values.  ValueError with the reason."""
    if not 1 <= len(schedule) <= SCHED_MAX_SEGMENTS:
        raise ValueError(f"a schedule has 1 to {SCHED_MAX_SEGMENTS} segments, this one has {len(schedule)}")
    if int(schedule[0]["start_step"]) != 0:
        raise ValueError(f"the first segment of a schedule starts at step 0 (the command the episode begins with), not at {schedule[0]['start_step']}")
    for i, seg in enumerate(schedule):
        at = int(seg["start_step"])
        if i and at <= int(schedule[i - 1]["start_step"]):
            raise ValueError(f"the start steps of a schedule increase: segment {i} starts at {at}, segment {i - 1} at {schedule[i - 1]['start_step']}")
        if episode_length is not None and at >= int(episode_length):
            raise ValueError(f"segment {i} starts at step {at}, at or beyond the episode's {int(episode_length)} steps (--episode_length): it would never run")
        cmd = np.asarray(seg["command"], np.float64).reshape(-1)
        with np.errstate(over="ignore"):      # a value past float32's range becomes inf there, which is the finding
            fits = cmd.shape == (7,) and bool(np.all(np.isfinite(cmd.astype(np.float32))))
        if not fits:
            raise ValueError(f"the command of segment {i} is not 7 finite values: {list(seg['command'])}")


def then_schedules(commands: Sequence[Sequence[float]], thens: Sequence[Sequence[float]], switch_at: int) -> List[List[Dict]]:
    """Every from-command crossed with every `--then` command: two-segment schedules that switch at step `switch_at`, the from-commands
    outermost (schedule c * len(thens) + k goes from commands[c] to thens[k]), like `cell_blocks`: the transition matrix of a grid."""
    return [[dict(start_step=0, command=[float(x) for x in c]), dict(start_step=int(switch_at), command=[float(x) for x in t])]
            for c in commands for t in thens]


def schedule_table(schedules: Sequence[Sequence[Dict]]) -> np.ndarray:
    """float32 [nsched, nseg, 8] for `Batch.command_schedule_apply`: nseg is the longest schedule's segment count, a row is start_step and
    the 7 command entries, and the unused trailing segments of a shorter schedule start at SCHED_NEVER (zero commands).  Every schedule
    is checked (`check_schedule`)."""
    if not schedules:
        raise ValueError("no schedule given")
    for s in schedules:
        check_schedule(s)
    nseg = max(len(s) for s in schedules)
    tab = np.zeros((len(schedules), nseg, SCHED_SEG_FLOATS), np.float32)
    tab[:, :, 0] = SCHED_NEVER
    for i, s in enumerate(schedules):
        for k, seg in enumerate(s):
            tab[i, k, 0] = float(int(seg["start_step"]))
            tab[i, k, 1:] = np.asarray(seg["command"], np.float32)
    return tab


def schedule_blocks(nsched: int, envs_per_schedule: int) -> np.ndarray:
    """int32 [nsched * envs_per_schedule], the env-to-schedule map: schedule s drives envs s * envs_per_schedule .. (s + 1) *
    envs_per_schedule - 1 (the blocks of `command_blocks`)."""
    return np.repeat(np.arange(int(nsched), dtype=np.int32), int(envs_per_schedule))


def reduce_response(acc: np.ndarray, schedules: Sequence[Sequence[Dict]], envs_per_block: int, dt: float) -> List[List[Dict]]:
    """Per schedule (a block of `envs_per_block` envs, in `schedule_blocks` order) the "segments" list of its row, from the response
    accumulator ([nenv, 8 * 24], include/odk.h ODK_RESP_*), in float64.  Per segment: `start_step`, `command`; `envs_entered`, the envs
    whose first episode ran a step in the segment; `velocity_samples` (steps that did not end the episode), pooled over the block;
    `mean_*` / `rms_error_*` of vx, vy, wz over those samples against the segment's command; `fall_rate`, the share of the entered envs
    whose first episode ended in the segment by falling, and `mean_steps_to_fall` from the segment's first step to the fall, counting
    both; `responded_fraction`, the share of the envs with a sample that came inside both tolerances at some sample, and
    `response_time_s`, the mean over those envs of the steps to the first such sample, times dt; `settled_fraction`, the share of the envs
    with a sample whose last sample was inside (LAST_OFF < SAMPLES), and `settle_time_s`, the mean over those envs of the steps to the
    last sample outside (0: never outside), times dt; `peak_lin_error` / `peak_ang_error`, the largest planar / yaw error any env of the
    block showed from its first sample inside onwards; `overshoot_v*`, the mean over the envs with a sample of the farthest the axis went
    past the command in the direction of the change (0 for an axis whose command did not change); `steady_state_error_v*`, the mean
    velocity over the samples later than `--response_tail_after` steps into the segment, minus the command.  A figure over an empty set
    is None: a segment without a sample has no means, one nobody responded to no response time, one without tail samples no steady state."""
    acc = np.asarray(acc, np.float64).reshape(-1, RESP_NACC)
    E, dt = int(envs_per_block), float(dt)
    out = []
    for s, sched in enumerate(schedules):
        segs = []
        for k, seg in enumerate(sched):
            blk = acc[s * E:(s + 1) * E, k * RESP_STRIDE:(k + 1) * RESP_STRIDE]
            cmd = [float(x) for x in seg["command"]]
            entered = blk[:, R_ENTERED] != 0
            n = blk[:, R_SAMPLES]
            live = n > 0
            samples = float(n.sum())
            fell = entered & (blk[:, R_FELL] != 0)
            responded = live & (blk[:, R_FIRST_IN] > 0)
            settled = live & (blk[:, R_LAST_OFF] < n)
            tail = float(blk[:, R_TAIL_SAMPLES].sum())
            g = dict(start_step=int(seg["start_step"]), command=cmd, envs_entered=int(entered.sum()), velocity_samples=int(round(samples)))
            for a, axis in enumerate(COMMAND_KEYS[:3]):
                g["mean_" + axis] = float(blk[:, R_SUM + a].sum() / samples) if samples > 0 else None
            for a, axis in enumerate(COMMAND_KEYS[:3]):
                g["rms_error_" + axis] = float(np.sqrt(blk[:, R_SQERR + a].sum() / samples)) if samples > 0 else None
            g.update(
                fall_rate=float(fell.sum() / entered.sum()) if entered.any() else None,
                mean_steps_to_fall=_mean_or_none(blk[fell, R_STEPS_TO_FALL]),
                responded_fraction=float(responded.sum() / live.sum()) if live.any() else None,
                response_time_s=float(blk[responded, R_FIRST_IN].mean() * dt) if responded.any() else None,
                settle_time_s=float(blk[settled, R_LAST_OFF].mean() * dt) if settled.any() else None,
                settled_fraction=float(settled.sum() / live.sum()) if live.any() else None,
                peak_lin_error=float(blk[responded, R_PEAK_LIN].max()) if responded.any() else None,
                peak_ang_error=float(blk[responded, R_PEAK_ANG].max()) if responded.any() else None)
            for a, axis in enumerate(COMMAND_KEYS[:3]):
                g["overshoot_" + axis] = float(blk[live, R_OVERSHOOT + a].mean()) if live.any() else None
            for a, axis in enumerate(COMMAND_KEYS[:3]):
                g["steady_state_error_" + axis] = float(blk[:, R_TAIL_SUM + a].sum() / tail - cmd[a]) if tail > 0 else None
            segs.append(g)
        out.append(segs)
    return out


SEGMENT_KEYS = ("start_step", "command", "envs_entered", "velocity_samples", "mean_vx", "mean_vy", "mean_wz", "rms_error_vx", "rms_error_vy",
                "rms_error_wz", "fall_rate", "mean_steps_to_fall", "responded_fraction", "response_time_s", "settle_time_s", "settled_fraction",
                "peak_lin_error", "peak_ang_error", "overshoot_vx", "overshoot_vy", "overshoot_wz", "steady_state_error_vx",
                "steady_state_error_vy", "steady_state_error_wz")
SCHEDULE_ROW_KEYS = ("schedule", "segments")


def response_tolerance(args) -> tuple:
    """`--response_tolerance LIN ANG` as odk_response_accumulate accepts it: two finite numbers >= 0; SystemExit otherwise."""
    tol = tuple(float(x) for x in getattr(args, "response_tolerance", None) or DEFAULT_PUSH_TOLERANCE)
    if len(tol) != 2 or not all(np.isfinite(x) and x >= 0 for x in tol):
        raise SystemExit(f"--response_tolerance LIN ANG: two finite errors >= 0 (m/s, rad/s), got {list(tol)}")
    return tol


def schedules_from_args(args) -> Optional[List[List[Dict]]]:
    """The schedules the command line asks for -- one per `--sequence`, or every `--command` / `--grid` row crossed with every `--then` --
    or None without a schedule flag.  SystemExit with the reason for a schedule that cannot run (`check_schedule`, against
    `--episode_length`), for `--then` without a from-command, for `--sequence` next to `--command` / `--grid` / `--then`, and for schedules next
    to pushes or `--posture`, whose figures assume one command per episode."""
    sequences, thens = getattr(args, "sequence", None) or [], getattr(args, "then", None) or []
    if not sequences and not thens:
        return None
    given = bool(getattr(args, "command", None)) or bool(getattr(args, "grid", None))
    if sequences and (given or thens):
        raise SystemExit("--sequence is a whole schedule of its own: it does not combine with --command, --grid or --then (write the commands into the sequence)")
    if thens and not given:
        raise SystemExit("--then switches away from a command: give the from-commands with --command or --grid")
    if getattr(args, "push", None) or getattr(args, "push_grid", None):
        raise SystemExit("command schedules (--sequence / --then) do not combine with --push / --push_grid: the push figures assume one command per episode")
    if getattr(args, "posture", False):
        raise SystemExit("command schedules (--sequence / --then) do not combine with --posture: its settle times assume one command per episode "
                         "(the response figures cover vx, vy and wz)")
    try:
        if sequences:
            schedules = [parse_sequence(text) for text in sequences]
        else:
            commands = [command_row(c) for c in (getattr(args, "command", None) or [])]
            if getattr(args, "grid", None):
                commands += parse_grid(args.grid)
            switch_at = int(getattr(args, "switch_at", DEFAULT_SWITCH_AT))
            schedules = then_schedules(commands, [command_row(t) for t in thens], switch_at)
        for i, sched in enumerate(schedules):
            try:
                check_schedule(sched, int(args.episode_length))
            except ValueError as err:
                raise ValueError(f"schedule {i}: {err}")
    except ValueError as err:
        raise SystemExit(str(err))
    response_tolerance(args)
    if int(getattr(args, "response_tail_after", DEFAULT_RESPONSE_TAIL_AFTER)) < 0:
        raise SystemExit("--response_tail_after is a number of steps: >= 0")
    return schedules


def reduce_pushes(acc: np.ndarray, commands: Sequence[Sequence[float]], pushes: Sequence[Dict], envs_per_cell: int, dt: float) -> List[Dict]:
    """Per command, what its rows of the report gain: {"pushes": [...], "max_push_survived": [...]}, from the push accumulator ([nenv, 10],
    include/odk.h ODK_PUSH_*) in `cell_blocks` order.  Per cell: `pushed_envs` counts the envs whose first episode reached the pushed step
    (the others ended before it and say nothing about the push); `fall_rate_after_push` is the share of the pushed envs that fell at or
    after it (0 when nobody was pushed) and `mean_steps_to_fall` their mean step count from the pushed step to the fall; the recovery
    statistics are over the survivors (pushed, did not fall): median and 90th percentile of the steps from the pushed step to the last
    velocity sample outside the tolerance (0: never outside), `recovery_time_s` = median * dt; the error peaks are means over the pushed
    envs; `pre_push_lin_err_mean` is the cell's mean planar velocity error over the samples before the push.  A figure over an empty set
    is None.  `max_push_survived`: per direction of the sweep, in order of first appearance, the largest magnitude whose cell has
    fall_rate_after_push == 0 among the cells where somebody was pushed (a cell whose envs all ended their first episode before the
    pushed step says nothing; the zero kick counts as survived) -- None when no magnitude of that direction was survived; a smaller
    magnitude with falls does not cap it."""
    acc = np.asarray(acc, np.float64).reshape(-1, PUSH_NACC)
    E, P = int(envs_per_cell), len(pushes)
    out = []
    for c, _ in enumerate(commands):
        cells = []
        for p, push in enumerate(pushes):
            blk = acc[(c * P + p) * E:(c * P + p + 1) * E]
            pushed = blk[:, P_PUSHED] != 0
            fell = pushed & (blk[:, P_FELL] != 0)
            ok = pushed & ~fell
            rec = blk[ok, P_LAST_OFF]
            med = float(np.median(rec)) if rec.size else None
            pre_n = float(blk[:, P_PRE_SAMPLES].sum())
            cells.append(dict(
                push=[float(x) for x in push["push"]], magnitude=float(push["magnitude"]), direction_deg=float(push["direction_deg"]),
                envs=E, pushed_envs=int(pushed.sum()),
                fall_rate_after_push=float(fell.sum() / max(int(pushed.sum()), 1)),
                mean_steps_to_fall=_mean_or_none(blk[fell, P_STEPS_TO_FALL]),
                recovery_steps_median=med,
                recovery_steps_p90=float(np.percentile(rec, 90)) if rec.size else None,
                recovery_time_s=med * float(dt) if med is not None else None,
                peak_lin_err_mean=_mean_or_none(blk[pushed, P_PEAK_LIN]),
                peak_ang_err_mean=_mean_or_none(blk[pushed, P_PEAK_ANG]),
                pre_push_lin_err_mean=float((blk[:, P_PRE_SUM] + blk[:, P_PRE_LOW]).sum() / pre_n) if pre_n > 0 else None,
            ))
        best: Dict[float, Optional[float]] = {}
        for cell in cells:
            d = cell["direction_deg"]
            best.setdefault(d, None)
            tried = cell["pushed_envs"] > 0 or cell["magnitude"] == 0.0      # a kick that reached nobody was not survived by anybody
            if tried and cell["fall_rate_after_push"] == 0.0 and (best[d] is None or cell["magnitude"] > best[d]):
                best[d] = cell["magnitude"]
        out.append(dict(pushes=cells, max_push_survived=[dict(direction_deg=d, magnitude=m) for d, m in best.items()]))
    return out


PUSH_ROW_KEYS = ("pushes", "max_push_survived")
PUSH_CELL_KEYS = ("push", "magnitude", "direction_deg", "envs", "pushed_envs", "fall_rate_after_push", "mean_steps_to_fall", "recovery_steps_median",
                  "recovery_steps_p90", "recovery_time_s", "peak_lin_err_mean", "peak_ang_err_mean", "pre_push_lin_err_mean")


def torque_limits(model) -> np.ndarray:
    """[nu] float32: actuator u's torque limit, `actuator_forcerange[u, 1]` where `actuator_forcelimited` is set, 0 for an actuator without a
    force range (`odk_gait_accumulate` never counts that one as saturated)."""
    fr = np.asarray(model.a["actuator_forcerange"], np.float64).reshape(-1, 2)
    on = np.asarray(model.a["actuator_forcelimited"]).reshape(-1) != 0
    return np.where(on, fr[:, 1], 0.0).astype(np.float32)


def nominal_weight(model) -> float:
    """m * g of the cost of transport: the compiled model's total body mass (not a randomised one) times the norm of its gravity."""
    return float(np.asarray(model.a["body_mass"], np.float64).sum() * np.linalg.norm(np.asarray(model.a["opt_gravity"], np.float64)))


MIN_COT_DISTANCE = 0.01      # metres: below it the cost of transport is a ratio of noise and is reported as None


def reduce_gait(acc: np.ndarray, commands: Sequence, envs_per_block: int, dt: float, model) -> List[Dict]:
    """One "gait" object per block of `envs_per_block` envs (a block per entry of `commands`: the command blocks of `command_blocks`, or the
    (command, push) cells of `cell_blocks`), from the gait accumulator ([nenv, 144], include/odk.h ODK_GAIT_*), in float64.  Sums are pooled
    over the block's gait samples (the steps of the envs' first episodes that did not end them); [L, R] = left, right foot:
    `duty_factor` the share of samples with the foot in contact; `double_support_fraction` / `flight_fraction` with both / no foot in
    contact; `step_frequency_hz` = touchdowns / (samples * dt); `mean_swing_time_s` = mean non-contact run before a touchdown * dt (None
    without a touchdown); `foot_slip_mps` the mean planar foot speed over the foot's contact samples (None without one);
    `root_height_mean` / `root_height_std`; `roll_pitch_rate_rms` = sqrt(mean(gyro_x^2 + gyro_y^2)); `action_rate_mean` = mean over samples
    of sum_u (last_act - last_last_act)^2; `mean_abs_power_w` = mean over samples of sum_u |force * joint_vel|; `cost_of_transport` =
    ABS_POWER_SUM / (m g SPEED_SUM) with m the model's nominal total mass and g its gravity (`nominal_weight`), None when the distance
    SPEED_SUM * dt is under 1 cm; `actuators`: by name, `torque_rms`, `torque_peak` (max over the block), `torque_limit` (`torque_limits`,
    0 = none), `saturation_fraction` (share of samples at >= 99 % of the limit), `velocity_peak`, `mean_abs_power_w`, `range` [min, max] of
    the joint angle minus the default pose ([None, None] without a sample).  A block without samples reports 0 for the means."""
    acc = np.asarray(acc, np.float64).reshape(-1, GAIT_NACC)
    E, dt = int(envs_per_block), float(dt)
    nu = int(model.nu)
    names = [str(n) for n in model.a["names_actuator"]]
    limit = torque_limits(model).astype(np.float64)
    weight = nominal_weight(model)
    pair = lambda blk, s: blk[:, s:s + 2].sum(0)
    out = []
    for c, _ in enumerate(commands):
        blk = acc[c * E:(c + 1) * E]
        live = blk[:, G_SAMPLES] > 0
        samples = float(blk[:, G_SAMPLES].sum())
        den = max(samples, 1.0)
        contact, touch, swing, slip = pair(blk, G_CONTACT), pair(blk, G_TOUCH), pair(blk, G_SWING), pair(blk, G_SLIP)
        h_mean = float(blk[:, G_HEIGHT].sum() / den)
        speed, power = float(blk[:, G_SPEED].sum()), float(blk[:, G_POWER].sum())
        arr = lambda s: blk[:, s:s + nu]
        actuators = {}
        for u in range(nu):
            actuators[names[u]] = dict(
                torque_rms=float(np.sqrt(arr(G_TORQUE_SQ)[:, u].sum() / den)), torque_peak=float(arr(G_TORQUE_PEAK)[:, u].max()),
                torque_limit=float(limit[u]), saturation_fraction=float(arr(G_SAT)[:, u].sum() / den),
                velocity_peak=float(arr(G_VEL_PEAK)[:, u].max()), mean_abs_power_w=float(arr(G_ABS_POWER)[:, u].sum() / den),
                range=[float(arr(G_RANGE_MIN)[live, u].min()), float(arr(G_RANGE_MAX)[live, u].max())] if live.any() else [None, None])
        out.append(dict(
            samples=int(round(samples)),
            duty_factor=[float(x / den) for x in contact],
            double_support_fraction=float(blk[:, G_DOUBLE].sum() / den), flight_fraction=float(blk[:, G_FLIGHT].sum() / den),
            step_frequency_hz=[float(x / (den * dt)) for x in touch],
            mean_swing_time_s=[float(s / n * dt) if n > 0 else None for s, n in zip(swing, touch)],
            foot_slip_mps=[float(s / n) if n > 0 else None for s, n in zip(slip, contact)],
            root_height_mean=h_mean, root_height_std=float(np.sqrt(max(blk[:, G_HEIGHT_SQ].sum() / den - h_mean * h_mean, 0.0))),
            roll_pitch_rate_rms=float(np.sqrt(blk[:, G_WOBBLE].sum() / den)),
            action_rate_mean=float(blk[:, G_ARATE].sum() / den),
            mean_abs_power_w=power / den,
            cost_of_transport=power / (weight * speed) if speed * dt >= MIN_COT_DISTANCE else None,
            actuators=actuators,
        ))
    return out


GAIT_KEYS = ("samples", "duty_factor", "double_support_fraction", "flight_fraction", "step_frequency_hz", "mean_swing_time_s", "foot_slip_mps",
             "root_height_mean", "root_height_std", "roll_pitch_rate_rms", "action_rate_mean", "mean_abs_power_w", "cost_of_transport", "actuators")
GAIT_ACTUATOR_KEYS = ("torque_rms", "torque_peak", "torque_limit", "saturation_fraction", "velocity_peak", "mean_abs_power_w", "range")


# BUILD-DEFINED default (the reference has no such measure): a head joint counts as settled within 0.1 rad (under 6 degrees) of its command
DEFAULT_POSTURE_TOLERANCE = 0.1
HEAD_SLOTS = COMMAND_KEYS[3:]      # constants.HEAD_SLOTS: the posture commands, in the order of the head-joint map


def posture_tolerance(text: str) -> float:
    """`--posture_tolerance RAD`: a finite number >= 0 (what odk_posture_accumulate accepts)."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number")
    if not np.isfinite(v) or v < 0:
        raise argparse.ArgumentTypeError(f"{text}: a tolerance is a finite angle >= 0, in radians")
    return v


def posture_head_map(env):
    """(head_map, joint_names) of `reduce_posture` for an env: the head-joint map its batch holds -- the Standing task's `head_joints`, the
    duck's own actuators 5..8 otherwise -- and, per actuator, the name of the joint it drives.  ValueError for the Joystick task on another
    robot: that batch has no head-joint map (odk_posture_accumulate would refuse it)."""
    model = env.mj_model
    hmap = env.head_joints
    if hmap is None:
        from . import constants
        if not constants.robot_of(model).is_open_duck:
            raise ValueError("--posture: the joystick env on a robot that is not the duck has no head-joint map; give it one with "
                             "--env standing --head_joints SLOT=JOINT[,SLOT=JOINT...] (or --head_joints none for the stillness part alone)")
        hmap = [5, 6, 7, 8]
    jn = [str(n) for n in model.a["names_jnt"]]
    trn = [int(j) for j in np.asarray(model.a["actuator_trnid"]).reshape(model.nu, -1)[:, 0]]
    return [int(u) for u in hmap], [jn[j] for j in trn]


def reduce_posture(acc: np.ndarray, commands: Sequence[Sequence[float]], envs_per_block: int, dt: float, head_map: Sequence[int],
                   joint_names: Sequence[str]) -> List[Dict]:
    """One "posture" object per block of `envs_per_block` envs (a block per entry of `commands`, whose entries 3..6 are the block's posture
    commands: the command blocks of `command_blocks`, or the (command, push) cells of `cell_blocks`), from the posture accumulator
    ([nenv, 32], include/odk.h ODK_POSTURE_*), in float64.  `head_map[k]` is the actuator of head slot k (-1: none), `joint_names[u]` the
    joint actuator u drives.  Sums are pooled over the block's samples (the steps of the envs' first episodes that did not end them).
    Per mapped slot, under the slot's name (an unmapped slot is absent): `joint`, `command`, `mean_angle` (the absolute joint angle),
    `rms_error` and `peak_error` (max over the block) of angle - command; `settle_time_s` = the mean over the envs that settled of LAST_OFF
    * dt -- the time of the last sample outside the tolerance, 0 for an env that never left it; `settled_fraction` = the share, among the
    envs with a sample, of those whose LAST_OFF < SAMPLES: the last sample was inside the tolerance.  An env still outside at its last sample
    has no settle time and is left out of that mean (None when nobody settled).  `head_cost_mean` = mean over samples of the summed squared
    error (cost_head_pos without its move-command gate).  `stillness`: `drift_speed_mps` mean planar speed, `yaw_rate_rms`,
    `roll_pitch_rate_rms` = sqrt(mean(gyro_x^2 + gyro_y^2)), `tilt_mean` / `tilt_peak` of the sine of the lean, `root_height_mean`,
    `leg_pose_deviation_mean` / `leg_joint_speed_mean` = mean over samples of the sum over the joints no slot maps to of |angle - default| /
    |joint_vel| (the two parts of cost_stand_still(ignore_head=True)).  A block without a sample has nothing to average: every figure is None."""
    acc = np.asarray(acc, np.float64).reshape(-1, POSTURE_NACC)
    E, dt = int(envs_per_block), float(dt)
    out = []
    for c, cmd in enumerate(commands):
        blk = acc[c * E:(c + 1) * E]
        n = blk[:, S_SAMPLES]
        live = n > 0
        samples = float(n.sum())
        mean = lambda s: float(blk[:, s].sum() / samples) if samples > 0 else None
        rms = lambda s: float(np.sqrt(blk[:, s].sum() / samples)) if samples > 0 else None
        peak = lambda s: float(blk[live, s].max()) if samples > 0 else None
        g = dict(samples=int(round(samples)))
        for k, slot in enumerate(HEAD_SLOTS):
            u = int(head_map[k])
            if u < 0:
                continue
            off = blk[:, S_LAST_OFF + k]
            settled = live & (off < n)
            g[slot] = dict(
                joint=str(joint_names[u]), command=float(cmd[3 + k]), mean_angle=mean(S_ANGLE + k), rms_error=rms(S_ERR_SQ + k),
                peak_error=peak(S_ERR_PEAK + k), settle_time_s=float(off[settled].mean() * dt) if settled.any() else None,
                settled_fraction=float(settled.sum() / live.sum()) if samples > 0 else None)
        g["head_cost_mean"] = mean(S_HEAD_SQERR)
        g["stillness"] = dict(
            drift_speed_mps=mean(S_DRIFT), yaw_rate_rms=rms(S_YAW), roll_pitch_rate_rms=rms(S_WOBBLE), tilt_mean=mean(S_TILT),
            tilt_peak=peak(S_TILT_PEAK), root_height_mean=mean(S_HEIGHT), leg_pose_deviation_mean=mean(S_LEG_POSE),
            leg_joint_speed_mean=mean(S_LEG_VEL))
        out.append(g)
    return out


POSTURE_SLOT_KEYS = ("joint", "command", "mean_angle", "rms_error", "peak_error", "settle_time_s", "settled_fraction")
STILLNESS_KEYS = ("drift_speed_mps", "yaw_rate_rms", "roll_pitch_rate_rms", "tilt_mean", "tilt_peak", "root_height_mean", "leg_pose_deviation_mean",
                  "leg_joint_speed_mean")


JOINT_POS_WEIGHT, JOINT_VEL_WEIGHT = 15.0, 1.0e-3      # the imitation reward's weights of its joint terms (custom_rewards.py:127-128)
FEET = ("left", "right")


def imitation_refusal(args) -> Optional[str]:
    """Why `--imitation_report` cannot run with these arguments, or None.  Host work only (at most the robot's MJCF is compiled), so `run`
    asks before it makes a batch: the Standing task has no reference-motion frame in its privileged row, and a robot that is not the duck
    runs without the imitation reward unless `--reference_motion` gives it a table."""
    if args.env != "joystick":
        return (f"--imitation_report: the {args.env} env has no imitation reward and no reference-motion frame in its privileged observation; "
                "the report belongs to --env joystick")
    if getattr(args, "xml", None) and not getattr(args, "reference_motion", None):
        from . import constants
        from .model import Model
        if not constants.robot_of(Model.from_xml(args.xml)).is_open_duck:
            return ("--imitation_report: a robot that is not the duck runs without the imitation reward (the shipped table is the duck's), so there "
                    "is no reference motion to compare with; give the robot's own with --reference_motion polynomial_coefficients.pkl")
    return None


def imitation_joint_info(env):
    """(imap, joint_names, period_steps) of `reduce_imitation` and `Tracker(imitation=True)` for an env: the imitation joint map its batch
    holds (frame joint per actuator, -1: not compared), per actuator the name of the joint it drives, and the reference motion's
    nb_steps_in_period -- the `reference_motion` key's, or the shipped table's for the duck.  ValueError for an env without the reward."""
    from .reference_motion import ReferenceMotion, actuated_joint_names
    imap = env.imitation_joints
    if imap is None:
        raise ValueError("--imitation_report: the env runs without the imitation reward (the Standing task, or a robot that is not the duck "
                         "without --reference_motion)")
    motion = env.reference_motion
    period = motion.nb_steps_in_period if motion is not None else ReferenceMotion.from_npz().nb_steps_in_period
    return [int(j) for j in imap], actuated_joint_names(env.mj_model), int(period)


def reduce_imitation(acc: np.ndarray, commands: Sequence, envs_per_block: int, dt: float, imap: Sequence[int], joint_names: Sequence[str],
                     period_steps: int) -> List[Dict]:
    """One "imitation" object per block of `envs_per_block` envs (a block per entry of `commands`: the command blocks of `command_blocks`,
    or the (command, push) cells of `cell_blocks`), from the imitation accumulator ([nenv, 160], include/odk.h ODK_IMIT_*), in float64.
    `imap[u]` is the frame joint of actuator u (-1: not compared), `joint_names[u]` the joint it drives.  Sums are pooled over the block's
    samples (the steps of the envs' first episodes that did not end them), so an env weighs by its samples.  `gated_share`: the share of
    samples with a move command, those the reward pays.  `joints`: one entry per compared actuator, in actuator order -- `joint`,
    `frame_joint`, `bias` (mean of angle - reference), `rms_error`, `peak_error` (max over the block), `vel_rms_error`, `range` and
    `reference_range` ([min, max] over the block of the joint angle and of the reference's) and `amplitude_ratio` = the width of the former
    over the latter's (None for a reference that does not move).  `joint_pos_term` / `joint_vel_term`: the mean over samples of the summed
    squared position / velocity error times the reward's weights 15 and 1e-3.  `feet` (left, right): `contact_agreement` the share of
    samples whose contact equals the reference's, `stance_share` / `reference_stance_share`, `touchdowns` (the robot's, from the reference's
    first touchdown on: those with a lag) and `reference_touchdowns`, `touchdown_lag_steps` the mean signed lag behind the reference's
    touchdown (negative: early for the next one; folded at half of `period_steps`), `touchdown_lag_s` = that times dt,
    `touchdown_lag_abs_steps` the mean |lag|; None without a counted touchdown.  `contact_term`: the agreements of both feet added, the
    mean of the reward's contact term.  `speed_rms_error` / `reference_speed_mean`: planar speed against the frame's.  A block without a
    sample has nothing to average: its figures are None."""
    acc = np.asarray(acc, np.float64).reshape(-1, IMIT_NACC)
    E, dt = int(envs_per_block), float(dt)
    out = []
    for c, _ in enumerate(commands):
        blk = acc[c * E:(c + 1) * E]
        n = blk[:, I_SAMPLES]
        live = n > 0
        samples = float(n.sum())
        some = samples > 0
        mean = lambda s: float(blk[:, s].sum() / samples) if some else None
        rms = lambda s: float(np.sqrt(blk[:, s].sum() / samples)) if some else None
        joints = []
        for u, ri in enumerate(imap):
            if ri < 0:
                continue
            lo, hi = (float(blk[live, I_RANGE_MIN + u].min()), float(blk[live, I_RANGE_MAX + u].max())) if some else (None, None)
            rlo, rhi = (float(blk[live, I_REF_RANGE_MIN + u].min()), float(blk[live, I_REF_RANGE_MAX + u].max())) if some else (None, None)
            joints.append(dict(
                joint=str(joint_names[u]), frame_joint=int(ri), bias=mean(I_POS_ERR + u), rms_error=rms(I_POS_ERR_SQ + u),
                peak_error=float(blk[live, I_POS_ERR_PEAK + u].max()) if some else None, vel_rms_error=rms(I_VEL_ERR_SQ + u),
                range=[lo, hi], reference_range=[rlo, rhi], amplitude_ratio=float((hi - lo) / (rhi - rlo)) if some and rhi > rlo else None))
        feet = []
        for f, name in enumerate(FEET):
            both, ronly, fonly = (float(blk[:, s + f].sum()) for s in (I_BOTH, I_ROBOT_ONLY, I_REF_ONLY))
            td, lag, lag_abs = (float(blk[:, s + f].sum()) for s in (I_TOUCH, I_LAG, I_LAG_ABS))
            feet.append(dict(
                foot=name, contact_agreement=float(1.0 - (ronly + fonly) / samples) if some else None,
                stance_share=float((both + ronly) / samples) if some else None, reference_stance_share=float((both + fonly) / samples) if some else None,
                touchdowns=int(round(td)), reference_touchdowns=int(round(float(blk[:, I_REF_TOUCH + f].sum()))),
                touchdown_lag_steps=float(lag / td) if td > 0 else None, touchdown_lag_s=float(lag / td * dt) if td > 0 else None,
                touchdown_lag_abs_steps=float(lag_abs / td) if td > 0 else None))
        jp, jv = mean(I_JOINT_POS_SQ), mean(I_JOINT_VEL_SQ)
        out.append(dict(
            samples=int(round(samples)), gated_share=mean(I_GATED), period_steps=int(period_steps), joints=joints,
            joint_pos_term=JOINT_POS_WEIGHT * jp if some else None, joint_vel_term=JOINT_VEL_WEIGHT * jv if some else None, feet=feet,
            contact_term=float(sum(ft["contact_agreement"] for ft in feet)) if some else None,
            speed_rms_error=rms(I_SPEED_ERR_SQ), reference_speed_mean=mean(I_REF_SPEED)))
    return out


IMITATION_KEYS = ("samples", "gated_share", "period_steps", "joints", "joint_pos_term", "joint_vel_term", "feet", "contact_term", "speed_rms_error",
                  "reference_speed_mean")
IMITATION_JOINT_KEYS = ("joint", "frame_joint", "bias", "rms_error", "peak_error", "vel_rms_error", "range", "reference_range", "amplitude_ratio")
IMITATION_FOOT_KEYS = ("foot", "contact_agreement", "stance_share", "reference_stance_share", "touchdowns", "reference_touchdowns",
                       "touchdown_lag_steps", "touchdown_lag_s", "touchdown_lag_abs_steps")


DEFAULT_FALL_RING = 50        # one second at the duck's ctrl_dt of 0.02 s
DEFAULT_FALL_TILT = 0.35      # BUILD-DEFINED default (the reference has no such measure): a lean of 20 degrees still counts as upright
DEFAULT_SAVE_FALLS_MAX = 16
FALL_SECTORS = ("forward", "left", "backward", "right")      # 90-degree sectors of atan2(d_y, d_x), centred on +x, +y, -x, -y
MIN_FALL_DIRECTION = 1e-6      # a body-frame lean shorter than this has no direction


def falls_refusal(args) -> Optional[str]:
    """Why the fall flags cannot run as given, or None.  Host work only, so `run` asks before it makes a batch."""
    if getattr(args, "save_falls", None) and not getattr(args, "falls", False):
        return "--save_falls writes the clips of the fall report: give --falls too"
    ring = getattr(args, "fall_ring", DEFAULT_FALL_RING)
    if int(ring) != ring or not 1 <= int(ring) <= FALL_MAX_RING:
        return f"--fall_ring is a number of samples from 1 to {FALL_MAX_RING}, got {ring}"
    tilt = float(getattr(args, "fall_tilt", DEFAULT_FALL_TILT))
    if not np.isfinite(tilt) or tilt < 0 or tilt > np.pi / 2:
        return f"--fall_tilt is a lean in radians: finite, >= 0 and at most pi / 2, got {tilt}"
    if int(getattr(args, "save_falls_max", DEFAULT_SAVE_FALLS_MAX)) < 1:
        return f"--save_falls_max is a number of clips >= 1, got {args.save_falls_max}"
    return None


def fall_tilt_tol(rad: float) -> float:
    """`--fall_tilt RAD` as odk_fall_accumulate takes it: the sine of the lean, as the float32 the launch receives."""
    return float(np.float32(np.sin(float(rad))))


def fall_ring_order(n: int, ring: int) -> np.ndarray:
    """The slots of a ring of `ring` that hold samples after `n` of them, oldest first: min(n, ring) slots, starting at slot n % ring once
    n >= ring and at slot 0 before.  The one unrolling rule of `reduce_falls` and `fall_clips`."""
    n, ring = int(n), int(ring)
    start = n % ring if n >= ring else 0
    return (start + np.arange(min(n, ring), dtype=np.int64)) % ring


def fall_rows(acc: np.ndarray, ring: int, nq: int):
    """(head [nenv, FALL_HEAD], slots [nenv, ring, FALL_SAMPLE + nq]) views of a fall accumulator whose rows may be wider than they need."""
    acc = np.asarray(acc)
    w = FALL_SAMPLE + int(nq)
    nfl = FALL_HEAD + int(ring) * w
    if acc.ndim != 2 or acc.shape[1] < nfl:
        raise ValueError(f"a fall accumulator of ring {ring} and nq {nq} has rows of at least {nfl} floats, got {acc.shape}")
    return acc[:, :FALL_HEAD], acc[:, FALL_HEAD:nfl].reshape(acc.shape[0], int(ring), w)


def _quartiles(x: np.ndarray, scale: float = 1.0) -> Dict:
    if not x.size:
        return dict(q25=None, median=None, q75=None)
    q = np.percentile(np.asarray(x, np.float64), [25, 50, 75]) * scale
    return dict(q25=float(q[0]), median=float(q[1]), q75=float(q[2]))


def _spread(x: np.ndarray, scale: float = 1.0) -> Dict:
    x = np.asarray(x, np.float64)
    return dict(min=float(x.min() * scale) if x.size else None, **_quartiles(x, scale), max=float(x.max() * scale) if x.size else None)


def _mean_unit(v: np.ndarray) -> Optional[List[float]]:
    """Mean of the unit vectors of the rows of v [k, 2] that have a direction; None without one."""
    v = np.asarray(v, np.float64).reshape(-1, 2)
    r = np.hypot(v[:, 0], v[:, 1])
    ok = r > 0
    if not ok.any():
        return None
    m = (v[ok] / r[ok, None]).mean(0)
    return [float(m[0]), float(m[1])]


def body_lean(quat: np.ndarray) -> np.ndarray:
    """d = -(R(q)^T e_z)[0:2] for base quaternions [k, 4] (w x y z, normalised here): the planar part, in the base body's frame, of the
    direction the body leans to -- +x forward, +y left.  A zero quaternion gives a zero d."""
    q = np.asarray(quat, np.float64).reshape(-1, 4)
    nrm = np.linalg.norm(q, axis=1, keepdims=True)
    q = q / np.where(nrm > 0, nrm, 1.0)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return -np.stack([2.0 * (x * z - w * y), 2.0 * (y * z + w * x)], axis=1)


def reduce_falls(acc: np.ndarray, commands: Sequence, envs_per_block: int, dt: float, ring: int, nq: int) -> List[Dict]:
    """One "falls" object per block of `envs_per_block` envs (a block per entry of `commands`: the command blocks of `command_blocks`, the
    (command, push) cells of `cell_blocks` or the schedules of `schedule_blocks`), from the fall accumulator ([nenv, >= FALL_HEAD + ring *
    (FALL_SAMPLE + nq)], include/odk.h ODK_FALL_*), in float64.  A fall is an env with FELL set; its ring is unrolled by `fall_ring_order`.
    `episodes` the block's envs, `falls`, `fall_rate`; `fall_step` / `fall_time_s` = FALL_STEP (* dt): min, q25, median, q75, max over the
    falls.  `direction`, from the last sample of each fall: shares of `forward`, `left`, `backward`, `right` -- the 90-degree sector of
    atan2(d_y, d_x), d = `body_lean` of the sample's base quaternion qpos[3:7] -- and of `undetermined` (no sample: the fall ended step 0;
    or |d| < 1e-6), `mean_unit_vector` of d over the determined falls and `world_mean_unit_vector` of the sample's up vector's (x, y).
    `onset`: `samples` and `seconds` (q25, median, q75) from the last upright sample (LAST_UPRIGHT, lean within the tolerance) to the
    termination, SAMPLES - LAST_UPRIGHT + 1, over the falls that were upright at some sample; `never_upright` the share of the falls that
    never were; `support_at_onset` the shares of `left`, `right`, `both`, `none` of UPRIGHT_CONTACT over the former.  `saturated_before`:
    the share of falls with S_SAT > 0 at a sample in the ring.  `tilt_peak_survivors`: `envs`, `mean` and `max` of TILT_PEAK over the
    block's envs that did not fall.  `profile`: lists of length `ring`, entry k - 1 for the k-th last sample before the termination --
    `count` of falls that have one, and over them the means of `tilt` = hypot(up_x, up_y), `root_height`, `roll_pitch_rate` =
    hypot(gyro_x, gyro_y), `lin_error` and `saturated_actuators`; None where the count is 0.  A figure over an empty set is None."""
    head, slots = fall_rows(acc, ring, nq)
    head, slots = head.astype(np.float64), slots.astype(np.float64)
    E, dt, ring = int(envs_per_block), float(dt), int(ring)
    out = []
    for c, _ in enumerate(commands):
        H, S = head[c * E:(c + 1) * E], slots[c * E:(c + 1) * E]
        fell = H[:, F_FELL] != 0
        idx = np.flatnonzero(fell)
        k = int(idx.size)
        n = H[idx, F_SAMPLES].astype(np.int64)
        share = lambda m: float(np.count_nonzero(m) / k) if k else None
        # direction: the last sample of every fall that has one
        has = n > 0
        last = S[idx[has], (n[has] - 1) % ring]
        d = body_lean(last[:, FALL_SAMPLE + 3:FALL_SAMPLE + 7])
        det = np.hypot(d[:, 0], d[:, 1]) >= MIN_FALL_DIRECTION
        sector = np.floor(((np.arctan2(d[:, 1], d[:, 0]) + np.pi / 4) % (2 * np.pi)) / (np.pi / 2)).astype(np.int64) % 4
        direction = {name: share(det & (sector == i)) for i, name in enumerate(FALL_SECTORS)}
        direction = dict(forward=direction["forward"], backward=direction["backward"], left=direction["left"], right=direction["right"],
                         undetermined=float((k - np.count_nonzero(det)) / k) if k else None,
                         mean_unit_vector=_mean_unit(d[det]), world_mean_unit_vector=_mean_unit(last[:, FS_UP:FS_UP + 2]))
        # onset
        lu = H[idx, F_LAST_UPRIGHT]
        was = lu > 0
        gap = n[was] - lu[was] + 1
        cl, cr = H[idx[was], F_UPRIGHT_CONTACT] != 0, H[idx[was], F_UPRIGHT_CONTACT + 1] != 0
        nw = int(np.count_nonzero(was))
        sup = lambda m: float(np.count_nonzero(m) / nw) if nw else None
        onset = dict(samples=_quartiles(gap), seconds=_quartiles(gap, dt), never_upright=share(~was),
                     support_at_onset=dict(left=sup(cl & ~cr), right=sup(cr & ~cl), both=sup(cl & cr), none=sup(~cl & ~cr)))
        # the rings in time order, aligned at the termination: column k - 1 is the k-th last sample
        count = np.zeros(ring, np.int64)
        sums = np.zeros((5, ring))
        sat_any = np.zeros(k, bool)
        for i, e in enumerate(idx):
            r = S[e, fall_ring_order(n[i], ring)][::-1]
            m = r.shape[0]
            count[:m] += 1
            sums[0, :m] += np.hypot(r[:, FS_UP], r[:, FS_UP + 1])
            sums[1, :m] += r[:, FS_HEIGHT]
            sums[2, :m] += np.hypot(r[:, FS_GYRO], r[:, FS_GYRO + 1])
            sums[3, :m] += r[:, FS_LIN_ERR]
            sums[4, :m] += r[:, FS_SAT]
            sat_any[i] = bool((r[:, FS_SAT] > 0).any())
        prof = lambda j: [float(sums[j, i] / count[i]) if count[i] else None for i in range(ring)]
        surv = H[~fell, F_TILT_PEAK]
        out.append(dict(
            episodes=E, falls=k, fall_rate=float(k / E) if E else None,
            fall_step=_spread(H[idx, F_STEP]), fall_time_s=_spread(H[idx, F_STEP], dt),
            direction=direction, onset=onset, saturated_before=share(sat_any),
            tilt_peak_survivors=dict(envs=int(surv.size), mean=_mean_or_none(surv), max=float(surv.max()) if surv.size else None),
            profile=dict(count=[int(x) for x in count], tilt=prof(0), root_height=prof(1), roll_pitch_rate=prof(2), lin_error=prof(3),
                         saturated_actuators=prof(4))))
    return out


FALL_KEYS = ("episodes", "falls", "fall_rate", "fall_step", "fall_time_s", "direction", "onset", "saturated_before", "tilt_peak_survivors", "profile")
FALL_DIRECTION_KEYS = ("forward", "backward", "left", "right", "undetermined", "mean_unit_vector", "world_mean_unit_vector")
FALL_PROFILE_KEYS = ("count", "tilt", "root_height", "roll_pitch_rate", "lin_error", "saturated_actuators")
FALL_CLIP_KEYS = ("qpos", "valid", "steps", "env", "row", "fall_step", "command")


def fall_clips(acc: np.ndarray, commands: Sequence[Sequence[float]], envs_per_block: int, ring: int, nq: int, max_per_block: int) -> Dict:
    """The pre-fall clips `--save_falls` writes: the first `max_per_block` falls of every block (`reduce_falls`'s blocks, `commands[b]` the 7
    command entries of block b), in env order.  `qpos` [k, ring, nq] float32 in time order (`fall_ring_order`), zero-padded at the FRONT:
    clip i's real samples are qpos[i, ring - valid[i]:], the last one the step before the termination; `valid` [k] int32; `steps` [k, ring]
    int32, the first-episode step index of every sample (-1 in the padding); `env` [k], `row` [k] (the block) and `fall_step` [k] int32;
    `command` [k, 7] float32."""
    head, slots = fall_rows(acc, ring, nq)
    E, ring, nq = int(envs_per_block), int(ring), int(nq)
    envs = [e for b, _ in enumerate(commands) for e in (b * E + np.flatnonzero(head[b * E:(b + 1) * E, F_FELL] != 0)[:int(max_per_block)])]
    k = len(envs)
    clips = dict(qpos=np.zeros((k, ring, nq), np.float32), valid=np.zeros(k, np.int32), steps=np.full((k, ring), -1, np.int32),
                 env=np.asarray(envs, np.int32).reshape(k), row=np.zeros(k, np.int32), fall_step=np.zeros(k, np.int32),
                 command=np.zeros((k, 7), np.float32))
    for i, e in enumerate(envs):
        r = slots[e, fall_ring_order(head[e, F_SAMPLES], ring)]
        m = r.shape[0]
        clips["valid"][i] = m
        if m:
            clips["qpos"][i, ring - m:] = r[:, FALL_SAMPLE:]
            clips["steps"][i, ring - m:] = r[:, FS_STEP].astype(np.int32)
        clips["row"][i] = e // E
        clips["fall_step"][i] = int(head[e, F_STEP])
        clips["command"][i] = np.asarray(commands[e // E], np.float32)[:7]
    return clips


def save_falls(path: str, clips: Dict, dt: float) -> None:
    """`fall_clips` and the control step as an .npz: qpos[i, ring - valid[i]:] with dt has `--save_qpos`'s meaning."""
    np.savez(path, dt=np.float64(dt), **clips)


# BUILD-DEFINED defaults: controller settings of the waypoint follower, not measured constants (the reference has no follower).  A waypoint
# counts as reached within 5 cm; the follower cruises at 0.1 m/s, turns at up to 0.6 rad/s with 2 rad/s per unit sine of the heading error,
# and slows down inside 10 cm of the last waypoint
DEFAULT_WAYPOINT_RADIUS = 0.05
DEFAULT_WAYPOINT_SPEED = 0.1
DEFAULT_WAYPOINT_TURN_RATE = 0.6
DEFAULT_WAYPOINT_GAIN = 2.0
DEFAULT_WAYPOINT_SLOW_DIST = 0.1


def parse_waypoints(text: str) -> List[List[float]]:
    """`--waypoints "0.5,0 | 0.5,0.5 | 0,0.5 | 0,0"` -> one course: its points [x, y] in start-frame metres, apart by `|`.  ValueError for
    a point that is not `x,y`, a coordinate that is not a number, and (`check_course`) a course of no point or of more than 8."""
    points = []
    for part in str(text).split("|"):
        if not part.strip():
            continue
        bits = part.split(",")
        if len(bits) != 2:
            raise ValueError(f"--waypoints: {part.strip()!r} is not `x,y`")
        try:
            points.append([float(bits[0]), float(bits[1])])
        except ValueError:
            raise ValueError(f"--waypoints: the point {part.strip()!r} is not two numbers")
    check_course(points)
    return points


def check_course(points: Sequence[Sequence[float]]) -> None:
    """What a course must satisfy before it reaches the device (the kernels cannot report it): 1 to 8 points of two finite float32 values.
    ValueError with the reason."""
    if not 1 <= len(points) <= PATH_MAX_WAYPOINTS:
        raise ValueError(f"--waypoints: a course has 1 to {PATH_MAX_WAYPOINTS} points, this one has {len(points)}")
    for i, p in enumerate(points):
        v = np.asarray(p, np.float64).reshape(-1)
        with np.errstate(over="ignore"):
            fits = v.shape == (2,) and bool(np.all(np.isfinite(v.astype(np.float32))))
        if not fits:
            raise ValueError(f"--waypoints: point {i} is not two finite numbers: {list(p)}")


def course_table(courses: Sequence[Sequence[Sequence[float]]]) -> np.ndarray:
    """float32 [ncourse, 17] for `Batch.path_accumulate` / `Batch.waypoint_command_apply`: a row is the course's count, then its points
    x0 y0 x1 y1 ..., zeros past the last.  Every course is checked (`check_course`)."""
    if not courses:
        raise ValueError("no course given")
    tab = np.zeros((len(courses), PATH_COURSE_FLOATS), np.float32)
    for i, pts in enumerate(courses):
        check_course(pts)
        tab[i, 0] = float(len(pts))
        tab[i, 1:1 + 2 * len(pts)] = np.asarray(pts, np.float32).reshape(-1)
    return tab


def course_of_envs(course_map: np.ndarray, ncourse: int) -> np.ndarray:
    """The course every env really follows: the map entry clamped into 0 .. ncourse - 1, as the kernels clamp it."""
    return np.clip(np.asarray(course_map, np.int64), 0, int(ncourse) - 1)


def course_length(points: Sequence[Sequence[float]]) -> float:
    """Length of the polyline origin -> point 0 -> ... -> the last point, in float64."""
    p = np.concatenate([np.zeros((1, 2)), np.asarray(points, np.float64).reshape(-1, 2)])
    return float(np.hypot(*np.diff(p, axis=0).T).sum())


def waypoint_limits_refusal(speed: float, turn_rate: float, cmd_range) -> Optional[str]:
    """`--waypoint_speed` / `--waypoint_turn_rate` against the env's `cmd_range` (rows vx and wz; [lo, hi] each): the follower commands vx in
    0 .. speed and wz in -turn_rate .. turn_rate, which the policy must have been trained on.  The reason, or None."""
    vx, wz = [float(x) for x in cmd_range[0]], [float(x) for x in cmd_range[2]]
    if float(speed) > vx[1]:
        return f"--waypoint_speed {float(speed)} is beyond the env's command range for vx, {vx[0]} .. {vx[1]} m/s"
    if float(turn_rate) > wz[1] or -float(turn_rate) < wz[0]:
        return f"--waypoint_turn_rate {float(turn_rate)} is beyond the env's command range for wz, {wz[0]} .. {wz[1]} rad/s"
    return None


def waypoints_from_args(args) -> Optional[Dict]:
    """The waypoint follower the command line asks for -- `courses` (one per `--waypoints`), `radius`, `speed`, `turn_rate`, `gain`,
    `slow_dist` and the `flags` as given -- or None without `--waypoints`.  SystemExit with the reason for a course that cannot be parsed, a
    setting that is not a finite number >= 0 (gain and slow-down distance: > 0), and for `--waypoints` next to `--sequence` / `--then` (two
    writers of the command buffer), `--command` / `--grid` (the course is the command), pushes and `--posture` (one command per episode)
    -- host work only, before any batch exists."""
    texts = getattr(args, "waypoints", None) or []
    if not texts:
        return None
    if getattr(args, "sequence", None) or getattr(args, "then", None):
        raise SystemExit("--waypoints does not combine with --sequence / --then: the follower and the schedule would both write the command buffer")
    if getattr(args, "command", None) or getattr(args, "grid", None):
        raise SystemExit("--waypoints does not combine with --command / --grid: the course is the command (every --waypoints is one row of the report)")
    if getattr(args, "push", None) or getattr(args, "push_grid", None):
        raise SystemExit("--waypoints does not combine with --push / --push_grid: the push figures assume one command per episode")
    if getattr(args, "posture", False):
        raise SystemExit("--waypoints does not combine with --posture: its settle times assume one command per episode")
    try:
        courses = [parse_waypoints(t) for t in texts]
    except ValueError as err:
        raise SystemExit(str(err))
    out = dict(courses=courses, flags=dict(waypoints=list(texts)))
    for key, flag, default, positive in (("radius", "waypoint_radius", DEFAULT_WAYPOINT_RADIUS, False), ("speed", "waypoint_speed", DEFAULT_WAYPOINT_SPEED, False),
                                         ("turn_rate", "waypoint_turn_rate", DEFAULT_WAYPOINT_TURN_RATE, False),
                                         ("gain", "waypoint_gain", DEFAULT_WAYPOINT_GAIN, True), ("slow_dist", "waypoint_slow_dist", DEFAULT_WAYPOINT_SLOW_DIST, True)):
        v = float(getattr(args, flag, default))
        if not np.isfinite(v) or v < 0 or (positive and v == 0):
            raise SystemExit(f"--{flag} is a finite number {'> 0' if positive else '>= 0'}, got {v}")
        out[key] = v
    return out


def ideal_pose(command: Sequence[float], t) -> tuple:
    """(x, y, psi) after holding the body-frame velocities `command[:3]` = (vx, vy, wz) for `t` seconds from the pose (0, 0, 0), in float64:
    the arc x = (vx sin a - vy (1 - cos a)) / wz, y = (vx (1 - cos a) + vy sin a) / wz with a = wz t, written with sin(a) / a and
    (1 - cos a) / a = sin(a / 2) * sin(a / 2) / (a / 2) so that wz -> 0 is the line (vx t, vy t) without a cancellation or a branch."""
    vx, vy, wz = (float(x) for x in list(command)[:3])
    t = np.asarray(t, np.float64)
    a = wz * t
    s = t * np.sinc(a / np.pi)                                 # sin(a) / wz
    c = t * np.sin(0.5 * a) * np.sinc(0.5 * a / np.pi)         # (1 - cos a) / wz
    return vx * s - vy * c, vx * c + vy * s, a


def _mean_std(x: np.ndarray) -> Dict:
    x = np.asarray(x, np.float64)
    return dict(mean=float(x.mean()) if x.size else None, std=float(x.std()) if x.size else None)


def path_frame(acc: np.ndarray) -> tuple:
    """(forward, lateral) [nenv] float64: the start-frame displacement of every env at its last sample, from a path accumulator."""
    a = np.asarray(acc, np.float64).reshape(-1, PATH_NACC)
    rx, ry = a[:, W_X] - a[:, W_START_X], a[:, W_Y] - a[:, W_START_Y]
    hx, hy = a[:, W_START_HX], a[:, W_START_HY]
    return rx * hx + ry * hy, hx * ry - hy * rx


def reduce_path(acc: np.ndarray, commands: Sequence, envs_per_block: int, dt: float, constant: bool = True) -> List[Dict]:
    """One "path" object per block of `envs_per_block` envs (a block per entry of `commands`), from the path accumulator ([nenv, 32],
    include/odk.h ODK_PATH_*), in float64.  Per env, then {mean, std} over the block: `forward_m` and `lateral_m`, the displacement at the
    env's last sample in its start frame; `heading_change_rad` (TURN: the sum of the sines of the per-step heading changes, within 1e-4
    relative of the heading change at 50 Hz and |wz| <= 1 rad/s); `path_length_m`; `straightness`, displacement over length, over the envs
    that covered at least MIN_COT_DISTANCE (None when nobody did).  `samples`: the block's samples.  `constant`: every env of a block held
    the block's one command throughout; then `ideal` is the block's mean dead-reckoned pose (`ideal_pose` over each env's own SAMPLES * dt)
    and `error_vs_ideal_m` the mean distance from the env's displacement to its own ideal one; both None otherwise (schedules, courses)."""
    a = np.asarray(acc, np.float64).reshape(-1, PATH_NACC)
    fwd_all, lat_all = path_frame(a)
    E, dt = int(envs_per_block), float(dt)
    out = []
    for c, cmd in enumerate(commands):
        sl = slice(c * E, (c + 1) * E)
        blk, fwd, lat = a[sl], fwd_all[sl], lat_all[sl]
        length = blk[:, W_LENGTH]
        moved = length >= MIN_COT_DISTANCE
        g = dict(samples=int(round(float(blk[:, W_SAMPLES].sum()))), forward_m=_mean_std(fwd), lateral_m=_mean_std(lat),
                 heading_change_rad=_mean_std(blk[:, W_TURN]), path_length_m=_mean_std(length),
                 straightness=_mean_std(np.hypot(fwd[moved], lat[moved]) / length[moved]) if moved.any() else None, ideal=None, error_vs_ideal_m=None)
        if constant:
            ix, iy, ipsi = ideal_pose(cmd, blk[:, W_SAMPLES] * dt)
            g["ideal"] = dict(forward_m=float(ix.mean()), lateral_m=float(iy.mean()), heading_change_rad=float(ipsi.mean()))
            g["error_vs_ideal_m"] = float(np.hypot(fwd - ix, lat - iy).mean())
        out.append(g)
    return out


def reduce_course(acc: np.ndarray, courses: Sequence[Sequence[Sequence[float]]], envs_per_block: int, dt: float) -> List[Dict]:
    """One "course" object per block of `envs_per_block` envs (a block per entry of `courses`: the block's points), from the path
    accumulator, in float64.  `points`; `completed_fraction`, the share of the envs that reached every waypoint; `waypoints`: per waypoint
    its `point`, `reached_fraction` and `time_to_reach_s`, the median over the envs that reached it of the step at which they did, times
    dt (None when nobody did); `cross_track_rms_m` / `cross_track_peak_m`, over the block's samples with a waypoint still ahead, the RMS
    and the maximum of the distance to the leg being walked (None without such a sample); `final_goal_distance_m`, the mean over the
    envs with such a sample of the distance to the last waypoint at the latest of them (a completer's: where it was when it reached the
    goal); `length_ratio`, the mean over the completers of path length over the course's polyline length from the origin (None without a
    completer or for a course of zero length); `falls_by_leg`: entry i counts the envs that fell heading for waypoint i, the last entry
    those that fell after the course was finished."""
    a = np.asarray(acc, np.float64).reshape(-1, PATH_NACC)
    E, dt = int(envs_per_block), float(dt)
    out = []
    for c, pts in enumerate(courses):
        blk, n = a[c * E:(c + 1) * E], len(pts)
        done = blk[:, W_WP_INDEX] >= n
        steps = blk[:, W_REACHED:W_REACHED + n]
        wps = []
        for i, p in enumerate(pts):
            hit = steps[:, i] > 0
            wps.append(dict(point=[float(x) for x in p], reached_fraction=float(hit.sum() / E),
                            time_to_reach_s=float(np.median(steps[hit, i]) * dt) if hit.any() else None))
        xn = blk[:, W_XTRACK_SAMPLES]
        seen, total = xn > 0, float(xn.sum())
        fell = blk[:, W_FELL] != 0
        legs = np.clip(blk[fell, W_FELL_LEG].astype(np.int64), 0, n)
        poly = course_length(pts)
        out.append(dict(
            points=[[float(x) for x in p] for p in pts], completed_fraction=float(done.sum() / E), waypoints=wps,
            cross_track_rms_m=float(np.sqrt(blk[:, W_XTRACK_SQ].sum() / total)) if total > 0 else None,
            cross_track_peak_m=float(blk[seen, W_XTRACK_PEAK].max()) if seen.any() else None,
            final_goal_distance_m=_mean_or_none(blk[seen, W_GOAL_DIST]),
            length_ratio=float((blk[done, W_LENGTH] / poly).mean()) if done.any() and poly > 0 else None,
            falls_by_leg=[int((legs == i).sum()) for i in range(n + 1)]))
    return out


PATH_KEYS = ("samples", "forward_m", "lateral_m", "heading_change_rad", "path_length_m", "straightness", "ideal", "error_vs_ideal_m")
COURSE_KEYS = ("points", "completed_fraction", "waypoints", "cross_track_rms_m", "cross_track_peak_m", "final_goal_distance_m", "length_ratio",
               "falls_by_leg")
COURSE_POINT_KEYS = ("point", "reached_fraction", "time_to_reach_s")


def reduce_tracking(acc: np.ndarray, commands: Sequence[Sequence[float]], envs_per_command: int) -> List[Dict]:
    """The per-command rows of the report from the accumulator ([nenv, 12], include/odk.h ODK_TRACK_*).  Velocity statistics are over
    the velocity samples of the block's envs (the steps of their first episode that did not end it), pooled; the fall rate is the
    share of the block's envs whose first episode ended by falling; the episode reward is the mean over envs of their first episode's
    reward sum.  Under a command schedule the block is a schedule's, `commands` holds segment 0's commands, and the errors are against the
    command in force at each step (the accumulator reads the bound row as the step read it)."""
    acc = np.asarray(acc, np.float64).reshape(-1, NACC)
    E = int(envs_per_command)
    rows = []
    for c, cmd in enumerate(commands):
        blk = acc[c * E:(c + 1) * E]
        samples = float(blk[:, SAMPLES].sum())
        den = max(samples, 1.0)
        mean = blk[:, SUM:SUM + 3].sum(0) / den
        rms = np.sqrt(blk[:, SQERR:SQERR + 3].sum(0) / den)
        rows.append(dict(
            command=[float(x) for x in cmd],
            mean_vx=float(mean[0]), mean_vy=float(mean[1]), mean_wz=float(mean[2]),
            rms_error_vx=float(rms[0]), rms_error_vy=float(rms[1]), rms_error_wz=float(rms[2]),
            fall_rate=float(blk[:, FALLS].sum() / E),
            mean_episode_reward=float(blk[:, REWARD].mean()),
            mean_episode_steps=float(blk[:, STEPS].mean()),
            steps=int(round(float(blk[:, STEPS].sum()))),
            velocity_samples=int(round(samples)),
            envs=E,
        ))
    return rows


REPORT_KEYS = ("settings", "commands")
ROW_KEYS = ("command", "mean_vx", "mean_vy", "mean_wz", "rms_error_vx", "rms_error_vy", "rms_error_wz", "fall_rate", "mean_episode_reward",
            "mean_episode_steps", "steps", "velocity_samples", "envs")


def make_report(settings: Dict, rows: List[Dict]) -> Dict:
    return {"settings": dict(settings), "commands": list(rows)}


def save_obs(path: str, obs: np.ndarray) -> None:
    """mujoco_infer.py's mujoco_saved_obs.pkl format: a pickled list of one 1-D numpy array per step (plot_saved_obs.py reads it)."""
    with open(path, "wb") as f:
        pickle.dump([np.array(o, np.float32) for o in obs], f)


def config_overrides(args) -> Dict:
    """The env's config_overrides from the command line."""
    from .runner import head_joint_overrides, imitation_overrides
    overrides = {"episode_length": int(args.episode_length)}
    if args.hfield_up_normals_only:
        overrides["hfield_up_normals_only"] = True
    if args.cone:
        overrides["cone"] = args.cone
    overrides.update(imitation_overrides(args))
    overrides.update(head_joint_overrides(args))
    if getattr(args, "noise_level", None) is not None:
        overrides["noise_config.level"] = float(args.noise_level)
    return overrides


def make_env(args, num_envs: int, device: int):
    from . import joystick, standing
    envs = {"joystick": joystick.Joystick, "standing": standing.Standing}     # runner.py's --env
    if args.env not in envs:
        raise ValueError(f"Unknown env {args.env}")
    overrides = config_overrides(args)
    extra = {"xml_path": args.xml} if args.xml else {}
    # a few hundred envs: one env per wave finishes a step sooner (Joystick.make_eval_env)
    return envs[args.env](task=args.task, num_envs=num_envs, device=device, autoreset=True, lanes_per_env=64 if num_envs <= 1024 else 0,
                          config_overrides=overrides, **extra)


def load_networks(path: Optional[str], env, device):
    import torch
    from .ppo.networks import PPONetworks
    from .ppo.train import ppo_config
    nf = ppo_config()["network_factory"]
    net = PPONetworks(env.observation_size["state"][0], env.observation_size["privileged_state"][0], env.action_size,
                      nf["policy_hidden_layer_sizes"], nf["value_hidden_layer_sizes"]).to(device)
    net.load_state_dict(torch.load(path, map_location=device)["networks"])      # ppo/train.py save_checkpoint (a `fault_spec` beside it is not read here)
    net.eval()
    return net


def trained_under(path: Optional[str]):
    """The faults a checkpoint was trained under (runner --train_sensor / --train_actuation: ppo/train.py save_checkpoint's `fault_spec`),
    None for one trained on the nominal robot and for every file from before the key."""
    from .ppo.train import checkpoint_fault_spec
    return checkpoint_fault_spec(path)


def trained_with_curriculum(path: Optional[str]):
    """The command curriculum a checkpoint was trained with (runner --command_curriculum: ppo/train.py save_checkpoint's
    `command_curriculum`), None for every other checkpoint."""
    if not path:
        return None
    from .ppo.train import checkpoint_command_curriculum
    return checkpoint_command_curriculum(path)


@dataclasses.dataclass
class Report:
    """One report of a Tracker.  `acc`: its zeroed accumulator ([num_envs, ncol] on the env's device); `launch(batch, track_acc)`: after the
    step, before the tracking accumulator sets ENDED; `shown`: the accumulator and the device-side extras, by the Tracker attribute that shows
    them.  For `run`: `reduce(acc_numpy, commands, envs_per_block)` gives one value per block of envs (`commands`: the blocks' commands), which
    `put(block, value)` sets on its row or cell (default: under `key`), and `settings` are its entries of the report's.  `drives`: it sets what
    the episode is given (pushes, commands), so its entries lead.  `report_rows` reduces every report per row and once more per cell of the
    `CellAxis`, but the one whose row entries ARE the cells (key "pushes")."""
    key: str
    acc: object
    launch: Callable
    shown: Dict
    reduce: Optional[Callable] = None
    settings: Dict = dataclasses.field(default_factory=dict)
    put: Optional[Callable] = None
    zero: Optional[Callable] = None      # default: acc.zero_
    drives: bool = False
    before_reset: Callable = lambda batch, track_acc: None
    before_step: Callable = lambda batch, track_acc: None


def _zeros(env, ncol: int):
    return env.batch.torch.zeros(env.num_envs, ncol, device=env.batch.obs.device)


def _device_torque_limits(env):
    return env.batch.torch.from_numpy(torque_limits(env.mj_model)).to(env.batch.obs.device)


def push_report(env, kicks, push_at: int, tolerance, entries: Sequence[Dict] = (), envs_per_cell: int = 0, flags: Optional[Dict] = None) -> Report:
    """`kicks` ([num_envs, 2], one world-frame kick per env): a bound push buffer that holds env e's kick during the step at which the device
    step counter -- the first-episode step, since first episodes start together at `reset` -- equals `push_at`, and zeros otherwise.
    For `run`: `entries`, the pushes of a command's cells, `envs_per_cell` envs each, and its `flags`."""
    torch, acc = env.batch.torch, _zeros(env, PUSH_NACC)
    kicks = kicks.to(device=acc.device, dtype=torch.float32).reshape(env.num_envs, 2).contiguous()
    push_at, tol = int(push_at), (float(tolerance[0]), float(tolerance[1]))
    buf, counter = torch.zeros_like(kicks), torch.full((), -1, dtype=torch.int64, device=acc.device)
    env.set_pushes(buf)

    def before_step(batch, track_acc):      # device ops only: the same graph replay serves every step
        counter.add_(1)
        torch.mul(kicks, (counter == push_at).to(kicks.dtype), out=buf)
    return Report("pushes", acc, lambda b, t: b.push_accumulate(acc, t, *tol), dict(push_acc=acc, push_buf=buf, kicks=kicks, counter=counter),
                  reduce=lambda a, cmds, _: reduce_pushes(a, cmds, entries, envs_per_cell, float(env.dt)),      # (a row's block is its cells)
                  settings=dict(flags or {}, push_at=push_at, push_tolerance=list(tol), pushes_per_command=len(entries)),
                  put=lambda row, extra: row.update(extra), zero=lambda: (acc.zero_(), buf.zero_(), counter.fill_(-1)), drives=True,
                  before_step=before_step)


def gait_report(env) -> Report:
    acc, limit = _zeros(env, GAIT_NACC), _device_torque_limits(env)
    return Report("gait", acc, lambda b, t: b.gait_accumulate(acc, t, limit), dict(gait_acc=acc, torque_limit=limit),
                  reduce=lambda a, cmds, E: reduce_gait(a, cmds, E, float(env.dt), env.mj_model), settings=dict(gait=True))


def posture_report(env, tolerance: float, head=None) -> Report:
    """`tolerance`: the head error in radians; `head`: (head_map, joint_names) of `posture_head_map`, for `run`."""
    acc, tol = _zeros(env, POSTURE_NACC), float(tolerance)
    return Report("posture", acc, lambda b, t: b.posture_accumulate(acc, t, tol), dict(posture_acc=acc),
                  reduce=lambda a, cmds, E: reduce_posture(a, cmds, E, float(env.dt), *head), settings=dict(posture=True, posture_tolerance=tol))


def imitation_report(env, info=None) -> Report:
    """`info`: (imap, joint_names, period_steps), `imitation_joint_info(env)` unless given."""
    acc = _zeros(env, IMIT_NACC)
    imap, names, period = info if info is not None else imitation_joint_info(env)
    return Report("imitation", acc, lambda b, t: b.imitation_accumulate(acc, t, period), dict(imitation_acc=acc, period_steps=period),
                  reduce=lambda a, cmds, E: reduce_imitation(a, cmds, E, float(env.dt), imap, names, period),
                  settings=dict(imitation_report=True, imitation_period_steps=period))


def response_report(env, schedule: Dict) -> Report:
    """`schedule`: a dict of `table` (`schedule_table`), `map` (`schedule_blocks`), `tolerance` (lin, ang), `tail_after`, and for `run` the
    `schedules` and its `flags`.  `odk_command_schedule_apply` writes the bound command tensor before the env's reset and before every step."""
    torch, acc = env.batch.torch, _zeros(env, RESP_NACC)
    table = torch.as_tensor(np.ascontiguousarray(schedule["table"], np.float32)).to(acc.device).contiguous()
    smap = torch.as_tensor(np.ascontiguousarray(schedule["map"], np.int32)).to(acc.device).contiguous()
    tol = tuple(float(x) for x in schedule.get("tolerance", DEFAULT_PUSH_TOLERANCE))
    tail_after, schedules = int(schedule.get("tail_after", DEFAULT_RESPONSE_TAIL_AFTER)), schedule.get("schedules") or ()

    def before_reset(batch, track_acc):      # the reset must find segment 0's command: a zeroed clock, one apply launch, then the env
        track_acc.zero_()
        acc.zero_()
        batch.command_schedule_apply(table, smap, track_acc)

    def reduce(a, cmds, E):      # the blocks: every schedule's, or each schedule's cells (as many blocks per schedule as `cmds` has per schedule)
        scheds = [s for s in schedules for _ in range(len(cmds) // len(schedules))]
        return list(zip(scheds, reduce_response(a, scheds, E, float(env.dt))))

    def put(block, value):
        block["schedule"] = [dict(start_step=int(seg["start_step"]), command=[float(x) for x in seg["command"]]) for seg in value[0]]
        block["segments"] = value[1]
    return Report("segments", acc, lambda b, t: b.response_accumulate(acc, t, table, smap, *tol, tail_after),
                  dict(response_acc=acc, sched=table, sched_map=smap), reduce=reduce, put=put, drives=True, before_reset=before_reset,
                  settings=dict(schedule.get("flags") or {}, response_tolerance=list(tol), response_tail_after=tail_after, schedules=len(schedules)),
                  before_step=lambda b, t: b.command_schedule_apply(table, smap, t))      # the command of the step about to run; the clock is STEPS


def fall_report(env, falls: Dict) -> Report:
    """`falls`: a dict of `ring` (samples) and `tilt_tol` (the sine of the upright lean), and for `run`'s settings the flags `tilt`, `save`,
    `save_max` as given.  The recorder is [num_envs, fall_row_floats(ring)]."""
    ring, tilt_tol, nq = int(falls["ring"]), float(falls["tilt_tol"]), int(env.batch.model.nq)
    acc, limit = _zeros(env, env.batch.fall_row_floats(ring)), _device_torque_limits(env)
    return Report("falls", acc, lambda b, t: b.fall_accumulate(acc, t, tilt_tol, ring, limit), dict(fall_acc=acc, torque_limit=limit),
                  reduce=lambda a, cmds, E: reduce_falls(a, cmds, E, float(env.dt), ring, nq),
                  settings=dict(falls=True, fall_ring=ring, fall_tilt=falls.get("tilt"), fall_tilt_tol=tilt_tol, save_falls=falls.get("save"),
                                save_falls_max=falls.get("save_max")))


def path_report(env, constant: bool = True) -> Report:
    """The odometry of every env in its start frame (`odk_path_begin` after the reset, `odk_path_accumulate` every step).  `constant`, for
    `run`: every block holds one command throughout, so its "path" object carries the dead-reckoned `ideal`."""
    acc = _zeros(env, PATH_NACC)
    return Report("path", acc, lambda b, t: b.path_accumulate(acc, t), dict(path_acc=acc), zero=lambda: env.batch.path_begin(acc),
                  reduce=lambda a, cmds, E: reduce_path(a, cmds, E, float(env.dt), constant), settings=dict(path=True))


def waypoint_report(env, course: Dict) -> Report:
    """`course`: a dict of `table` (`course_table`), `map` (`schedule_blocks`: env e's course), `radius`, `speed`, `turn_rate`, `gain`,
    `slow_dist` (defaults: DEFAULT_WAYPOINT_*), and for `run` the `courses` and its `flags`.  `odk_waypoint_command_apply` writes entries
    0..2 of the bound command tensor before the env's reset (a zeroed clock: the start pose) and before every step; the path accumulator
    also follows the course."""
    torch, acc = env.batch.torch, _zeros(env, PATH_NACC)
    table = torch.as_tensor(np.ascontiguousarray(course["table"], np.float32)).to(acc.device).contiguous()
    cmap = torch.as_tensor(np.ascontiguousarray(course["map"], np.int32)).to(acc.device).contiguous()
    radius = float(course.get("radius", DEFAULT_WAYPOINT_RADIUS))
    drive = (float(course.get("speed", DEFAULT_WAYPOINT_SPEED)), float(course.get("turn_rate", DEFAULT_WAYPOINT_TURN_RATE)),
             float(course.get("gain", DEFAULT_WAYPOINT_GAIN)), float(course.get("slow_dist", DEFAULT_WAYPOINT_SLOW_DIST)))
    courses = course.get("courses") or ()

    def before_reset(batch, track_acc):      # the reset must find the first command: a zeroed clock, one apply launch, then the env
        track_acc.zero_()
        batch.waypoint_command_apply(table, cmap, track_acc, acc, *drive)

    def reduce(a, cmds, E):      # the blocks: every course's, or each course's cells (as many blocks per course as `cmds` has per course)
        cs = [c for c in courses for _ in range(len(cmds) // len(courses))]
        return list(zip(reduce_path(a, cmds, E, float(env.dt), False), reduce_course(a, cs, E, float(env.dt))))

    def put(block, value):
        block["path"], block["course"] = value
    return Report("path", acc, lambda b, t: b.path_accumulate(acc, t, table, cmap, radius), dict(path_acc=acc, course=table, course_map=cmap),
                  reduce=reduce, put=put, zero=lambda: env.batch.path_begin(acc), drives=True, before_reset=before_reset,
                  before_step=lambda b, t: b.waypoint_command_apply(table, cmap, t, acc, *drive),
                  settings=dict(course.get("flags") or {}, path=True, waypoint_radius=radius, waypoint_speed=drive[0], waypoint_turn_rate=drive[1],
                                waypoint_gain=drive[2], waypoint_slow_dist=drive[3], courses=len(courses)))


class Tracker:
    """One tracking run on a bound command buffer: `step()` = policy + env step + the reports' accumulators + the tracking accumulator,
    captured as one graph.  `reports`: the `Report`s the step carries, in launch order; or (never both) the switches that make them in this
    order -- `kicks` with `push_at` / `push_tolerance`, `gait`, `posture` with `posture_tolerance`, `imitation`, `schedule` (the bound command
    tensor is then written by the Tracker), `falls`, `path` or (never both) `waypoints` (`waypoint_report`'s dict: the follower writes the
    bound command tensor).  A report's accumulator and device buffers are also the Tracker's attributes (below),
    None without the report.  `delays` ([num_envs] device int32, one action delay per env: 0, 1, 2, or -1 for the sampled one) are bound
    (`set_action_delays`) and kept; the step itself is unchanged.  Model parameters (`Batch.set_param`) are the caller's to set before `reset`.
    `sensors`: dict(fault=<[num_envs, SENSOR_NPRM] float32, a fault row per env: `Batch.sensor_fault_rows`, `sensors.fault_row`>): the step
    begins with `odk_sensor_apply` from the env's observation into `sensor_obs`, which the policy reads instead; `sensor_fault` (the caller's
    own tensor when it is float32 on the env's device: writing it between steps is followed by the captured graph) and `sensor_state` (the
    sample ring, zeroed by `reset`) are kept.  Without `sensors` the three are None and the launch sequence is the plain one.
    `actuation`: dict(fault=<[num_envs, ACT_NPRM] float32, a fault row per env: `Batch.action_fault_rows`, `actuation.fault_row`>): after the
    policy and the reports' `before_step`, `odk_action_apply` turns the policy's action into `actuation_act`, the action each env's link
    delivers, and the env step takes that tensor; `actuation_fault` (kept as `sensor_fault` is) and `actuation_state` (the stage's
    counters, filter state and last delivered action, zeroed by `reset`) are kept.  Without `actuation` the three are None and the
    launch sequence is the plain one."""
    def _shown(name):      # what the first report that has `name` in its `shown` holds there
        return property(lambda self: next((r.shown[name] for r in self.reports if name in r.shown), None))
    push_acc, push_buf, kicks, counter = _shown("push_acc"), _shown("push_buf"), _shown("kicks"), _shown("counter")
    gait_acc, posture_acc, imitation_acc, period_steps = _shown("gait_acc"), _shown("posture_acc"), _shown("imitation_acc"), _shown("period_steps")
    response_acc, sched, sched_map, fall_acc, torque_limit = _shown("response_acc"), _shown("sched"), _shown("sched_map"), _shown("fall_acc"), _shown("torque_limit")
    path_acc, course, course_map = _shown("path_acc"), _shown("course"), _shown("course_map")

    def __init__(self, env, net, use_graph: bool = True, kicks=None, push_at: int = DEFAULT_PUSH_AT, push_tolerance=DEFAULT_PUSH_TOLERANCE,
                 gait: bool = False, posture: bool = False, posture_tolerance: float = DEFAULT_POSTURE_TOLERANCE,
                 imitation: bool = False, schedule: Optional[Dict] = None, falls: Optional[Dict] = None, delays=None, reports=None, path: bool = False,
                 waypoints: Optional[Dict] = None, sensors: Optional[Dict] = None, actuation: Optional[Dict] = None):
        import torch
        self.env, self.net, self.torch = env, net, torch
        self.acc = torch.zeros(env.num_envs, NACC, device=env.batch.obs.device)
        self.sensor_fault = self.sensor_state = self.sensor_obs = None
        if sensors is not None:      # (a float32 tensor already on the device is kept as it is: the caller's later writes reach the step)
            self.sensor_fault = torch.as_tensor(sensors["fault"]).to(device=self.acc.device, dtype=torch.float32).reshape(env.num_envs, SENSOR_NPRM).contiguous()
            self.sensor_state = torch.zeros(env.num_envs, SENSOR_NSTATE, device=self.acc.device)
            self.sensor_obs = torch.zeros_like(env.batch.obs)
        self.actuation_fault = self.actuation_state = self.actuation_act = None
        if actuation is not None:      # (as the sensors' three)
            self.actuation_fault = torch.as_tensor(actuation["fault"]).to(device=self.acc.device, dtype=torch.float32).reshape(env.num_envs, ACT_NPRM).contiguous()
            self.actuation_state = torch.zeros(env.num_envs, ACT_NSTATE, device=self.acc.device)
            self.actuation_act = torch.zeros(env.num_envs, int(env.batch.model.nu), device=self.acc.device)
        if reports is not None and (kicks is not None or gait or posture or imitation or schedule is not None or falls is not None or path
                                    or waypoints is not None):
            raise ValueError("Tracker: give the reports or the switches that make them, not both")
        if path and waypoints is not None:
            raise ValueError("Tracker: `waypoints` carries the path report: give one of `path` and `waypoints`")
        if reports is None:
            reports = [make() for on, make in (
                (kicks is not None, lambda: push_report(env, kicks, push_at, push_tolerance)), (gait, lambda: gait_report(env)),
                (posture, lambda: posture_report(env, posture_tolerance)), (imitation, lambda: imitation_report(env)),
                (schedule is not None, lambda: response_report(env, schedule)), (falls is not None, lambda: fall_report(env, falls)),
                (path, lambda: path_report(env)), (waypoints is not None, lambda: waypoint_report(env, waypoints))) if on]
        self.reports = list(reports)
        self.delays = None
        if delays is not None:
            self.delays = delays.to(device=self.acc.device, dtype=torch.int32).reshape(env.num_envs).contiguous()
            env.set_action_delays(self.delays)
        from .ppo.learner import fused_policy
        self.fp = fused_policy(net, env.num_envs)
        self.use_graph, self.graph = use_graph, None

    def actions(self, obs):
        """The deterministic policy: tanh(loc) of the policy head (Evaluator._one_step)."""
        logits = self.fp(obs) if self.fp is not None else self.net.policy(self.net.norm_obs(obs))
        return self.torch.tanh(logits[..., : self.net.action_size]).contiguous()

    def _one_step(self):
        b = self.env.batch
        obs = b.obs
        if self.sensor_fault is not None:      # what the faulty sensors deliver of the row the step wrote; the row itself is only read
            b.sensor_apply(b.obs, b.done, self.sensor_fault, self.sensor_state, self.sensor_obs)
            obs = self.sensor_obs
        act = self.actions(obs)
        for r in self.reports:
            r.before_step(b, self.acc)
        if self.actuation_fault is not None:      # what the link delivers of the action the policy asked for; that action is only read
            b.action_apply(act, b.done, self.actuation_fault, self.actuation_state, self.actuation_act)
            act = self.actuation_act
        b.step(act)                                 # Joystick.step without the State wrapper (nothing here reads it)
        for r in self.reports:
            r.launch(b, self.acc)                   # before the tracking accumulator sets ENDED
        b.tracking_accumulate(self.acc)

    def reset(self, seed: int):
        for r in self.reports:
            r.before_reset(self.env.batch, self.acc)
        self.env.reset(int(seed))
        self.acc.zero_()
        for r in self.reports:
            (r.zero or r.acc.zero_)()
        if self.sensor_state is not None:
            self.sensor_state.zero_()               # an empty ring: the first call fills it with the reset's observation
        if self.actuation_state is not None:
            self.actuation_state.zero_()            # step 0 of episode 1: the filter and the last delivered action start from action 0
        if self.fp is not None:
            self.fp.refresh()                       # its packed weight copy <- the current parameters

    def step(self):
        torch = self.torch
        if not (self.use_graph and self.env.batch.obs.is_cuda):
            self._one_step()
            return
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._one_step()                    # warm-up: this IS the first step
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._one_step()                    # captured, not executed
            return
        self.graph.replay()


@dataclasses.dataclass
class CellAxis:
    """What divides a command's envs into cells of `--envs_per_command` envs: the pushes, the plants, the sensor or the actuation settings (they exclude
    each other).  `row_key`: where a row holds its cells; `cells`: a dict per cell, in the layout's order.  `label_key`: a cell is a whole
    command row of its own and holds its dict of `cells` there; None for the pushes, whose cells are their `Report`'s.  `robustness_key`:
    where a row holds `reduce_robustness` of its cells at `threshold`, with `nominals` and `order`; None for none.  `settings`: the axis'
    entries of the report's."""
    row_key: str
    cells: Sequence[Dict]
    label_key: Optional[str] = None
    robustness_key: Optional[str] = None
    threshold: float = DEFAULT_ROBUST_FALL_RATE
    nominals: Optional[Dict] = None
    order: Optional[Callable] = None
    settings: Dict = dataclasses.field(default_factory=dict)


def cell_axis(args, pushes: Sequence[Dict], plants: Sequence[Dict], sensors: Sequence[Dict], actuations: Sequence[Dict] = ()) -> Optional[CellAxis]:
    """The cell axis of a run from what its flags gave (at most one of the four is not empty: the `*_from_args` refusals), None without."""
    robust = float(getattr(args, "robust_fall_rate", DEFAULT_ROBUST_FALL_RATE))
    if pushes:
        return CellAxis("pushes", pushes)      # (its settings are the push report's)
    if plants:
        return CellAxis("plants", plants, "plant", "robustness", robust, settings=dict(
            plant=getattr(args, "plant", None), plant_grid=getattr(args, "plant_grid", None), plants_per_command=len(plants), robust_fall_rate=robust,
            plant_semantics="kp, mass, frictionloss, armature: scales on the model's values (kp: every actuator's gain, the bias "
                            "following; mass: every body's mass, inertias NOT rescaled, as the reference's randomize.py; frictionloss, "
                            "armature: the actuated dofs'); delay: action delay in control steps, 0 1 2 or random (the sampler); "
                            "--gait's cost_of_transport keeps the model's nominal mass"))
    if sensors:
        return CellAxis("sensors", sensors, "sensor", "sensor_robustness", robust, nominal_sensor(), sensor_order, settings=dict(
            sensor=getattr(args, "sensor", None), sensor_grid=getattr(args, "sensor_grid", None), sensors_per_command=len(sensors), robust_fall_rate=robust,
            sensor_semantics="what the policy reads, not what the robot does: every report reads the noise-free privileged row.  "
                             "gyro / acc: out = scale * (R x) + bias, R the mounting rotation of imu_roll / pitch / yaw (degrees), "
                             "biases in rad/s and m/s^2; imu_delay / joint_delay: whole control steps, a ring of raw samples that a "
                             "new episode fills with its first observation; encoder_offset: every env draws each actuator's zero "
                             "error uniformly in +-X rad (seeded by --seed), encoder_quant: the position step in rad, after the "
                             "offset; contact_left / contact_right: ok, off (stuck at 0) or on (stuck at 1); the env's own noise is "
                             "in the row before the fault"))
    if actuations:
        return CellAxis("actuations", actuations, "actuation", "actuation_robustness", robust, nominal_actuation(), actuation_order, settings=dict(
            actuation=getattr(args, "actuation", None), actuation_grid=getattr(args, "actuation_grid", None), actuations_per_command=len(actuations),
            robust_fall_rate=robust,
            actuation_semantics="what the servos receive, not what the policy asked for: the env step, its three action memories and "
                                "motor_targets in the observation take the delivered action (the reference's deployment order: the "
                                "filter runs before last_action is taken).  Stages in order: gain; offset (every env draws each "
                                "actuator's horn error uniformly in +-X rad, seeded by --seed); noise (uniform, +-X action units); limit "
                                "(clamp, action units); cutoff (the reference's LowPassActionFilter, Hz); quant (the target's step in "
                                "rad); drop / drop_len (a step's packet is lost with probability drop, then drop_len steps in a row "
                                "deliver the last delivered action); freeze / freeze_at (from that episode step on the named actuator "
                                "keeps its last delivered action).  A new episode starts filter and last delivered action at action "
                                "0, the default pose.  \"link\": dropped_share = lost packets / calls over the cell's envs"))
    return None


def block_commands(rows: Sequence[Dict], axis: Optional[CellAxis]) -> List[List[float]]:
    """The command of every block of `envs_per_cell` envs, in env order: each row's, once per cell of the axis."""
    return [row["command"] for row in rows for _ in (axis.cells if axis else [0])]


def report_rows(acc: np.ndarray, reports: Sequence[tuple], commands: Sequence[Sequence[float]], axis: Optional[CellAxis], envs_per_cell: int) -> List[Dict]:
    """The rows of the report, host arithmetic only.  `acc`: the tracking accumulator; `reports`: (`Report`, its accumulator as numpy) pairs
    in the report's order, of which `key`, `reduce` and `put` are read; `commands`: one per row; `axis`: the cell axis or None.  A row is
    `reduce_tracking` over its command's envs; with a labelled axis (plants, sensors) it then holds, under the axis' `row_key`, one whole
    command row per cell of `envs_per_cell` envs (`sweeps.cell_rows`' order) with the cell's dict under `label_key`.  Every report then puts
    its object on every row and, but the one whose row entries ARE the cells (pushes), on every cell; the robustness object comes last,
    for its lines read the cells' own figures."""
    E, P = int(envs_per_cell), len(axis.cells) if axis else 1
    rows = reduce_tracking(acc, commands, P * E)
    if axis and axis.label_key:
        cells = reduce_tracking(acc, block_commands(rows, axis), E)
        for i, cell in enumerate(cells):
            cell[axis.label_key] = dict(axis.cells[i % P])
        for c, row in enumerate(rows):
            row[axis.row_key] = cells[c * P:(c + 1) * P]
    for r, a in reports:
        put = r.put or (lambda block, value, key=r.key: block.__setitem__(key, value))
        for row, value in zip(rows, r.reduce(a, commands, P * E)):
            put(row, value)
        if axis and r.key != axis.row_key:
            cells = [cell for row in rows for cell in row[axis.row_key]]
            for cell, value in zip(cells, r.reduce(a, block_commands(rows, axis), E)):
                put(cell, value)
    if axis and axis.robustness_key:
        for row in rows:
            row[axis.robustness_key] = reduce_robustness(row[axis.row_key], axis.threshold, axis.label_key, axis.nominals, axis.order)
    return rows


def run(args, out=sys.stdout) -> Dict:
    import torch
    way = waypoints_from_args(args)            # None without --waypoints; refusals before any batch work
    schedules = schedules_from_args(args)      # None without --sequence / --then; refusals before any batch work
    if way is not None:
        commands = [[0.0] * 7 for _ in way["courses"]]      # a course row's `command`: the follower writes vx, vy, wz, the head entries stay 0
    elif schedules is not None:
        commands = [list(s[0]["command"]) for s in schedules]      # a schedule row's `command` is segment 0's
    else:
        commands = [command_row(c) for c in (args.command or [])]
        if args.grid:
            commands += parse_grid(args.grid)
    if not commands:
        raise SystemExit("give at least one --command or a --grid")
    plants = plants_from_args(args)      # [] without --plant / --plant_grid; refusals (pushes next to plants among them) before any batch work
    pushes = [push_row(p) for p in (getattr(args, "push", None) or [])]
    if getattr(args, "push_grid", None):
        pushes += parse_push_grid(args.push_grid)
    sensors = sensors_from_args(args)    # [] without --sensor / --sensor_grid; refusals (pushes or plants next to sensors among them) before any batch work
    actuations = actuations_from_args(args)    # [] without --actuation / --actuation_grid; refusals (another cell axis next to them) before any batch work
    axis = cell_axis(args, pushes, plants, sensors, actuations)
    ncell = len(axis.cells) if axis else 1      # cells per command
    randomized = bool(getattr(args, "randomize", False))
    imitation = bool(getattr(args, "imitation_report", False))
    for why in (imitation_refusal(args) if imitation else None, falls_refusal(args)):      # before any batch work
        if why:
            raise SystemExit(why)
    E = int(args.envs_per_command)
    n = len(commands) * ncell * E
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    env = make_env(args, n, args.device)
    motion = getattr(env, "reference_motion", None)
    if motion is not None:
        print(motion.describe(), file=sys.stderr)      # stdout may carry the JSON report
    if hasattr(env, "describe_head_joints"):
        print(env.describe_head_joints(), file=sys.stderr)
    if way is not None:
        why = waypoint_limits_refusal(way["speed"], way["turn_rate"], env.batch.cfg.cmd_range)
        if why:
            raise SystemExit(why)
    try:      # what the reductions need of the robot, before the checkpoint is read
        head = posture_head_map(env) if getattr(args, "posture", False) else None
        imitation_info = imitation_joint_info(env) if imitation else None
    except ValueError as err:
        raise SystemExit(str(err))
    net = load_networks(args.checkpoint, env, dev)
    delays_t = None
    if plants or randomized:      # per-env model parameters: the training-time draw, the plants' scales, or the one times the other
        from . import randomize
        fields = randomize.domain_randomize(env.mj_model, np.random.default_rng(int(args.seed)), n)[0] if randomized else None
        if plants:
            _, scales, delays_np = plant_blocks(commands, plants, E)
            fields = plant_fields(env.mj_model, scales, fields)
            delays_t = torch.from_numpy(delays_np).to(dev)
        randomize.apply(env.batch, fields)
    cmd_np, kicks_np = cell_blocks(commands, pushes, E) if pushes else (command_blocks(commands, ncell * E), None)
    cmd = torch.from_numpy(cmd_np).to(dev)      # with schedules: segment 0's; the Tracker's apply launch rewrites it every step
    env.set_commands(cmd)
    reports = []      # in launch order
    if pushes:
        if int(args.push_at) < 0:
            raise SystemExit("--push_at is a step of the episode: >= 0")
        reports.append(push_report(env, torch.from_numpy(kicks_np).to(dev), int(args.push_at), args.push_tolerance, entries=pushes, envs_per_cell=E,
                                   flags=dict(push=getattr(args, "push", None), push_grid=getattr(args, "push_grid", None))))
    if getattr(args, "gait", False):
        reports.append(gait_report(env))
    if head is not None:
        reports.append(posture_report(env, getattr(args, "posture_tolerance", DEFAULT_POSTURE_TOLERANCE), head))
    if imitation:
        reports.append(imitation_report(env, imitation_info))
    if schedules is not None:
        then = getattr(args, "then", None)
        reports.append(response_report(env, dict(
            table=schedule_table(schedules), map=schedule_blocks(len(schedules), ncell * E), tolerance=response_tolerance(args),
            tail_after=getattr(args, "response_tail_after", DEFAULT_RESPONSE_TAIL_AFTER), schedules=schedules,
            flags=dict(sequence=getattr(args, "sequence", None), then=then, switch_at=int(getattr(args, "switch_at", DEFAULT_SWITCH_AT)) if then else None))))
    falls = None
    if getattr(args, "falls", False):      # (falls_refusal has seen the flags)
        falls = dict(ring=int(getattr(args, "fall_ring", DEFAULT_FALL_RING)), tilt_tol=fall_tilt_tol(getattr(args, "fall_tilt", DEFAULT_FALL_TILT)),
                     tilt=float(getattr(args, "fall_tilt", DEFAULT_FALL_TILT)), save=getattr(args, "save_falls", None),
                     save_max=int(getattr(args, "save_falls_max", DEFAULT_SAVE_FALLS_MAX)))
        reports.append(fall_report(env, falls))
    if way is not None:
        reports.append(waypoint_report(env, dict(way, table=course_table(way["courses"]), map=schedule_blocks(len(way["courses"]), ncell * E))))
    elif getattr(args, "path", False):
        reports.append(path_report(env, constant=schedules is None))
    fault_t = torch.from_numpy(sensor_blocks(len(commands), sensors, E, int(args.seed))).to(dev) if sensors else None
    act_fault_t = None
    if actuations:
        try:      # (a `freeze` names one of this robot's actuators: known once the env is made)
            act_fault_t = torch.from_numpy(actuation_blocks(len(commands), actuations, E, int(args.seed), float(env.batch.cfg.action_scale), float(env.dt),
                                                            [str(s) for s in env.batch.model.a["names_actuator"]])).to(dev)
        except ValueError as err:
            raise SystemExit(str(err))
    tr = Tracker(env, net, delays=delays_t, reports=reports, **(dict(sensors=dict(fault=fault_t)) if sensors else {}),
                 **(dict(actuation=dict(fault=act_fault_t)) if actuations else {}))
    reports = sorted(reports, key=lambda r: not r.drives)      # the report's order: pushes and schedules first (a stable sort)
    nobs = env.observation_size["state"][0]
    T = int(args.episode_length)
    save_obs_path, save_qpos_path = getattr(args, "save_obs", None), getattr(args, "save_qpos", None)
    obs_hist = torch.zeros(T, nobs, device=dev) if save_obs_path else None
    qpos_hist = []
    with torch.no_grad():
        tr.reset(args.seed)
        if save_qpos_path:
            qpos_hist.append(env.batch.get_state()[0][0].copy())
        for t in range(T):
            tr.step()
            if obs_hist is not None:
                # env 0's observation, stream-ordered after the step; with sensor faults the row the policy read in this step
                obs_hist[t].copy_(env.batch.obs[0] if tr.sensor_obs is None else tr.sensor_obs[0])
            if save_qpos_path:
                qpos_hist.append(env.batch.get_state()[0][0].copy())
        acc = tr.acc.cpu().numpy()
        accs = [r.acc.cpu().numpy() for r in reports]
    rows = report_rows(acc, list(zip(reports, accs)), commands, axis, E)
    if actuations:      # the stage's own counters, per cell
        cells = [cell for row in rows for cell in row[axis.row_key]]
        for cell, link in zip(cells, reduce_link(tr.actuation_state.cpu().numpy(), len(cells), E)):
            cell["link"] = link
    if falls and falls["save"]:      # the clips of every row, or with a cell axis of every cell
        save_falls(falls["save"], fall_clips(accs[[r.key for r in reports].index("falls")], block_commands(rows, axis), E, falls["ring"],
                                             int(env.batch.model.nq), falls["save_max"]), float(env.dt))
    settings = dict(checkpoint=args.checkpoint, trained_under=trained_under(args.checkpoint), env=args.env, task=args.task, xml=args.xml, cone=args.cone,
                    hfield_up_normals_only=bool(args.hfield_up_normals_only), envs_per_command=E, episode_length=T, seed=int(args.seed),
                    num_envs=n, dt=float(env.dt), policy="deterministic tanh(loc)", fused_policy=tr.fp is not None, graph=tr.graph is not None,
                    reference_motion=getattr(args, "reference_motion", None), reference_motion_sha256=motion.sha256 if motion is not None else None)
    with_curriculum = trained_with_curriculum(args.checkpoint)
    if with_curriculum is not None:      # only then: every other checkpoint keeps its keys
        settings.update(trained_with_curriculum=with_curriculum)
    settings.update({k: v for r in reports if r.drives for k, v in r.settings.items()})
    if axis:
        settings.update(axis.settings)
    if randomized:
        settings.update(randomize=True)
    if getattr(args, "noise_level", None) is not None:
        settings.update(noise_level=float(args.noise_level))
    settings.update({k: v for r in reports if not r.drives for k, v in r.settings.items()})
    report = make_report(settings, rows)
    if save_obs_path:
        save_obs(save_obs_path, obs_hist.cpu().numpy())
    if save_qpos_path:
        np.savez(save_qpos_path, qpos=np.stack(qpos_hist), dt=np.float64(env.dt))
    text = json.dumps(report, indent=1)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text + "\n")
    else:
        print(text, file=out)
    env.set_commands(None)
    if pushes:
        env.set_pushes(None)
    if delays_t is not None:
        env.set_action_delays(None)
    return report


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Velocity tracking of a trained policy under given commands (GPU)")
    p.add_argument("--checkpoint", required=True, help="a checkpoint written by runner (ppo/train.py save_checkpoint)")
    p.add_argument("--env", type=str, default="joystick", help="env (as runner)")
    p.add_argument("--task", type=str, default="flat_terrain", help="task (as runner)")
    p.add_argument("--xml", type=str, default=None, help="a robot of your own: its MJCF (as runner)")
    p.add_argument("--cone", choices=["pyramidal", "elliptic"], default=None, help="friction cone (as runner)")
    p.add_argument("--hfield_up_normals_only", action="store_true", help="height-field contact reading (as runner)")
    from .runner import add_head_joint_flag, add_imitation_flags
    add_imitation_flags(p)
    add_head_joint_flag(p)
    p.add_argument("--command", nargs="+", type=float, action="append", metavar="V",
                   help="vx vy wz [neck_pitch head_pitch head_yaw head_roll]; repeat for more commands")
    p.add_argument("--grid", type=str, default=None, help="a grid of commands: vx=a:b:n,wz=c:d:m (axes vx vy wz neck_pitch head_pitch head_yaw head_roll)")
    p.add_argument("--envs_per_command", type=int, default=128, help="envs per command, or per (command, push) / (command, plant) cell when pushes / plants are given")
    p.add_argument("--push", nargs=2, type=float, action="append", metavar=("DVX", "DVY"),
                   help="a world-frame velocity kick in m/s, added once to the base's planar velocity; repeat for more pushes")
    p.add_argument("--push_grid", type=str, default=None, help="a grid of pushes: magnitude=a:b:n,direction=c:d:m (m/s; degrees, world frame, 0 = +x)")
    p.add_argument("--push_at", type=int, default=DEFAULT_PUSH_AT, help="the step of the first episode (0 = its first) at which the kick is applied, once")
    p.add_argument("--push_tolerance", nargs=2, type=float, default=list(DEFAULT_PUSH_TOLERANCE), metavar=("LIN", "ANG"),
                   help="recovery: planar velocity error (m/s) and yaw-rate error (rad/s) above which a step counts as not recovered (BUILD-DEFINED defaults)")
    p.add_argument("--plant", type=str, action="append", metavar="KEY=V[,KEY=V...]",
                   help="a plant: scales kp (every actuator's gain, the bias following), mass (every body's mass; inertias are NOT rescaled, as the "
                        "reference's randomize.py), frictionloss and armature (the actuated dofs') on the model's values, and delay = 0, 1, 2 or "
                        "random (the action delay in control steps; random, the default, is the sampler); axes not named stay nominal; repeat "
                        "for more plants.  Every (command, plant) cell gets --envs_per_command envs; every command row gains \"plants\" and "
                        "\"robustness\".  Not with --push / --push_grid")
    p.add_argument("--plant_grid", type=str, default=None,
                   help="a cross product of plants: kp=0.7:1.3:4,mass=0.9:1.2:3,delay=0:2:3 (--grid's syntax; axes kp mass frictionloss armature "
                        "delay; a delay axis must come out as whole numbers within 0..2)")
    p.add_argument("--robust_fall_rate", type=float, default=DEFAULT_ROBUST_FALL_RATE, metavar="RATE",
                   help="robustness: the fall rate up to which a plant counts as survived in \"survived_range\" (a reporting threshold of the "
                        "user's, not a measured constant); read with plants, sensor faults or actuation faults only")
    p.add_argument("--sensor", type=str, action="append", metavar="KEY=V[,KEY=V...]",
                   help="a sensor fault between the env's observation and the policy: gyro_bias_x|y|z (rad/s), gyro_scale, acc_bias_x|y|z (m/s^2), "
                        "acc_scale, imu_roll|imu_pitch|imu_yaw (degrees: a tilted IMU mount), imu_delay, joint_delay (whole control steps, 0 .. 7), "
                        "encoder_offset (rad: every env draws each actuator's zero error uniformly in +-X, seeded by --seed), encoder_quant (rad), "
                        "contact_left|contact_right = ok|off|on (a foot switch that sticks); keys not named stay nominal; repeat for more settings.  "
                        "Every (command, sensor) cell gets --envs_per_command envs; every command row gains \"sensors\" and \"sensor_robustness\".  "
                        "Not with --push / --push_grid or --plant / --plant_grid")
    p.add_argument("--sensor_grid", type=str, default=None,
                   help="a cross product of sensor settings: imu_delay=0:7:8,gyro_bias_y=-0.3:0.3:5 (--grid's syntax; every key of --sensor but the "
                        "contact ones; a delay axis must come out as whole numbers within 0..7)")
    p.add_argument("--actuation", type=str, action="append", metavar="KEY=V[,KEY=V...]",
                   help="a fault between the policy's action and the servos: gain, offset (rad: every env draws each actuator's horn error "
                        "uniformly in +-X, seeded by --seed), noise (action units, uniform +-X), limit (action units, a clamp; 0 = off), cutoff (Hz, "
                        "the reference's low-pass action filter; 0 = off), quant (rad, the servo's position step; 0 = off), drop (0..1, the "
                        "probability that a step's packet is lost: the servos keep their last target), drop_len (whole steps >= 1 a loss "
                        "lasts), freeze=ACTUATOR|none with freeze_at (the episode step from which that servo is off the bus); keys not named "
                        "stay nominal; repeat for more settings.  Every (command, actuation) cell gets --envs_per_command envs; every command "
                        "row gains \"actuations\" and \"actuation_robustness\".  Not with pushes, plants or sensor faults")
    p.add_argument("--actuation_grid", type=str, default=None,
                   help="a cross product of actuation settings: cutoff=5:40:3,drop=0:0.2:2 (--grid's syntax; every key of --actuation but "
                        "freeze; drop_len and freeze_at axes must come out as whole numbers)")
    p.add_argument("--randomize", action="store_true",
                   help="apply the training-time domain randomisation (randomize.domain_randomize, seeded by --seed) to every env; a plant's "
                        "scales multiply it")
    p.add_argument("--noise_level", type=float, default=None, metavar="X", help="override noise_config.level (default: the env's own, 1.0)")
    p.add_argument("--sequence", type=str, action="append", metavar="SCHEDULE",
                   help="a command schedule: \"0: 0 0 0 | 150: 0.15 0 0 | 400: 0 0 0.5\" -- segments apart by |, each `start_step: vx vy wz "
                        "[neck_pitch head_pitch head_yaw head_roll]`, the first at step 0, at most 8; repeat for more schedules.  Each is one row of "
                        "the report with a \"segments\" list: per segment the response time, settle time, overshoot, steady-state error and fall rate "
                        "after the change.  Not with --command / --grid / --then, pushes or --posture")
    p.add_argument("--then", nargs="+", type=float, action="append", metavar="V",
                   help="switch every --command / --grid row to this command (vx vy wz [...]) at step --switch_at; repeat for more targets: every "
                        "(from, then) pair is a two-segment schedule and a row of the report, from-commands outermost")
    p.add_argument("--switch_at", type=int, default=DEFAULT_SWITCH_AT, help="the step of the first episode at which --then takes over")
    p.add_argument("--response_tolerance", nargs=2, type=float, default=list(DEFAULT_PUSH_TOLERANCE), metavar=("LIN", "ANG"),
                   help="response: planar velocity error (m/s) and yaw-rate error (rad/s) within which a step counts as following the segment's "
                        "command (BUILD-DEFINED defaults, --push_tolerance's); read with schedules only")
    p.add_argument("--response_tail_after", type=int, default=DEFAULT_RESPONSE_TAIL_AFTER, metavar="STEPS",
                   help="steady state: the samples later than this many steps into a segment give its steady-state error; read with schedules only")
    p.add_argument("--gait", action="store_true",
                   help="add a \"gait\" object to every command row (and push cell): duty factor, double support, flight, step frequency, swing time and "
                        "foot slip per foot, root height, roll/pitch rate RMS, action rate, mean |torque * joint speed| and per-actuator torque RMS / peak "
                        "against the force range, saturation share (>= 99 %% of the limit), speed peak, power and joint range.  cost_of_transport = "
                        "sum |torque * joint speed| / (m g sum of planar speed): m is the model's nominal total mass (not a randomised one), g the model's "
                        "gravity; null when the distance covered (sum of planar speed * dt) is under 1 cm")
    p.add_argument("--posture", action="store_true",
                   help="add a \"posture\" object to every command row (and push cell): per mapped head slot (neck_pitch, head_pitch, head_yaw, head_roll) "
                        "the joint, the command, mean angle, RMS and peak error, settle time and settled fraction; the mean cost_head_pos; and the "
                        "robot's stillness (drift speed, yaw and roll/pitch rate RMS, lean, root height, leg pose deviation and leg joint speed).  "
                        "The head-joint map is the duck's own, or --env standing --head_joints for another robot")
    p.add_argument("--posture_tolerance", type=posture_tolerance, default=DEFAULT_POSTURE_TOLERANCE, metavar="RAD",
                   help="settling: the head joint error (rad) above which a step counts as not settled (BUILD-DEFINED default); read by --posture only")
    p.add_argument("--imitation_report", action="store_true",
                   help="add an \"imitation\" object to every command row (and push cell): does the policy walk the reference gait?  Per compared "
                        "joint (the imitation joint map) the bias, RMS and peak error against the reference motion, the velocity RMS error, the range "
                        "used against the reference's and their ratio; the reward's joint_pos, joint_vel and contact terms; per foot the contact "
                        "agreement, stance shares, touchdowns and the touchdown lag behind the reference's (negative: early); the planar speed error.  "
                        "The Joystick task with the imitation reward: the duck, or another robot with --reference_motion")
    p.add_argument("--falls", action="store_true",
                   help="add a \"falls\" object to every command row (push cell, schedule row): fall rate and fall step, the direction of the fall "
                        "(forward / backward / left / right in the base body's frame, from the last recorded sample), the onset (time from the last "
                        "upright sample to the termination, and the support foot then), the share of falls with a saturated actuator, how close the "
                        "survivors came, and the mean profile of lean, height, roll/pitch rate, command error and saturation before the termination")
    p.add_argument("--fall_ring", type=int, default=DEFAULT_FALL_RING, metavar="N",
                   help=f"samples kept per env before the end of its first episode, 1 .. {FALL_MAX_RING} (50: one second at the duck's control step).  "
                        "Device memory: (16 + N * (16 + nq)) floats per env, 61 MB for 8192 duck envs at the default; read by --falls only")
    p.add_argument("--fall_tilt", type=float, default=DEFAULT_FALL_TILT, metavar="RAD",
                   help="the lean (rad, 0 .. pi/2) up to which a sample counts as upright; the device compares the sine (BUILD-DEFINED default); "
                        "read by --falls only")
    p.add_argument("--save_falls", type=str, default=None, metavar="PATH",
                   help="with --falls: the pre-fall clips of the first --save_falls_max falls of every row (with pushes: cell) as .npz -- qpos "
                        "[k, ring, nq] in time order, zero-padded at the front, valid [k], steps, env, row, fall_step, command and dt; "
                        "qpos[i, ring - valid[i]:] replays like --save_qpos")
    p.add_argument("--save_falls_max", type=int, default=DEFAULT_SAVE_FALLS_MAX, metavar="K", help="clips kept per row (cell); read by --save_falls only")
    p.add_argument("--path", action="store_true",
                   help="add a \"path\" object to every command row (push cell, plant cell, schedule row): where did it end up?  The base pose is "
                        "integrated on the device in each env's start frame (the pose right after the reset): forward and lateral displacement, heading "
                        "change, path length and straightness, each as mean and std over the envs, and for a row with one constant command the "
                        "dead-reckoned ideal pose and the mean distance to it.  Any robot, both tasks, every other flag")
    p.add_argument("--waypoints", type=str, action="append", metavar="COURSE",
                   help="a course for the waypoint follower: \"0.5,0 | 0.5,0.5 | 0,0.5 | 0,0\" -- 1 to 8 points x,y in metres in each env's start "
                        "frame, apart by |; repeat for more courses.  Each is one row of the report with \"path\" and \"course\": per waypoint the "
                        "share of envs that reached it and when, the cross-track error, the distance left to the goal, the path length against the "
                        "course's and the falls by leg.  The follower writes vx and wz of the command inside the captured step.  A course that begins "
                        "with a minus sign is written --waypoints=\"-0.05,0.05 | ...\" (argparse reads a bare one as a flag).  Implies --path; not "
                        "with --command / --grid / --sequence / --then, pushes or --posture")
    p.add_argument("--waypoint_radius", type=float, default=DEFAULT_WAYPOINT_RADIUS, metavar="M",
                   help="the distance (m) within which a waypoint counts as reached (BUILD-DEFINED default, a controller setting)")
    p.add_argument("--waypoint_speed", type=float, default=DEFAULT_WAYPOINT_SPEED, metavar="MPS",
                   help="the follower's cruise speed (m/s, within the env's vx command range; BUILD-DEFINED default)")
    p.add_argument("--waypoint_turn_rate", type=float, default=DEFAULT_WAYPOINT_TURN_RATE, metavar="RADPS",
                   help="the follower's largest yaw-rate command (rad/s, within the env's wz command range; BUILD-DEFINED default)")
    p.add_argument("--waypoint_gain", type=float, default=DEFAULT_WAYPOINT_GAIN, metavar="G",
                   help="yaw-rate command per unit sine of the heading error (rad/s; BUILD-DEFINED default)")
    p.add_argument("--waypoint_slow_dist", type=float, default=DEFAULT_WAYPOINT_SLOW_DIST, metavar="M",
                   help="the distance (m) from the LAST waypoint inside which the speed command falls linearly to 0 (BUILD-DEFINED default)")
    p.add_argument("--episode_length", type=int, default=1000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--output", type=str, default=None, help="write the JSON report here (default: stdout)")
    p.add_argument("--save_obs", type=str, default=None, help="env 0's `state` observation per step, pickled list of arrays (mujoco_saved_obs.pkl format)")
    p.add_argument("--save_qpos", type=str, default=None, help="env 0's qpos per step (first row: after reset) and dt, as .npz")
    return p


def main(argv=None):
    from .runner import check_env_flags
    parser = build_parser()
    args = parser.parse_args(argv)
    check_env_flags(parser, args)
    run(args)


if __name__ == "__main__":
    main()
