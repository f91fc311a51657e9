"""Runs training for Open Duck Mini V2 (mirror of reference playground/open_duck_mini_v2/runner.py and
playground/common/runner.py).  Same flags as the reference (runner.py:36-56) plus additive ones
(--num_envs, --seed, --device, --no_randomize).  Launch with torchrun for multi-GPU data parallelism.

    python -m open_duck_playground_amd.runner --task flat_terrain --num_timesteps 150000000
"""
from __future__ import annotations

import argparse
import os
from datetime import datetime

import numpy as np


def _parse_kv(item: str, flag: str):
    if "=" not in item:
        raise ValueError(f"{flag} {item!r}: expected KEY=VALUE")
    k, v = item.split("=", 1)
    return k.strip(), v.strip()


def reward_overrides(env: str, scales=None, params=None) -> dict:
    """--reward_scale KEY=VALUE / --reward_param KEY=VALUE -> config overrides (`reward_config.scales.KEY`, `reward_config.KEY`;
    soft_joint_pos_limit_factor is a top-level key).  A scale key must be one of the env's native reward slots or a reward-library term
    (joystick.LIBRARY_TERMS); a parameter key one of joystick.REWARD_PARAMS: anything else is a ValueError (a typo on the command line
    would otherwise train silently without the term).  air_time_range and pose_weights take comma-separated numbers."""
    from . import joystick, standing
    native = {"joystick": joystick.REWARD_SLOTS, "standing": standing.REWARD_SLOTS}.get(env, joystick.REWARD_SLOTS)
    known = [k for k in native if k is not None] + [k for k in joystick.LIBRARY_TERMS if k not in native]
    out = {}
    for item in scales or ():
        k, v = _parse_kv(item, "--reward_scale")
        if k not in known:
            raise ValueError(f"--reward_scale {k}: unknown reward key for env {env} (known: {', '.join(known)})")
        out[f"reward_config.scales.{k}"] = float(v)
    for item in params or ():
        k, v = _parse_kv(item, "--reward_param")
        if k not in joystick.REWARD_PARAMS:
            raise ValueError(f"--reward_param {k}: unknown reward parameter (known: {', '.join(joystick.REWARD_PARAMS)})")
        if k in ("air_time_range", "pose_weights"):
            val = [float(x) for x in v.split(",") if x.strip()]
            if k == "air_time_range" and len(val) != 2:
                raise ValueError(f"--reward_param air_time_range={v}: expected two numbers MIN,MAX")
        else:
            val = float(v)
        out[k if k == "soft_joint_pos_limit_factor" else f"reward_config.{k}"] = val
    return out


def _names(spec):
    return [n.strip() for n in spec.split(",") if n.strip()] if spec else None


def imitation_overrides(args) -> dict:
    """--reference_motion PATH / --imitation_joints a,b,... / --imitation_ignore a,b,... -> the Joystick config keys reference_motion,
    imitation_joints, imitation_ignore (those not given stay out)."""
    out = {}
    if getattr(args, "reference_motion", None):
        out["reference_motion"] = args.reference_motion
    for k in ("imitation_joints", "imitation_ignore"):
        names = _names(getattr(args, k, None))
        if names is not None:
            out[k] = names
    return out


def parse_head_joints(spec: str) -> dict:
    """--head_joints SLOT=JOINT[,SLOT=JOINT...] | none -> the Standing config key head_joints ({} for `none`: no head joints).  The names
    are resolved against the robot by standing.head_joint_map."""
    if spec.strip().lower() == "none":
        return {}
    out = {}
    for item in spec.split(","):
        if not item.strip():
            continue
        k, v = _parse_kv(item, "--head_joints")
        if k in out:
            raise ValueError(f"--head_joints {k}: slot given twice")
        out[k] = v
    if not out:
        raise ValueError(f"--head_joints {spec!r}: expected SLOT=JOINT[,SLOT=JOINT...] or none")
    return out


def head_joint_overrides(args) -> dict:
    """--head_joints -> the Standing config key head_joints (nothing when the flag is not given); ValueError with another --env."""
    spec = getattr(args, "head_joints", None)
    if spec is None:
        return {}
    if args.env != "standing":
        raise ValueError(f"--head_joints is a flag of --env standing (the {args.env} env has no head-joint map)")
    return {"head_joints": parse_head_joints(spec)}


def config_overrides(args):
    """The env's config_overrides from the command line (None when nothing is overridden)."""
    overrides = {"hfield_up_normals_only": True} if getattr(args, "hfield_up_normals_only", False) else None
    if getattr(args, "cone", None):
        overrides = dict(overrides or {}, cone=args.cone)
    overrides = dict(overrides or {}, **reward_overrides(args.env, getattr(args, "reward_scale", None), getattr(args, "reward_param", None)))
    return dict(overrides, **imitation_overrides(args), **head_joint_overrides(args)) or None


def add_imitation_flags(parser) -> None:
    parser.add_argument("--reference_motion", type=str, default=None, metavar="PATH",
                        help="train with the imitation reward on this reference motion (a polynomial_coefficients.pkl, reference README "
                             "'imitation reward'); any robot.  Default: the duck's shipped table for the duck, no imitation reward otherwise")
    parser.add_argument("--imitation_joints", type=str, default=None, metavar="A,B,...",
                        help="the reference motion's frame joints in frame order (default: the duck's 16 for the duck, the actuated joints otherwise)")
    parser.add_argument("--imitation_ignore", type=str, default=None, metavar="A,B,...",
                        help="frame joints the imitation reward leaves out (default: the duck's antennas for the duck, none otherwise)")


def add_head_joint_flag(parser) -> None:
    parser.add_argument("--head_joints", type=str, default=None, metavar="SLOT=JOINT[,SLOT=JOINT...]|none",
                        help="--env standing on a robot of your own: the joints that track the posture commands (slots neck_pitch, head_pitch, "
                             "head_yaw, head_roll; a slot left out has none), or `none` for a robot without head joints.  Default: the duck's "
                             "head for the duck; another robot needs the flag")


class OpenDuckMiniV2Runner:
    def __init__(self, args):
        import torch
        import torch.distributed as dist
        from . import joystick, standing
        from .ppo import train as ppo_train
        self.args = args
        self.output_dir = os.path.join(os.getcwd(), args.output_dir)
        available_envs = {"joystick": joystick.Joystick, "standing": standing.Standing}   # reference runner.py:14-17
        if args.env not in available_envs:
            raise ValueError(f"Unknown env {args.env}")
        self.world = int(os.environ.get("WORLD_SIZE", "1")); self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world > 1 and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        device = args.device if self.world == 1 else local_rank
        torch.cuda.set_device(device)
        n_local = args.num_envs // self.world
        overrides = config_overrides(args)
        extra = {}
        if getattr(args, "xml", None):      # a robot of one's own (reference README.md:74-85 "Adding a new robot"): its MJCF instead of a shipped task
            extra["xml_path"] = args.xml
        self.env = available_envs[args.env](task=args.task, num_envs=n_local, device=device, env_id_offset=self.rank * n_local, config_overrides=overrides, **extra)
        if getattr(self.env, "reference_motion", None) is not None:
            print(self.env.reference_motion.describe())
        if hasattr(self.env, "describe_head_joints"):
            print(self.env.describe_head_joints())
        # training under faults redrawn per episode (fault_training.py): a stage of the training env only -- the Evaluator stays the nominal robot
        from . import fault_training
        self.fault_spec = fault_training.spec_from_args(args)      # None without --train_sensor / --train_actuation: no stage at all
        self.faults = None if self.fault_spec is None else fault_training.FaultStage(self.env, self.fault_spec, seed=args.seed)
        if self.faults is not None:
            import json
            print(f"Training under faults: {json.dumps(self.faults.describe())}")
        # the command curriculum (command_curriculum.py): it draws the training env's commands -- the Evaluator keeps the nominal sampled ones
        from . import command_curriculum
        self.curriculum_spec = command_curriculum.spec_from_args(args, self.env)      # None without --command_curriculum: every launch is as before
        self.curriculum = None if self.curriculum_spec is None else command_curriculum.CommandCurriculum(self.env, self.curriculum_spec, seed=args.seed)
        if self.curriculum is not None:
            import json
            print(f"Command curriculum: {json.dumps(self.curriculum_spec)}")
        self.action_size = self.env.action_size
        self.obs_size = int(self.env.observation_size["state"][0])
        # one generator per (seed, rank, stream): stream 0 = training envs, 1 = evaluation envs (ppo/train.py)
        self.randomizer = None if args.no_randomize else (lambda env, stream=0: env.randomize(np.random.default_rng([args.seed, self.rank, stream])))
        self.ppo = ppo_train
        print(f"Observation size: {self.obs_size}")

    def progress_callback(self, num_steps, metrics):   # rank 0 only (ppo/train.py)
        for name, value in metrics.items():   # reference common/runner.py:58-60
            self.writer.add_scalar(name, value, num_steps)
        self.writer.flush()
        print("-----------")
        print(f'STEP: {num_steps} reward: {metrics.get("eval/episode_reward")} reward_std: {metrics.get("eval/episode_reward_std")}'
              f' sps: {metrics.get("training/sps", 0.0):.0f}')
        print("-----------")

    def policy_params_fn(self, current_step, net):
        d = datetime.now().strftime("%Y_%m_%d_%H%M%S")
        path = f"{self.output_dir}/{d}_{current_step}.pt"
        print(f"Saving checkpoint (step: {current_step}): {path}")
        self.ppo.save_checkpoint(path, net, fault_spec=None if self.faults is None else self.faults.describe(),
                                 command_curriculum=None if self.curriculum is None else self.curriculum.describe())
        from .export_onnx import export_onnx   # reference common/runner.py:77-84
        export_onnx(net, output_path=f"{self.output_dir}/{d}_{current_step}.onnx")

    def train(self):
        self.writer = None
        if self.rank == 0:   # one writer, one output directory: the other ranks only train
            os.makedirs(self.output_dir, exist_ok=True)
            from .tb_writer import SummaryWriter
            self.writer = SummaryWriter(self.output_dir)   # reference common/runner.py:38-39 (tensorboardX)
        try:
            return self.ppo.train(self.env, num_timesteps=self.args.num_timesteps, progress_fn=self.progress_callback,
                                  policy_params_fn=self.policy_params_fn, restore_checkpoint_path=self.args.restore_checkpoint_path,
                                  seed=self.args.seed, randomization_fn=self.randomizer, log_path=os.path.join(self.output_dir, "metrics.jsonl"),
                                  faults=self.faults, curriculum=self.curriculum, num_envs=self.args.num_envs)
        finally:
            if self.writer is not None:
                self.writer.close()

    def close(self):
        import torch.distributed as dist
        if self.world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Open Duck Mini Runner Script")
    parser.add_argument("--output_dir", type=str, default="checkpoints", help="Where to save the checkpoints")
    parser.add_argument("--num_timesteps", type=int, default=150000000)
    parser.add_argument("--env", type=str, default="joystick", help="env")
    parser.add_argument("--task", type=str, default="flat_terrain", help="Task to run")
    parser.add_argument("--restore_checkpoint_path", type=str, default=None, help="Resume training from this checkpoint")
    parser.add_argument("--num_envs", type=int, default=8192)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--no_randomize", action="store_true")
    parser.add_argument("--hfield_up_normals_only", action="store_true",
                        help="height-field floors: count a prism pair's contacts only when the normal points up (BUILD-DEFINED opt-in, DESIGN 2; "
                             "the reading under which rough_terrain_backlash trains: profiles/r4/hfield_variants.json)")
    parser.add_argument("--cone", choices=["pyramidal", "elliptic"], default=None,
                        help="friction cone of the contact solver (what <option cone=...> in the robot's XML sets; default: the model's own, pyramidal for the duck)")
    parser.add_argument("--xml", type=str, default=None,
                        help="train a robot of your own: path of its MJCF (additive; the reference's recipe is a copy of this package per robot, README.md:74-85). "
                             "The XML carries the names constants.py looks up (sites imu / left_foot / right_foot, geoms left_foot_bottom_tpu / right_foot_bottom_tpu / "
                             "floor, the 15 sensors, keyframe home); its model shape needs a compiled kernel: tools/new_shape.py <xml> prints the lines to add")
    parser.add_argument("--reward_scale", action="append", default=[], metavar="KEY=VALUE",
                        help="repeatable: set reward_config.scales[KEY]; a native slot of the env or a reward-library term (README: reward library), "
                             "e.g. feet_air_time=2.0; a non-zero scale turns a library term on")
    parser.add_argument("--reward_param", action="append", default=[], metavar="KEY=VALUE",
                        help="repeatable: a parameter of the library terms: base_height_target, max_foot_height, air_time_range=MIN,MAX, "
                             "pose_weights=W1,...,Wnu, soft_joint_pos_limit_factor")
    parser.add_argument("--train_sensor", action="append", default=[], metavar="KEY=V|KEY=LO:HI[,...]",
                        help="repeatable: train under a sensor fault between the env's observation and the policy, with track --sensor's keys "
                             "and units.  KEY=V is fixed; KEY=LO:HI is redrawn per env at the start of every episode, uniformly (imu_delay / "
                             "joint_delay: the whole steps LO .. HI).  encoder_offset=X redraws every actuator's zero error in +-X; the IMU "
                             "mounting angles and the contact modes take one value.  e.g. imu_delay=0:3,acc_bias_x=1.3")
    parser.add_argument("--train_actuation", action="append", default=[], metavar="KEY=V|KEY=LO:HI[,...]",
                        help="repeatable: train under a fault between the policy's action and the servos, with track --actuation's keys and "
                             "units, fixed or redrawn per episode as --train_sensor's.  cutoff=A:B draws the filter coefficient uniformly "
                             "between the two cutoffs' (a range that holds 0 = off is refused); offset=X redraws every actuator's horn error "
                             "in +-X; freeze and freeze_at take one value.  e.g. cutoff=15:40,drop=0:0.05")
    parser.add_argument("--command_curriculum", type=str, default=None, metavar="AXIS=LO:HI:BINS[,...]",
                        help="--env joystick: train on commands drawn from a grid over vx, vy, wz whose bins open as the policy tracks well inside "
                             "their neighbours (an axis not named keeps the env's range with one bin; at most 16 bins per axis, 4096 in all).  "
                             "e.g. vx=-0.15:0.222:8,vy=-0.2:0.2:4,wz=-1.1:1.2:8 (a grid beyond the reference-motion table is refused while the "
                             "imitation reward is on: --curriculum_allow_clipped_reference)")
    parser.add_argument("--curriculum_start", type=str, default=None, metavar="AXIS=LO:HI[,...]",
                        help="the range whose bins are open from the start (those whose centre lies inside it; default: the env config's command "
                             "ranges).  A start that covers the whole grid is uniform sampling over the grid")
    parser.add_argument("--curriculum_allow_clipped_reference", action="store_true",
                        help="take a grid wider than the reference-motion table while the imitation reward is on (a warning instead of a refusal)")
    from .command_curriculum import SETTINGS as curriculum_settings
    for key, what in (("period", "steps per command (a stint)"), ("skip", "steps of a stint before its first velocity sample"),
                      ("min_samples", "samples a stint needs to be judged"), ("min_tries", "judged stints a bin needs before it can promote"),
                      ("promote_rate", "share of successful stints that promotes a bin's neighbourhood"),
                      ("tol_lin", "planar RMS velocity error of a successful stint, m/s"),
                      ("tol_yaw", "yaw-rate RMS error of a successful stint, rad/s"), ("p_zero", "share of all-zero commands")):
        whole = isinstance(curriculum_settings[key], int)
        parser.add_argument(f"--curriculum_{key}", type=int if whole else float, default=None,
                            help=f"command curriculum: {what} (default {curriculum_settings[key]})")
    add_imitation_flags(parser)
    add_head_joint_flag(parser)
    return parser


def check_env_flags(parser, args) -> None:
    """Refuses a flag of another --env right after parsing, before any GPU or process-group set-up (argparse error, exit status 2)."""
    try:
        head_joint_overrides(args)
        if getattr(args, "train_sensor", None) or getattr(args, "train_actuation", None):
            from . import fault_training
            fault_training.spec_from_args(args)
        from . import command_curriculum
        if command_curriculum.spec_from_args(args) is not None and args.env != "joystick":
            raise ValueError(f"--command_curriculum belongs to --env joystick: the {args.env} task has no velocity commands to track "
                             "(its commands are head postures)")
    except ValueError as e:
        parser.error(str(e))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_env_flags(parser, args)
    runner = OpenDuckMiniV2Runner(args)
    try:
        runner.train()
    finally:
        runner.close()


if __name__ == "__main__":
    main()
