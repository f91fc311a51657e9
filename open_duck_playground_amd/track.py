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
"""
from __future__ import annotations

import argparse
import itertools
import json
import pickle
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

COMMAND_KEYS = ("vx", "vy", "wz", "neck_pitch", "head_pitch", "head_yaw", "head_roll")   # the order of cmd_range (include/odk.h)
NACC = 12
ENDED, STEPS, SAMPLES, FALLS, REWARD, SUM, SQERR = 0, 1, 2, 3, 4, 5, 8      # include/odk.h ODK_TRACK_*


def command_row(values: Sequence[float]) -> List[float]:
    """`--command vx vy wz [neck_pitch head_pitch head_yaw head_roll]` -> the 7 floats of a command row (head entries default to 0)."""
    v = [float(x) for x in values]
    if len(v) not in (3, 4, 5, 6, 7):
        raise ValueError(f"a command is vx vy wz [neck_pitch head_pitch head_yaw head_roll]: 3 to 7 numbers, got {len(v)}")
    return v + [0.0] * (7 - len(v))


def parse_grid(spec: str) -> List[List[float]]:
    """`vx=a:b:n,wz=c:d:m` -> the command rows of the grid: each named axis takes n values from a to b (numpy.linspace, ends included),
    axes not named stay 0, rows in itertools.product order of the axes as written (the last axis varies fastest)."""
    axes = []
    for part in spec.split(","):
        part = part.strip()
        if not part:
            continue
        name, _, rng = part.partition("=")
        name = name.strip()
        if name not in COMMAND_KEYS:
            raise ValueError(f"--grid: unknown axis {name!r} (one of {', '.join(COMMAND_KEYS)})")
        if any(name == a for a, _ in axes):
            raise ValueError(f"--grid: axis {name!r} given twice")
        bits = rng.split(":")
        if len(bits) != 3:
            raise ValueError(f"--grid: {part!r} is not {name}=start:stop:count")
        lo, hi, n = float(bits[0]), float(bits[1]), int(bits[2])
        if n < 1:
            raise ValueError(f"--grid: {part!r} needs a count >= 1")
        axes.append((name, np.linspace(lo, hi, n).tolist()))
    if not axes:
        raise ValueError("--grid: no axis given")
    rows = []
    for combo in itertools.product(*[vals for _, vals in axes]):
        row = [0.0] * 7
        for (name, _), v in zip(axes, combo):
            row[COMMAND_KEYS.index(name)] = float(v)
        rows.append(row)
    return rows


def command_blocks(commands: Sequence[Sequence[float]], envs_per_command: int) -> np.ndarray:
    """[len(commands) * envs_per_command, 7] float32: command c drives envs c * envs_per_command .. (c + 1) * envs_per_command - 1."""
    return np.repeat(np.asarray(commands, np.float32).reshape(-1, 7), int(envs_per_command), axis=0)


def reduce_tracking(acc: np.ndarray, commands: Sequence[Sequence[float]], envs_per_command: int) -> List[Dict]:
    """The per-command rows of the report from the accumulator ([nenv, 12], include/odk.h ODK_TRACK_*).  Velocity statistics are over
    the velocity samples of the block's envs (the steps of their first episode that did not end it), pooled; the fall rate is the
    share of the block's envs whose first episode ended by falling; the episode reward is the mean over envs of their first episode's
    reward sum."""
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
    net.load_state_dict(torch.load(path, map_location=device)["networks"])      # ppo/train.py save_checkpoint
    net.eval()
    return net


class Tracker:
    """One tracking run on a bound command buffer: `step()` = policy + env step + accumulator, captured as one graph."""

    def __init__(self, env, net, use_graph: bool = True):
        import torch
        self.env, self.net, self.torch = env, net, torch
        b = env.batch
        self.acc = torch.zeros(env.num_envs, NACC, device=b.obs.device)
        from .ppo.learner import fused_policy
        self.fp = fused_policy(net, env.num_envs)
        self.use_graph = use_graph
        self.graph = None

    def actions(self, obs):
        """The deterministic policy: tanh(loc) of the policy head (Evaluator._one_step)."""
        logits = self.fp(obs) if self.fp is not None else self.net.policy(self.net.norm_obs(obs))
        return self.torch.tanh(logits[..., : self.net.action_size]).contiguous()

    def _one_step(self):
        b = self.env.batch
        b.step(self.actions(b.obs))                 # Joystick.step without the State wrapper (nothing here reads it)
        b.tracking_accumulate(self.acc)

    def reset(self, seed: int):
        self.env.reset(int(seed))
        self.acc.zero_()
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


def run(args, out=sys.stdout) -> Dict:
    import torch
    commands = [command_row(c) for c in (args.command or [])]
    if args.grid:
        commands += parse_grid(args.grid)
    if not commands:
        raise SystemExit("give at least one --command or a --grid")
    E = int(args.envs_per_command)
    n = len(commands) * E
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    env = make_env(args, n, args.device)
    motion = getattr(env, "reference_motion", None)
    if motion is not None:
        print(motion.describe(), file=sys.stderr)      # stdout may carry the JSON report
    if hasattr(env, "describe_head_joints"):
        print(env.describe_head_joints(), file=sys.stderr)
    net = load_networks(args.checkpoint, env, dev)
    cmd = torch.from_numpy(command_blocks(commands, E)).to(dev)
    env.set_commands(cmd)
    tr = Tracker(env, net)
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
                obs_hist[t].copy_(env.batch.obs[0])          # env 0's observation, stream-ordered after the step
            if save_qpos_path:
                qpos_hist.append(env.batch.get_state()[0][0].copy())
        acc = tr.acc.cpu().numpy()
    rows = reduce_tracking(acc, commands, E)
    settings = dict(checkpoint=args.checkpoint, env=args.env, task=args.task, xml=args.xml, cone=args.cone,
                    hfield_up_normals_only=bool(args.hfield_up_normals_only), envs_per_command=E, episode_length=T, seed=int(args.seed),
                    num_envs=n, dt=float(env.dt), policy="deterministic tanh(loc)", fused_policy=tr.fp is not None, graph=tr.graph is not None,
                    reference_motion=getattr(args, "reference_motion", None), reference_motion_sha256=motion.sha256 if motion is not None else None)
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
    p.add_argument("--envs_per_command", type=int, default=128)
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
