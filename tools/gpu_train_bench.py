"""Full-PPO throughput (BASELINE.json configs[2]): flat_terrain_backlash + domain randomisation, 8192 envs,
Appendix-G hyper-parameters; reports env-steps/s including the learner, and the rollout/learner split.
    python tools/gpu_train_bench.py [task] [iters] [--train_sensor SPEC] [--train_actuation SPEC] [--command_curriculum GRID]
With one of the first two flags (runner's) the rollout runs through a fault_training.FaultStage: three more launches per step; with the
third the commands come from a command_curriculum.CommandCurriculum: one more launch per step and one per training step."""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from open_duck_playground_amd import joystick
from open_duck_playground_amd.ppo import train as T
from open_duck_playground_amd.ppo.networks import PPONetworks

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("task", nargs="?", default="flat_terrain_backlash")
ap.add_argument("iters", nargs="?", type=int, default=5)
ap.add_argument("--train_sensor", action="append", default=[])
ap.add_argument("--train_actuation", action="append", default=[])
ap.add_argument("--command_curriculum", default=None)
ap.add_argument("--curriculum_allow_clipped_reference", action="store_true")
args = ap.parse_args()
task, iters = args.task, args.iters
flags = {k: v for k, v in (("train_sensor", args.train_sensor), ("train_actuation", args.train_actuation)) if v}
env = joystick.Joystick(task=task, num_envs=8192)
faults = None
if flags:
    from open_duck_playground_amd import fault_training
    faults = fault_training.FaultStage(env, fault_training.spec_from_args(args), seed=0)
curriculum = None
if args.command_curriculum:
    from open_duck_playground_amd import command_curriculum
    curriculum = command_curriculum.CommandCurriculum(env, command_curriculum.spec_from_args(args, env), seed=0)
env.randomize(np.random.default_rng(0))
cfg = T.ppo_config()
dev = env.batch.obs.device
torch.manual_seed(0)
net = PPONetworks(101, 212, 14).to(dev)
opt = torch.optim.Adam(net.parameters(), lr=cfg["learning_rate"], capturable=True)
learner = None
gen = torch.Generator(device=dev); gen.manual_seed(0)
state = env.reset(0)
if faults is not None:
    faults.reset()
if curriculum is not None:
    curriculum.reset(state)
tr = tl = 0.0
WARM = 2   # untimed: learner construction, library handles, selection file
for it in range(iters + WARM):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if curriculum is None:
        data, state = T.rollout(env, net, state, cfg["unroll_length"], gen, faults=faults)
    else:
        data, state = T.rollout(env, net, state, cfg["unroll_length"], gen, faults=faults, curriculum=curriculum)
        curriculum.update()
    torch.cuda.synchronize(); t1 = time.perf_counter()
    net.norm_obs.update(data["obs"]); net.norm_priv.update(data["priv"])
    if it == 0:
        learner = T.make_learner(net, data, cfg) if os.environ.get("ODK_EAGER_LEARNER") != "1" else None
    m = T.sgd_epoch(net, opt, data, cfg, gen, learner=learner)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    if it >= WARM:
        tr += t1 - t0; tl += t2 - t1
steps = iters * 8192 * cfg["unroll_length"]
print(json.dumps({"task": task, "iters": iters, "faults": None if faults is None else flags, "curriculum": args.command_curriculum, "rollout_ms_per_step": 1e3 * tr / (iters * cfg["unroll_length"]), "env_steps_per_s_total": steps / (tr + tl), "rollout_env_steps_per_s": steps / tr,
                  "rollout_s_per_iter": tr / iters, "learner_s_per_iter": tl / iters, "last_loss": float(m["total_loss"]),
                  "reward_per_step": float(data["reward"].mean())}))
