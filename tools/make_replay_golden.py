#!/usr/bin/env python3
"""tests/golden/replay_oracle_log.npz: a 61-row observation log (60 control steps of replay.excitation) that the float64 oracle
(oracle.OracleEnv, flat_terrain) produces on the plant kp x 0.8, frictionloss x 1.5, delay 0, from the home keyframe at rest with noise and
pushes off -- the independent implementation that tests/test_gpu_replay.py fits with the GPU kernels.  The rows are in the reference's
layout (what `replay.read_log` reads from an .npz).

    python tools/make_replay_golden.py            # writes the fixture
    python tools/make_replay_golden.py --sweep    # the CPU feasibility study: replays the log of (0.8, 1.5, delay 1) over the grid of the
                                                  # GPU self-consistency test with the oracle alone and prints every cell

`oracle_log` / `oracle_scores` are what tests/test_replay_host.py re-generates the fixture with."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

TASK, STEPS, KP, FRICTIONLOSS = "flat_terrain", 60, 0.8, 1.5
OUT = os.path.join(ROOT, "tests", "golden", "replay_oracle_log.npz")


def oracle_env(O, task=TASK, kp=1.0, frictionloss=1.0, armature=1.0, mass=1.0):
    """An oracle env on the scaled plant: the model's values times the scale, rounded to float32 once as Batch.set_param rounds them."""
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    model = load_task_model(task)
    om = O.OracleModel(model.blob())
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    nu = om.nu
    g = om.f["actuator_gainprm0"]
    new = f32(g * kp)
    om.f["actuator_biasprm"].reshape(nu, 3)[:, 1] = -new
    g[:] = new
    for name, s in (("dof_frictionloss", frictionloss), ("dof_armature", armature), ("body_mass", mass)):
        v = om.f[name]
        v[:] = f32(v * s)
    env = O.OracleEnv(om, O.OraclePRM(engine.load_prm()))
    env.cfg["noise_level"][:] = 0.0
    env.cfg["push_enable"][:] = 0.0
    env.cfg["episode_length"][:] = 100000
    return env, model


def oracle_replay(O, actions, delay=0, **plant):
    """The rows [len(actions) + 1, nobs] float32 of `actions` run open-loop on the oracle from replay.record's start, and whether the robot
    fell.  The oracle draws its action delay; a fixed one is imposed from outside: the ring is filled with the action `delay` steps old
    before every step, so whichever row the draw picks drives the motors, and the row's last_act is put back to the action given."""
    from open_duck_playground_amd import replay
    env, model = oracle_env(O, **plant)
    nu, nq, nv = model.nu, model.nq, model.nv
    f = replay.obs_fields(nu)
    env.reset(0, 0)
    key_ctrl = np.asarray(model.a["key_ctrl"], np.float32).astype(np.float64).reshape(-1)[:nu]
    trn = np.asarray(model.a["actuator_trnid"]).reshape(nu, -1)[:, 0]
    qadr = np.asarray(model.a["jnt_qposadr"])[trn]
    qpos = np.array(model.a["key_qpos"], np.float64).reshape(-1)[:nq].astype(np.float32).astype(np.float64)
    qpos[7:] = 0.0
    qpos[qadr] = key_ctrl
    d = env.data
    d["qpos"][:nq] = qpos; d["qvel"][:nv] = 0.0; d["qacc_warmstart"][:nv] = 0.0
    for k in ("last_act", "last_last_act", "last_last_last_act", "action_history", "command"):
        env[k][:] = 0.0
    env["motor_targets"][:nu] = key_ctrl
    env.ints("step")[0] = 0
    rows = np.zeros((len(actions) + 1, replay.obs_width(nu)), np.float32)
    rows[0, f["motor_targets"]:f["motor_targets"] + nu] = key_ctrl
    fell = False
    for k, a in enumerate(np.asarray(actions, np.float64)):
        drive = actions[k - delay].astype(np.float64) if k >= delay else np.zeros(nu)
        h = env["action_history"]
        h[0:nu] = drive; h[nu:2 * nu] = drive
        env.step(drive)
        fell = fell or env["done"][0] != 0
        rows[k + 1] = env["obs"][:rows.shape[1]]
        rows[k + 1, f["last_act"]:f["last_act"] + nu] = a
    return rows, bool(fell)


def oracle_log(O):
    """The fixture's rows."""
    from open_duck_playground_amd import replay
    rows, fell = oracle_replay(O, replay.excitation(14, STEPS, 0), kp=KP, frictionloss=FRICTIONLOSS)
    assert not fell
    return rows


def position_score(rows, log, nu=14):
    """Mean squared joint-position residual of replayed rows against a log's, rad^2 (float64)."""
    from open_duck_playground_amd import replay
    f = replay.obs_fields(nu)
    d = rows[1:, f["pos"]:f["pos"] + nu].astype(np.float64) - log[1:, f["pos"]:f["pos"] + nu].astype(np.float64)
    return float((d * d).mean())


def sweep(O):
    from open_duck_playground_amd import replay
    acts = replay.excitation(14, STEPS, 0)
    log, fell = oracle_replay(O, acts, delay=1, kp=KP, frictionloss=FRICTIONLOSS)
    print("log: kp 0.8, frictionloss 1.5, delay 1; fell:", fell)
    for kp in np.linspace(0.6, 1.0, 5):
        for fl in np.linspace(0.5, 2.0, 4):
            for dl in (0, 1, 2):
                rows, fell = oracle_replay(O, acts, delay=dl, kp=float(kp), frictionloss=float(fl))
                print(f"kp {kp:.2f} frictionloss {fl:.2f} delay {dl}: score {position_score(rows, log):.3e}{'  FELL' if fell else ''}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import oracle as O
    O.build()
    if args.sweep:
        sweep(O)
        return
    rows = oracle_log(O)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, obs=rows)
    print(f"{OUT}: {rows.shape}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
