"""The env step of two robots that are not the duck, bit for bit, against a recording made with the commit BEFORE the model's
launch-invariant values left the substep's path (profiles/load_waits).

That change only moves where integers and constants of the model come from -- packed words read once per launch, a shared LDS table,
per-lane packed records of the subtree fold -- so no output may change by one bit.  tests/test_gpu_step_bits.py holds the duck's three
tasks to that; this file adds the shapes whose tables differ most from the duck's: tests/assets/biped12.xml (chains of six, 16 bodies,
contact wrenches in floats of their own) and tests/assets/tail_biped.xml (a third chain, 19 bodies, equality code compiled in).  Both run
the plane-floor step kernel at 32 lanes per env: 8 envs, 6 env steps, observation noise, pushes and auto-reset on, actions seeded on the
host (numpy's PCG64: the same inputs on every machine).  The recordings tests/golden/hot_bits_<robot>.npz are the PARENT commit's outputs
-- never the code under test --: the raw uint32 views of obs, priv, reward, done, truncation, metrics, qpos and qvel of every step.
Every comparison is np.array_equal on integers.

Regenerate (only ever from a build of the commit the change is measured against):
    ODK_LIB=/path/to/parent/libodk.so python tests/test_gpu_hot_constants.py --write
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROBOTS = ["biped12", "tail_biped"]
N_ENVS, N_STEPS = 8, 6
ARRAYS = ("obs", "priv", "reward", "done", "truncation", "metrics", "qpos", "qvel")


def run_robot(robot):
    """The recorded run on the loaded library: {name: uint32 array [N_STEPS, ...]}"""
    import torch
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model
    model = Model.from_xml(os.path.join(ROOT, "tests", "assets", robot + ".xml"), sim_dt=0.002)
    cfg = engine.default_config()
    cfg.use_imitation = 0                                                  # (a robot that is not the duck has no reference motion)
    cfg.noise_level = 1.0
    cfg.push_enable = 1.0
    cfg.push_interval_range[0] = 0.02; cfg.push_interval_range[1] = 0.06   # a push every 1 .. 3 env steps
    cfg.episode_length = 4                                                 # truncation and auto-reset inside the run
    cfg.autoreset = 1
    cfg.lanes_per_env = 32
    acts = np.random.Generator(np.random.PCG64(23)).uniform(-1.0, 1.0, (N_STEPS, N_ENVS, model.nu)).astype(np.float32)
    b = engine.Batch(model, N_ENVS, cfg)
    rec = {k: [] for k in ARRAYS}
    try:
        assert b.lanes_per_env == 32, (robot, b.lanes_per_env)
        b.reset(seed=7)
        for t in range(N_STEPS):
            b.step(torch.from_numpy(acts[t]).to("cuda:0"))
            torch.cuda.synchronize()
            qpos, qvel, _ = b.get_state()
            out = {k: getattr(b, k).cpu().numpy() for k in ("obs", "priv", "reward", "done", "truncation", "metrics")}
            out.update(qpos=qpos, qvel=qvel)
            for k in ARRAYS:
                rec[k].append(np.ascontiguousarray(out[k], np.float32).view(np.uint32).copy())
        return {k: np.stack(v) for k, v in rec.items()}
    finally:
        b.close()


@pytest.mark.parametrize("robot", ROBOTS)
def test_robot_step_outputs_equal_the_parent_recording(robot):
    gold = np.load(os.path.join(GOLDEN, f"hot_bits_{robot}.npz"))
    got = run_robot(robot)
    assert sorted(gold.files) == sorted(got)
    # the recorded run did meet what it is there for: truncations with auto-reset, finite outputs, feet on the floor (contact rows at work)
    assert gold["truncation"].view(np.float32).sum() > 0 and np.isfinite(gold["qpos"].view(np.float32)).all() and np.isfinite(gold["obs"].view(np.float32)).all()
    bad = []
    for k in sorted(gold.files):
        g, x = gold[k], got[k]
        assert g.dtype == np.uint32 and x.dtype == np.uint32 and g.shape == x.shape, (robot, k)
        if not np.array_equal(g, x):
            bad.append((k, int(np.argwhere(g != x)[0][0]), int((g != x).sum())))
    assert not bad, f"{robot}: (array, first differing step, differing words) {bad}"


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit(__doc__)
    sys.path.insert(0, ROOT)
    os.makedirs(GOLDEN, exist_ok=True)
    for robot in ROBOTS:
        r = run_robot(robot)
        path = os.path.join(GOLDEN, f"hot_bits_{robot}.npz")
        np.savez_compressed(path, **r)
        print(path, os.path.getsize(path), "bytes; done", float(r["done"].view(np.float32).sum()), "trunc", float(r["truncation"].view(np.float32).sum()))
