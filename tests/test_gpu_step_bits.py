"""The env step's outputs, bit for bit, against a recording made with the commit BEFORE the substep-diet change (profiles/substep_diet).

The instruction-count work on the env step kernels (fused final DPP stages, joint slots at compile time) may not change one bit of what a
caller gets.  The recordings under tests/golden/step_bits_<case>.npz are the PARENT commit's outputs -- never the code under test -- for the
three duck tasks at 32 lanes per env and the two flat tasks at 64 lanes: 64 envs, 20 env steps, observation noise, pushes and auto-reset on,
seeded random actions (numpy's PCG64 on the host, so the inputs are the same on every machine).

Per step the recording holds the raw uint32 views of reward, done, truncation, metrics, qpos and qvel.  obs and priv (101 + 212 floats per
env and step; the recordings would be 6 MB, and a committed file stays far below 1 MiB) are held as two independent 32-bit
multiply-xorshift digests per env row and step over the row's uint32 view, plus the raw arrays of the last step: a changed bit in any row of
any step changes that row's digests (a miss needs a simultaneous collision of both, 2^-64).  Every comparison is np.array_equal on integers.

The fifth recording, flat_terrain_backlash at 64 lanes (step_bits_flat_terrain_backlash_lanes64.npz), was added with the tests that hold the
64-lane kernels to the oracle (profiles/lanes64): it is the output of the commit before THAT change, which edited no kernel, so it is this
library's own output at that point, there for later changes to be measured against.  It is the size of the 32-lane recording of the same model
(0.4 MB).

Regenerate (only ever from a build of the commit the change is measured against); `--case` names the recordings to write (file name without
`step_bits_` and `.npz`, repeatable) and leaves the others untouched, without it all are rewritten:
    ODK_LIB=/path/to/parent/libodk.so python tests/test_gpu_step_bits.py --write [--case flat_terrain_backlash_lanes64]
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("flat_terrain", 0), ("flat_terrain_backlash", 0), ("rough_terrain_backlash", 0), ("flat_terrain", 64), ("flat_terrain_backlash", 64)]
N_ENVS, N_STEPS = 64, 20
RAW = ("reward", "done", "truncation", "metrics", "qpos", "qvel")
DIGESTED = ("obs", "priv")


def _case_name(task, lanes):
    return task + (f"_lanes{lanes}" if lanes else "")


def _digest(rows_u32):
    """[n, k] uint32 -> [n, 2] uint32: two multiply-xorshift hashes of each row (position dependent, different odd multipliers)."""
    out = np.empty((rows_u32.shape[0], 2), np.uint32)
    x = rows_u32.astype(np.uint64)
    for j, (mul, seed) in enumerate(((0x9E3779B1, 0x85EBCA77), (0xC2B2AE3D, 0x27D4EB2F))):
        h = np.full(x.shape[0], seed, np.uint64)
        for c in range(x.shape[1]):
            h = ((h ^ x[:, c]) * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
            h ^= h >> np.uint64(15)
        out[:, j] = h.astype(np.uint32)
    return out


def run_case(task, lanes):
    """The recorded run on the loaded library: {name: uint32 array}, per-step arrays stacked on axis 0."""
    import torch
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    model = load_task_model(task)
    cfg = engine.default_config()
    cfg.noise_level = 1.0
    cfg.push_enable = 1.0
    cfg.push_interval_range[0] = 0.1; cfg.push_interval_range[1] = 0.3      # a push every 5 .. 15 env steps
    cfg.episode_length = 12                                                # truncation and auto-reset inside the run
    cfg.autoreset = 1
    cfg.lanes_per_env = lanes
    acts = np.random.Generator(np.random.PCG64(20)).uniform(-1.0, 1.0, (N_STEPS, N_ENVS, model.nu)).astype(np.float32)
    b = engine.Batch(model, N_ENVS, cfg)
    rec = {k: [] for k in RAW + tuple(k + "_digest" for k in DIGESTED)}
    try:
        assert b.lanes_per_env == (lanes or 32), (task, lanes, b.lanes_per_env)
        b.reset(seed=5)
        for t in range(N_STEPS):
            b.step(torch.from_numpy(acts[t]).to("cuda:0"))
            torch.cuda.synchronize()
            qpos, qvel, _ = b.get_state()
            out = {k: getattr(b, k).cpu().numpy() for k in ("obs", "priv", "reward", "done", "truncation", "metrics")}
            out.update(qpos=qpos, qvel=qvel)
            for k in RAW:
                rec[k].append(np.ascontiguousarray(out[k], np.float32).view(np.uint32).copy())
            for k in DIGESTED:
                rec[k + "_digest"].append(_digest(np.ascontiguousarray(out[k], np.float32).view(np.uint32).reshape(N_ENVS, -1)))
        res = {k: np.stack(v) for k, v in rec.items()}
        for k in DIGESTED:
            res[k + "_last"] = np.ascontiguousarray(out[k], np.float32).view(np.uint32).copy()
        return res
    finally:
        b.close()


@pytest.mark.parametrize("task,lanes", CASES)
def test_step_outputs_equal_the_parent_recording(task, lanes):
    gold = np.load(os.path.join(GOLDEN, f"step_bits_{_case_name(task, lanes)}.npz"))
    got = run_case(task, lanes)
    assert sorted(gold.files) == sorted(got)
    # the recorded run did meet what it is there for: terminations with auto-reset, truncations, finite outputs
    done = gold["done"].view(np.float32)
    assert done.sum() > 0 and gold["truncation"].view(np.float32).sum() > 0 and np.isfinite(gold["qpos"].view(np.float32)).all()
    bad = []
    for k in sorted(gold.files):
        g, x = gold[k], got[k]
        assert g.dtype == np.uint32 and x.dtype == np.uint32 and g.shape == x.shape, (task, lanes, k)
        if not np.array_equal(g, x):
            step = N_STEPS - 1 if k.endswith("_last") else int(np.argwhere(g != x)[0][0])
            bad.append((k, step, int((g != x).sum())))
    assert not bad, f"{task} lanes={lanes}: (array, first differing step, differing words) {bad}"


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit(__doc__)
    sys.path.insert(0, ROOT)
    os.makedirs(GOLDEN, exist_ok=True)
    only = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--case"]
    unknown = sorted(set(only) - {_case_name(*c) for c in CASES})
    if unknown or sys.argv[-1] == "--case":
        raise SystemExit(f"--case takes one of {[_case_name(*c) for c in CASES]}, got {unknown}")
    for task, lanes in CASES:
        if only and _case_name(task, lanes) not in only:
            continue
        r = run_case(task, lanes)
        path = os.path.join(GOLDEN, f"step_bits_{_case_name(task, lanes)}.npz")
        np.savez_compressed(path, **r)
        print(path, os.path.getsize(path), "bytes; done", float(r["done"].view(np.float32).sum()), "trunc", float(r["truncation"].view(np.float32).sum()))
