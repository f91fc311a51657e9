#!/usr/bin/env python3
"""The two measurements of profiles/replay/NOTES.md.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_replay_measure.py trace
        100 replayed steps of 8192 duck envs (flat_terrain): the stats file has log_apply_kernel and replay_kernel next to step_kernel
    python tools/gpu_replay_measure.py fit
        wall time of a 6-generation fit (1024 candidates) of a 500-row log recorded here on kp 0.8, frictionloss 1.5, delay 1"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_duck_playground_amd import replay      # noqa: E402


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "fit"
    import torch
    true = dict(replay.replay_plant(), kp=0.8, frictionloss=1.5, delay=1)
    if mode == "trace":
        rows = replay.record("flat_terrain", plant=true, steps=100)
        r = replay.Replayer(rows, "flat_terrain", "joystick", 8192)
        rng = np.random.default_rng(0)
        plants = {k: (rng.integers(0, 3, 8192) if k == "delay" else rng.uniform(0.7, 1.3, 8192)) for k in replay.PLANT_AXES}
        scores, lasted, _, _, _ = r.evaluate(plants)
        torch.cuda.synchronize()
        print(f"8192 envs x {r.nrow} steps: {int(lasted.sum())} lasted, best score {scores.min():.3e}")
        r.close()
        return
    rows = None
    for amplitude in (0.15, 0.1, 0.05, 0.02):      # the open-loop duck falls after about 110 steps of the 0.3 excitation: a long log needs a gentler one
        try:
            rows = replay.record("flat_terrain", plant=true, actions=replay.excitation(14, 499, 0) * np.float32(amplitude / 0.3))
            print(f"excitation amplitude {amplitude}: the robot stands for 499 steps")
            break
        except RuntimeError as err:
            print(f"excitation amplitude {amplitude}: {err}")
    if rows is None:
        return
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "log.npz")
    replay.write_log(path, rows)
    t0 = time.perf_counter()
    rep = replay.main(["--log", path, "--fit", "kp=0.5:1.5,frictionloss=0.3:3,armature=0.5:2,delay=0:2", "--output", os.path.join(tmp, "fit.json")])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"fit of {len(rows)} rows, 6 generations x 1024 candidates: {dt:.2f} s wall; best {rep['best_plant']} score {rep['best_score']:.3e} "
          f"fell_share {rep['fell_share']:.3f}")
    print("history:", [f"{h['best_score']:.2e}" for h in rep["score_history"]])
    print("hint:", rep["identifiability_hint"]["elite_mean"], rep["identifiability_hint"]["elite_std"], rep["identifiability_hint"]["delay_shares"])


if __name__ == "__main__":
    main()
