"""Generates tests/golden/reward_library.npz by IMPORTING the reference's numpy reward library in the build
container (it cannot travel to the GPU box).  Data only: inputs + expected outputs of the twelve library terms
the step kernel computes (include/odk.h odk_xterm; README "Reward library").

    python tools/make_reward_library_golden.py [/root/reference]

Source (reference, imported not copied): playground/common/rewards_numpy.py.  Per term `<k>`: the inputs
`<k>/<arg>` ([N, ...] float32, one call per row) and `<k>/out` [N].  The rows cover ties (values on a limit,
on the target, on an air-time threshold), zero commands, both sides of the air-time clip and first_contact
on and off.
"""
import os
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
os.makedirs(OUT, exist_ok=True)

from playground.common import rewards_numpy as R  # noqa: E402

rng = np.random.default_rng(20261015)
N, NU = 64, 14
f32 = np.float32
u = lambda lo, hi, *shape: rng.uniform(lo, hi, (N,) + shape).astype(f32)
out = {}


def put(key, fn, **inputs):
    for k, v in inputs.items():
        out[f"{key}/{k}"] = np.asarray(v, f32)
    out[f"{key}/out"] = np.array([fn(*[v[i] for v in inputs.values()]) for i in range(N)], f32)


put("lin_vel_z", R.cost_lin_vel_z, global_linvel=u(-2, 2, 3))
put("ang_vel_xy", R.cost_ang_vel_xy, global_angvel=u(-4, 4, 3))
up = u(-1, 1, 3); up[:4] = [0, 0, 1]      # upright rows
put("orientation", R.cost_orientation, upvector=up)
z = u(0.05, 0.4); tgt = np.full(N, 0.2, f32); z[:4] = tgt[:4]     # ties: on the target
put("base_height", R.cost_base_height, base_height=z, base_height_target=tgt)
put("energy", R.cost_energy, qvel=u(-8, 8, NU), qfrc_actuator=u(-3, 3, NU))
lo, hi = u(-2, -0.2, NU), u(0.2, 2, NU)
q = u(-2.5, 2.5, NU); q[:4, :3] = lo[:4, :3]; q[:4, 3:6] = hi[:4, 3:6]     # ties: on a soft limit
put("joint_pos_limits", R.cost_joint_pos_limits, qpos=q, soft_lowers=lo, soft_uppers=hi)
put("termination", R.cost_termination, done=(rng.random(N) < 0.5).astype(f32))
d = u(-1, 1, NU); qp = u(-1.5, 1.5, NU); qp[:4] = d[:4]     # ties: at the default pose
put("pose", R.cost_pose, qpos=qp, default_pose=d, weights=u(0, 2, NU))
put("feet_slip", R.cost_feet_slip, contact=(rng.random((N, 2)) < 0.5).astype(f32), feet_vel=u(-1, 1, 2, 3))
fp = u(-0.5, 0.5, 2, 3); fp[..., 2] = u(0, 0.1, 2); mh = np.full(N, 0.03, f32); fp[:4, 0, 2] = mh[:4]   # ties: at max_foot_height
fv = u(-1, 1, 2, 3); fv[4:8] = 0                                                                     # still feet
put("feet_clearance", R.cost_feet_clearance, feet_vel=fv, foot_pos=fp, max_foot_height=mh)
pk = u(0, 0.08, 2); pk[:4, 0] = mh[:4]
put("feet_height", R.cost_feet_height, swing_peak=pk, first_contact=(rng.random((N, 2)) < 0.5).astype(f32), max_foot_height=mh)
air = u(0, 1.0, 2); air[:4, 0] = 0.1; air[4:8, 1] = 0.5          # ties on both thresholds; rows above 0.5 are clipped
cmd = u(-1, 1, 7); cmd[8:16, :3] = 0                             # zero move commands: no reward
cmd[16:20, :3] = [0.005, 0.005, 0.005]                           # norm below 0.01
fc = (rng.random((N, 2)) < 0.5).astype(f32); fc[:8] = 1          # first_contact on for the tie rows
put("feet_air_time", lambda a, f, c, lo_, hi_: R.reward_feet_air_time(a, f, c, lo_, hi_), air_time=air, first_contact=fc, commands=cmd,
    threshold_min=np.full(N, 0.1, f32), threshold_max=np.full(N, 0.5, f32))

path = os.path.join(OUT, "reward_library.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {len(out)} arrays")
