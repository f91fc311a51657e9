"""The env step of the duck where the other bit recordings do not reach, bit for bit, against a recording made with the commit BEFORE
the selects left the line search (profiles/selects).

That change removes instructions that chose nothing -- the zero-divisor guard of the line search's Newton step, and the third of the
three divisors a pass prepared -- so no output may change by one bit.  tests/test_gpu_step_bits.py and tests/test_gpu_hot_constants.py
hold the three duck tasks, 64 lanes, biped12 and tail_biped to that on states a reset produces.  This file adds

  (a) `cone`: the elliptic-cone instantiation of the duck's kernels (flat_terrain with opt_cone = 1): 16 envs, 10 env steps;
  (b) `placed`: flat_terrain from hand-placed states that force the rare sides of the selects: 16 envs, 6 env steps from
        envs  0 ..  3  feet overlapping (right hip roll far inwards): the foot-foot slot and the virtual-tree Hessian run,
        envs  4 ..  7  joints beyond their limits (limit rows active),
        envs  8 .. 11  joint velocities of 20 rad/s, signs alternating: friction-loss rows in both linear zones,
        envs 12 .. 13  the reset pose at rest (in the recording their search stops on a bracket that no longer moves; the gradient test ends the
                       search of envs 2, 6, 10 and 11: cov_ls_gradient below),
        envs 14 .. 15  the robot half a metre up: no foot contact.

Both with observation noise, pushes and auto-reset on, actions seeded on the host (numpy's PCG64).  The recordings
tests/golden/select_bits_<case>.npz are the PARENT commit's outputs -- never the code under test --: the raw uint32 views of obs, priv,
reward, done, truncation, metrics, qpos and qvel of every step.  Every comparison is np.array_equal on integers.

Coverage of (b) is decided when the recording is made, on the CPU with the oracle (one forward pass from each placed state), and stored
next to the outputs as cov_* (one flag per env); the test asserts from those arrays that every situation occurs in at least two envs and
that at least one env has no foot contact.  The flags are specific to what was placed (the reset pose itself has a knee past its range and,
at rest, every friction-loss row in a linear zone):
  cov_footfoot        a foot-foot candidate penetrates;
  cov_limit           a limit row is active that is NOT active in the unplaced pose (env 12);
  cov_fl_both_zones   among the joints given a velocity, rows sit in the zone opposing their velocity on BOTH sides (+loss and -loss), at least
                      one of them in another zone than in the unplaced pose;
  cov_ls_gradient     the line search ends before its pass limit, and with the gradient test switched off (the same model with
                      ls_tolerance = 0, so gtol = 0) it runs more passes: the gradient test is what ended it, not a bracket that stopped moving.
The test also asserts that the envs without a placed joint lack cov_limit and those without a placed velocity lack cov_fl_both_zones.

Regenerate (only ever from a build of the commit the change is measured against):
    ODK_LIB=/path/to/parent/libodk.so python tests/test_gpu_select_bits.py --write
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"cone": 10, "placed": 6}      # case: env steps
N_ENVS = 16
ARRAYS = ("obs", "priv", "reward", "done", "truncation", "metrics", "qpos", "qvel")
COVERAGE = ("cov_footfoot", "cov_limit", "cov_fl_both_zones", "cov_ls_gradient")
UNPLACED = 12                         # an env that keeps the reset pose at rest
R_HIP_ROLL, L_HIP_YAW, L_HIP_ROLL, L_KNEE, HEAD_PITCH, R_KNEE = 10, 0, 1, 3, 6, 12      # joint numbers behind the free joint


def placed_states(qpos, qvel):
    """The 16 hand-placed states, from env 0's state after the reset (every env starts from the same pose: what differs is placed here)"""
    q = np.repeat(qpos[:1], N_ENVS, axis=0).copy(); v = np.zeros((N_ENVS, qvel.shape[1]), np.float32)
    j = lambda k: 7 + k
    q[0, j(R_HIP_ROLL)] = -0.9; q[1, j(R_HIP_ROLL)] = -1.0
    q[2, j(R_HIP_ROLL)] = -1.2; q[2, j(L_HIP_YAW)] = 0.6
    q[3, j(R_HIP_ROLL)] = -1.2; q[3, j(L_HIP_YAW)] = 0.9
    q[4, j(L_HIP_ROLL)] = 0.7
    q[5, j(R_KNEE)] = 1.8; q[5, j(HEAD_PITCH)] = -1.0
    q[6, j(L_KNEE)] = 1.8
    q[7, j(L_HIP_ROLL)] = -0.6; q[7, j(R_KNEE)] = -1.8; q[7, j(HEAD_PITCH)] = 1.3
    sign = np.where(np.arange(v.shape[1] - 6) % 2, 1.0, -1.0).astype(np.float32)
    v[8, 6:] = 20.0 * sign; v[9, 6:] = -20.0 * sign; v[10, 6:] = 12.0 * sign; v[11, 6:] = -12.0 * sign
    q[14, 2] += 0.5; q[15, 2] += 0.5
    return q, v


def run_case(case):
    """The recorded run on the loaded library: {name: uint32 array [steps, ...]}, and for `placed` the states it started from"""
    import torch
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    model = load_task_model("flat_terrain")
    if case == "cone":
        model = Model({**model.a, "opt_cone": np.array([1], np.int32)})
    cfg = engine.default_config()
    cfg.noise_level = 1.0
    cfg.push_enable = 1.0
    cfg.push_interval_range[0] = 0.02; cfg.push_interval_range[1] = 0.06   # a push every 1 .. 3 env steps
    cfg.episode_length = 4                                                 # truncation and auto-reset inside the run
    cfg.autoreset = 1
    cfg.lanes_per_env = 32
    steps = CASES[case]
    acts = np.random.Generator(np.random.PCG64(31)).uniform(-1.0, 1.0, (steps, N_ENVS, model.nu)).astype(np.float32)
    b = engine.Batch(model, N_ENVS, cfg)
    rec = {k: [] for k in ARRAYS}
    start = None
    try:
        assert b.lanes_per_env == 32, (case, b.lanes_per_env)
        b.reset(seed=7)
        if case == "placed":
            qpos, qvel, _ = b.get_state()
            start = placed_states(qpos, qvel)
            b.set_state(qpos=start[0], qvel=start[1], warm=np.zeros_like(start[1]))
        for t in range(steps):
            b.step(torch.from_numpy(acts[t]).to("cuda:0"))
            torch.cuda.synchronize()
            qpos, qvel, _ = b.get_state()
            out = {k: getattr(b, k).cpu().numpy() for k in ("obs", "priv", "reward", "done", "truncation", "metrics")}
            out.update(qpos=qpos, qvel=qvel)
            for k in ARRAYS:
                rec[k].append(np.ascontiguousarray(out[k], np.float32).view(np.uint32).copy())
        return {k: np.stack(v) for k, v in rec.items()}, start
    finally:
        b.close()


def oracle_coverage(start):
    """One oracle forward pass from each placed state: {cov_*: uint32[N_ENVS]} (and cov_no_foot_contact)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    model = load_task_model("flat_terrain")
    no_gtol = Model({**model.a, "opt_ls_tolerance": np.zeros_like(model.a["opt_ls_tolerance"])})      # gtol = 0: the gradient test never fires
    prm = O.OraclePRM(engine.load_prm())
    ls_limit = int(np.asarray(model.a["opt_ls_iterations"]).ravel()[0])

    def forward(mod):
        om = O.OracleModel(mod.blob()); env = O.OracleEnv(om, prm); env.reset(7, 0)
        d = env.data
        out = []
        for e in range(N_ENVS):
            d["qpos"][:model.nq] = start[0][e]; d["qvel"][:model.nv] = start[1][e]; d["qacc_warmstart"][:model.nv] = 0
            d.forward()
            ne, nf, nl = d.i("ne"), d.i("nf"), d.i("nl")
            force = np.array(d["efc_force"][ne:ne + nf]); loss = np.array(d["efc_frictionloss"][ne:ne + nf])
            out.append(dict(dist=np.array(d["contact_dist"][:12]),                      # 2 x 4 foot-floor candidates, then 4 foot-foot
                            limit=np.array(d["efc_pos"][ne + nf:ne + nf + nl]) < 0,     # one row per limited joint
                            zone=(force >= loss).astype(int) - (force <= -loss).astype(int),      # one friction-loss row per joint dof: +1 / -1 linear zones
                            iters=d.i("ls_iters")))
        return out
    res, res0 = forward(model), forward(no_gtol)
    base = res[UNPLACED]
    cov = {k: np.zeros(N_ENVS, np.uint32) for k in COVERAGE + ("cov_no_foot_contact",)}
    for e in range(N_ENVS):
        r = res[e]
        vel = np.sign(start[1][e][6:6 + len(r["zone"])]).astype(int)
        opposing = (vel != 0) & (r["zone"] == -vel)
        cov["cov_footfoot"][e] = (r["dist"][8:12] < 0).any()
        cov["cov_limit"][e] = (r["limit"] & ~base["limit"]).any()
        cov["cov_fl_both_zones"][e] = (opposing & (r["zone"] > 0)).any() and (opposing & (r["zone"] < 0)).any() and (opposing & (r["zone"] != base["zone"])).any()
        cov["cov_ls_gradient"][e] = r["iters"] < ls_limit and res0[e]["iters"] > r["iters"]
        cov["cov_no_foot_contact"][e] = (r["dist"][:8] > 0).all()
    return cov


@pytest.mark.parametrize("case", list(CASES))
def test_step_outputs_equal_the_parent_recording(case):
    gold = np.load(os.path.join(GOLDEN, f"select_bits_{case}.npz"))
    got, _ = run_case(case)
    assert sorted(k for k in gold.files if not k.startswith("cov_")) == sorted(got)
    assert gold["truncation"].view(np.float32).sum() > 0 and np.isfinite(gold["obs"].view(np.float32)).all()
    if case == "placed":      # the recorded run did meet the situations it is there for (flags of the oracle, stored when it was recorded)
        for k in COVERAGE:
            assert int(gold[k].sum()) >= 2, (k, gold[k])
        assert int(gold["cov_no_foot_contact"].sum()) >= 1
        assert not gold["cov_limit"][8:].any() and not gold["cov_fl_both_zones"][:8].any() and not gold["cov_fl_both_zones"][12:].any()
    bad = []
    for k in sorted(got):
        g, x = gold[k], got[k]
        assert g.dtype == np.uint32 and x.dtype == np.uint32 and g.shape == x.shape, (case, k)
        if not np.array_equal(g, x):
            bad.append((k, int(np.argwhere(g != x)[0][0]), int((g != x).sum())))
    assert not bad, f"{case}: (array, first differing step, differing words) {bad}"


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit(__doc__)
    sys.path.insert(0, ROOT)
    os.makedirs(GOLDEN, exist_ok=True)
    for case in CASES:
        r, start = run_case(case)
        if start is not None:
            r.update(oracle_coverage(start))
            print({k: v.tolist() for k, v in r.items() if k.startswith("cov_")})
        path = os.path.join(GOLDEN, f"select_bits_{case}.npz")
        np.savez_compressed(path, **r)
        print(path, os.path.getsize(path), "bytes; done", float(r["done"].view(np.float32).sum()), "trunc", float(r["truncation"].view(np.float32).sum()),
              "finite", bool(np.isfinite(r["obs"].view(np.float32)).all()))
