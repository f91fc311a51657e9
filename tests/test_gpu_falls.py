"""GPU checks of the fall recorder (odk_fall_accumulate / Batch.fall_accumulate) and of `track --falls`: every float of the accumulator
against a float32 numpy restatement, bit for bit -- on synthetic outputs with a known qpos per step (three robots: nq not a multiple of 16,
16 live actuator lanes; a partly idle last block; guard floats and guard rows), on a real rollout whose action sequence was chosen on the
CPU oracle so that envs fall early, fall late and survive, eager and from a captured graph -- then the report, the clips and the refusals.

One refusal of the C entry has no test: a model with more than 16 actuators.  No such model loads (MAXU = 16 in csrc/odk_model.h: the
loader refuses it by name), so no batch of one exists to hand to the call."""
import json

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

G = RC.HEADER         # include/odk.h's constants, by engine's names

f32 = np.float32


def restate(priv, done, trunc, qpos, cmd, nobs, nu, nq, limit, tol, ring, acc0):
    """odk_fall_accumulate followed by odk_tracking_accumulate's ENDED / STEPS bookkeeping, restated in float32: priv [T, n, npriv], done and
    trunc [T, n], qpos [T, n, nq] (the state each step left), cmd [T, n, 7] (the bound row each step left), limit [nu] or None, acc0 the
    accumulator as allocated (any guard floats in place, zeros where a row lives).  Returns (the accumulator after every step
    [T, *acc0.shape], STEPS [n], ENDED [n])."""
    T, n = done.shape
    A = np.array(acc0, f32)
    w = G.FALL_SAMPLE + nq
    ended, steps = np.zeros(n, bool), np.zeros(n, f32)
    lim = None if limit is None else np.asarray(limit, f32)
    snaps = []
    for t in range(T):
        for e in range(n):
            if ended[e]:
                continue
            R, st = A[e], steps[e]
            steps[e] += 1
            if done[t, e] != 0:
                if trunc[t, e] == 0:
                    R[G.FALL_FELL], R[G.FALL_STEP] = 1, st
                ended[e] = True
                continue
            Q, C = priv[t, e, nobs:], cmd[t, e]
            s = int(R[G.FALL_SAMPLES])
            S = R[G.FALL_HEAD + (s % ring) * w:][:w]
            S[G.FALL_S_STEP] = st
            S[G.FALL_S_UP:G.FALL_S_UP + 3], S[G.FALL_S_GYRO:G.FALL_S_GYRO + 3], S[G.FALL_S_LINVEL:G.FALL_S_LINVEL + 3] = Q[6:9], Q[0:3], Q[9:12]
            S[G.FALL_S_HEIGHT] = Q[15 + 2 * nu]
            S[G.FALL_S_CONTACT:G.FALL_S_CONTACT + 2] = Q[16 + 3 * nu:18 + 3 * nu]
            S[G.FALL_S_LIN_ERR] = RC.planar32(f32(Q[9] - C[0]), f32(Q[10] - C[1]))
            S[G.FALL_S_ANG_ERR] = np.abs(f32(Q[2] - C[2]))
            force = np.abs(Q[16 + 2 * nu:16 + 3 * nu])
            S[G.FALL_S_SAT] = 0 if lim is None else np.count_nonzero((lim > 0) & (force >= f32(0.99) * lim))
            S[G.FALL_SAMPLE:] = qpos[t, e]
            tilt = RC.planar32(Q[6], Q[7])
            R[G.FALL_SAMPLES] = s + 1
            R[G.FALL_TILT_PEAK] = max(R[G.FALL_TILT_PEAK], tilt)
            if tilt <= tol:
                R[G.FALL_LAST_UPRIGHT] = s + 1
                R[G.FALL_UPRIGHT_CONTACT:G.FALL_UPRIGHT_CONTACT + 2] = S[G.FALL_S_CONTACT:G.FALL_S_CONTACT + 2]
        snaps.append(A.copy())
    return np.stack(snaps), steps, ended


N_SYN, T_SYN, RING_SYN = 300, 11, 4
TOL_SYN = f32(0.3)
# first episodes by e % 8: running at the end | fall in step 0 | fall with `ring` samples | with ring + 1 | after two wraps (10 samples) |
# truncation in step 0 | truncation at step 6 | running at the end
END_AT = (T_SYN + 1, 0, RING_SYN, RING_SYN + 1, 10, 0, 6, T_SYN + 1)
TRUNCATED = (5, 6)
E_TIE = 7                 # runs to the end: exactly the tolerance is upright, one ulp above is not


def synthetic_inputs(nobs, npriv, nu, nq, limits):
    """The host half of the synthetic test, a function of the sizes alone: (priv [T, n, npriv], done, trunc [T, n], qpos [T, n, nq], cmd
    [n, 7], end_at [n], limit [nu] or None)."""
    n, T = N_SYN, T_SYN
    rng = np.random.default_rng(7 + nq)
    priv = rng.normal(0.0, 1.0, (T, n, npriv)).astype(f32)
    priv[:, :, nobs + 6:nobs + 8] *= f32(0.3)                                       # leans on both sides of the tolerance
    priv[:, :, nobs + 16 + 3 * nu:nobs + 18 + 3 * nu] = rng.integers(0, 2, (T, n, 2))
    priv[2, E_TIE, nobs + 6:nobs + 8] = (TOL_SYN, 0.0)
    priv[3, E_TIE, nobs + 6:nobs + 8] = (0.0, np.nextafter(TOL_SYN, f32(1)))
    priv[4:, E_TIE, nobs + 6] = 1.0
    qpos = rng.normal(0.0, 1.0, (T, n, nq)).astype(f32)
    cmd = rng.uniform(-0.3, 0.3, (n, 7)).astype(f32)
    end_at, done, trunc, _ = RC.first_episodes(rng, T, n, END_AT, TRUNCATED)
    limit = None
    if limits:
        limit = np.ones(nu, f32)
        limit[1], limit[2], limit[3], limit[4] = 0.0, 0.5, 100.0, -1.0             # never counted; saturates often; never reached; never counted
        fcol = nobs + 16 + 2 * nu
        priv[1, 0, fcol] = f32(0.99) * f32(1.0)                                    # exactly at the threshold: counted
        priv[1, 8, fcol] = -np.nextafter(f32(0.99) * f32(1.0), f32(0))             # one ulp under it: not counted
        priv[:, :, fcol + 1] = 50.0                                                # a large force on the actuator without a limit
    return priv, done, trunc, qpos, cmd, end_at, limit


@pytest.mark.parametrize("robot,nu,limits", [("flat_terrain", 14, "given"), ("flat_terrain_backlash", 14, None), ("biped_arms.xml", 16, "given")])
def test_every_float_equals_a_numpy_restatement_on_synthetic_rows(robot, nu, limits):
    """300 envs (19 blocks of 256 threads, the last one partly idle), ring 4, 11 steps of seeded random privileged rows written straight into
    the batch's outputs, a known qpos per step put in with set_state, no odk_step.  Launch order as track's: the fall recorder, then the
    tracking accumulator.  The accumulator is 3 floats wider than a row and 2 rows longer than the batch, filled with 9.0 there; after every
    step it equals the restatement as int32 everywhere, and the fall launch leaves the tracking accumulator's bits alone."""
    import torch
    n, T, ring, e_tie = N_SYN, T_SYN, RING_SYN, E_TIE
    env = RC.robot_env(robot, n)
    b = env.batch
    nobs, npriv, nq = b.nobs, b.npriv, int(b.model.nq)
    assert b.model.nu == nu and nobs + 18 + 3 * nu <= npriv
    if robot == "flat_terrain_backlash":
        assert nq > 21 and nq % 16 != 0          # more than one pass of the qpos copy, the last one partly idle
    rf = b.fall_row_floats(ring)
    assert rf == G.FALL_HEAD + ring * (G.FALL_SAMPLE + nq)
    priv, done, trunc, qpos, cmd, end_at, limit = synthetic_inputs(nobs, npriv, nu, nq, limits)
    acc0 = np.full((n + 2, rf + 3), 9.0, f32)
    acc0[:n, :rf] = 0.0
    want, steps, ended = restate(priv, done, trunc, qpos, np.broadcast_to(cmd, (T, n, 7)), nobs, nu, nq, limit, TOL_SYN, ring, acc0)

    big = torch.tensor(acc0, device="cuda")
    acc = big[:n]
    tacc = torch.zeros(n, G.TRACK_NACC, device="cuda")
    b.bind_commands(torch.tensor(cmd, device="cuda"))
    b.reward.zero_()
    lim_dev = None if limit is None else torch.tensor(limit, device="cuda")
    priv_d, done_d, trunc_d = (torch.tensor(x, device="cuda") for x in (priv, done, trunc))
    for t in range(T):
        b.set_state(qpos[t])
        b.priv.copy_(priv_d[t]); b.done.copy_(done_d[t]); b.truncation.copy_(trunc_d[t])      # what the env step would have left
        before = tacc.clone()
        b.fall_accumulate(acc, tacc, float(TOL_SYN), ring, lim_dev)
        assert torch.equal(tacc.view(torch.int32), before.view(torch.int32))
        b.tracking_accumulate(tacc)
        np.testing.assert_array_equal(big.cpu().numpy().view(np.int32), want[t].view(np.int32), err_msg=f"step {t}")
    got, tr = big.cpu().numpy(), tacc.cpu().numpy()
    np.testing.assert_array_equal(tr[:, G.TRACK_STEPS], steps)
    np.testing.assert_array_equal(tr[:, G.TRACK_ENDED] != 0, ended)
    np.testing.assert_array_equal(got[n:], 9.0)
    np.testing.assert_array_equal(got[:, rf:], 9.0)

    # the run covers what it claims to
    row = lambda e: got[e, :rf]
    assert {int(x) for x in got[:n, G.FALL_SAMPLES]} == {0, ring, ring + 1, 6, 10, T}
    for e in range(16):
        k, r = e % 8, row(e)
        assert r[G.FALL_SAMPLES] == min(end_at[e], T) and np.all(r[G.FALL_TILT_PEAK + 1:G.FALL_HEAD] == 0.0)
        assert r[G.FALL_FELL] == (end_at[e] < T and k not in TRUNCATED) and r[G.FALL_STEP] == (end_at[e] if r[G.FALL_FELL] else 0)
        if k in (1, 5):                                                            # ended in step 0: nothing but the fall's two slots
            assert np.all(np.delete(r, [G.FALL_FELL, G.FALL_STEP]) == 0.0)
        order = np.array([(s % ring) for s in range(max(int(r[G.FALL_SAMPLES]) - ring, 0), int(r[G.FALL_SAMPLES]))], np.int64)
        slots = r[G.FALL_HEAD:].reshape(ring, G.FALL_SAMPLE + nq)
        np.testing.assert_array_equal(slots[order, G.FALL_S_STEP], np.arange(max(int(r[G.FALL_SAMPLES]) - ring, 0), int(r[G.FALL_SAMPLES])))
        np.testing.assert_array_equal(slots[order, G.FALL_SAMPLE:], qpos[int(r[G.FALL_SAMPLES]) - len(order):int(r[G.FALL_SAMPLES]), e])
    tie = want[:, e_tie]
    assert tie[2, G.FALL_LAST_UPRIGHT] == 3 and tie[3, G.FALL_LAST_UPRIGHT] == 3 and tie[3, G.FALL_SAMPLES] == 4
    assert tie[-1, G.FALL_LAST_UPRIGHT] == 3 and tie[-1, G.FALL_TILT_PEAK] >= 1.0
    np.testing.assert_array_equal(tie[-1, G.FALL_UPRIGHT_CONTACT:G.FALL_UPRIGHT_CONTACT + 2], priv[2, e_tie, nobs + 16 + 3 * nu:nobs + 18 + 3 * nu])
    sat = got[:n, G.FALL_HEAD:rf].reshape(n, ring, G.FALL_SAMPLE + nq)[:, :, G.FALL_S_SAT]
    if limit is None:
        assert np.all(sat == 0.0)
    else:
        assert sat.max() >= 3 and want[1, 0, G.FALL_HEAD + (G.FALL_SAMPLE + nq) + G.FALL_S_SAT] >= 1 and np.all(sat == np.round(sat)) and sat.max() <= nu - 3
    lu = got[:n, G.FALL_LAST_UPRIGHT]
    assert (lu == 0).any() and (lu == got[:n, G.FALL_SAMPLES]).any() and ((lu > 0) & (lu < got[:n, G.FALL_SAMPLES])).any()
    b.bind_commands(None)
    b.close()


# ---- a real rollout.  The action sequence was chosen on the CPU oracle (oracle.OracleVecEnv, the same reset seed, config and prepared
# state): see test_a_real_rollout_eager_and_captured
ROLL_N, ROLL_T, ROLL_RING, ROLL_EPISODE, ROLL_SEED, ROLL_AMP = 64, 80, 8, 60, 1, 1.0
TIPPED = (0, 1, 2)


def _roll_actions(nu):
    """One sequence of uniform actions for all envs, scaled per env from 0 (env 0) to ROLL_AMP (the last env)."""
    seq = np.random.default_rng(ROLL_SEED).uniform(-1, 1, (ROLL_T, 1, nu)).astype(f32)
    return (seq * np.linspace(0.0, ROLL_AMP, ROLL_N, dtype=f32)[None, :, None]).astype(f32)


def _rollout(graph):
    import torch
    from open_duck_playground_amd import engine, track
    n, T, ring = ROLL_N, ROLL_T, ROLL_RING
    env = RC.robot_env("flat_terrain", n, config_overrides={"episode_length": ROLL_EPISODE})
    b = env.batch
    nq = int(b.model.nq)
    cmd = torch.tensor(np.tile(f32([0.1, 0, 0, 0, 0, 0, 0]), (n, 1)), device="cuda")
    b.bind_commands(cmd)
    env.reset(ROLL_SEED)
    torch.cuda.synchronize()
    qpos, qvel, _ = b.get_state()
    th = np.deg2rad(80.0)
    for e in TIPPED:                                  # in the air, pitched 80 degrees forward and turning on: past the horizontal within a few steps
        qpos[e, 2] += 0.1
        qpos[e, 3:7] = [np.cos(th / 2), 0.0, np.sin(th / 2), 0.0]
        qvel[e, 4] = 5.0
    b.set_state(qpos, qvel)
    acts = torch.tensor(_roll_actions(b.model.nu), device="cuda")
    act = torch.zeros(n, b.model.nu, device="cuda")
    limit = track.torque_limits(env.mj_model)
    lim_dev = torch.tensor(limit, device="cuda")
    tol = track.fall_tilt_tol(0.35)
    acc = torch.zeros(n, b.fall_row_floats(ring), device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")

    def one():
        b.step(act)
        b.fall_accumulate(acc, tacc, tol, ring, lim_dev)
        b.tracking_accumulate(tacc)

    hist, g = [], None
    with torch.no_grad():
        for t in range(T):
            act.copy_(acts[t])
            if not graph:
                one()
                torch.cuda.synchronize()
                hist.append((b.priv.cpu().numpy(), b.done.cpu().numpy(), b.truncation.cpu().numpy(), b.get_state()[0]))
            elif g is None:                           # Tracker.step's way: the warm-up on a side stream is the first step, the capture runs nothing
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    one()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    one()
            else:
                g.replay()
    torch.cuda.synchronize()
    out = dict(acc=acc.cpu().numpy(), tacc=tacc.cpu().numpy(), hist=hist, nobs=b.nobs, nu=b.model.nu, nq=nq, limit=limit, tol=tol,
               cmd=cmd.cpu().numpy())
    b.bind_commands(None)
    b.close()
    return out


def test_a_real_rollout_eager_and_captured():
    """64 duck envs, ring 8, 80 steps, episode_length 60, command 0.1 0 0.  Env e gets ROLL_AMP * e / 63 times one uniform(-1, 1) action
    sequence (numpy default_rng(1)); envs 0..2 start 0.1 m up, pitched 80 degrees forward with 5 rad/s of pitch rate.  On the CPU oracle
    (OracleVecEnv, reset seed 1, the same prepared state) this gives 36 first episodes that fall after more than 8 steps, 3 that fall within
    8 (the prepared ones, at step 1) and 25 that never fall (truncated at step 59): 4 / 1 / 4 are asked for here, each with a margin of
    more than two.  Every step's privileged rows, flags and qpos come to the host; the restatement over them has the accumulator's bits,
    and the same run replayed from a captured graph has them too."""
    e = _rollout(graph=False)
    priv, done, trunc, qpos = (np.stack([h[i] for h in e["hist"]]) for i in range(4))
    n, ring, nq = ROLL_N, ROLL_RING, e["nq"]
    acc0 = np.zeros_like(e["acc"])
    want, steps, ended = restate(priv, done, trunc, qpos, np.broadcast_to(e["cmd"], (ROLL_T, n, 7)), e["nobs"], e["nu"], nq, e["limit"], f32(e["tol"]), ring, acc0)
    got = e["acc"]
    fell, ns = got[:, G.FALL_FELL] != 0, got[:, G.FALL_SAMPLES]
    late, early, never = int((fell & (ns > ring)).sum()), int((fell & (ns < ring)).sum()), int((~fell).sum())
    print(f"falls after more than {ring} samples: {late}, with fewer: {early}, never fell: {never}; truncated: {int((ended & ~fell).sum())}")
    assert late >= 4 and early >= 1 and never >= 4, (late, early, never)
    np.testing.assert_array_equal(e["tacc"][:, G.TRACK_STEPS], steps)
    np.testing.assert_array_equal(got.view(np.int32), want[-1].view(np.int32))
    assert (ended & ~fell).any()                      # somebody was truncated: nothing written at that done step
    np.testing.assert_array_equal(got[fell, G.FALL_STEP], ns[fell])      # every step before the termination was a sample
    assert (got[:, G.FALL_HEAD:].reshape(n, ring, G.FALL_SAMPLE + nq)[:, :, G.FALL_S_SAT] > 0).any() and (got[:, G.FALL_LAST_UPRIGHT] > 0).any()
    g = _rollout(graph=True)
    np.testing.assert_array_equal(g["acc"].view(np.int32), got.view(np.int32))
    np.testing.assert_array_equal(g["tacc"].view(np.int32), e["tacc"].view(np.int32))


# ---- track --falls
def _run(track, monkeypatch, argv, eager=False):
    """RC.run_track recording, after every step, the step's privileged rows, flags, qpos and bound command rows."""
    def after_step(tr, _):
        b = tr.env.batch
        return RC.step_outputs(tr) + (b.get_state()[0], b.commands.cpu().numpy())
    return RC.run_track(track, monkeypatch, argv, eager, after_step=after_step)


TRACK_RING = 8


def _restate_run(track, rep, tr, hist):
    priv, done, trunc, qpos, cmd = (np.stack([h[i] for h in hist]) for i in range(5))
    b = tr.env.batch
    got = tr.fall_acc.cpu().numpy()
    st = rep["settings"]
    assert st["falls"] is True and st["fall_ring"] == TRACK_RING and st["fall_tilt"] == 0.35 and st["fall_tilt_tol"] == float(f32(np.sin(0.35)))
    assert got.shape == (st["num_envs"], G.FALL_HEAD + TRACK_RING * (G.FALL_SAMPLE + int(b.model.nq)))
    want, steps, ended = restate(priv, done, trunc, qpos, cmd, b.nobs, 14, int(b.model.nq), track.torque_limits(tr.env.mj_model), f32(st["fall_tilt_tol"]),
                                 TRACK_RING, np.zeros_like(got))
    np.testing.assert_array_equal(tr.acc.cpu().numpy()[:, G.TRACK_STEPS], steps)
    np.testing.assert_array_equal(got.view(np.int32), want[-1].view(np.int32))
    return want[-1], qpos, cmd


def _check_clips(path, want, qpos_hist, blocks, E, nq, keep):
    """The saved clips are the recorded qpos of those envs at those steps, bit for bit; `blocks`: the rows or cells, in order."""
    z = np.load(path)
    fell = want[:, G.FALL_FELL] != 0
    envs = [e for k in range(len(blocks)) for e in (k * E + np.flatnonzero(fell[k * E:(k + 1) * E])[:keep])]
    np.testing.assert_array_equal(z["env"], envs)
    assert z["qpos"].shape == (len(envs), TRACK_RING, nq) and z["qpos"].dtype == np.float32
    for i, e in enumerate(envs):
        m, t = int(z["valid"][i]), int(z["fall_step"][i])
        assert m == min(int(want[e, G.FALL_SAMPLES]), TRACK_RING) and t == want[e, G.FALL_STEP] == want[e, G.FALL_SAMPLES] and z["row"][i] == e // E
        np.testing.assert_array_equal(z["steps"][i], [-1] * (TRACK_RING - m) + list(range(t - m, t)))
        np.testing.assert_array_equal(z["qpos"][i, :TRACK_RING - m], 0.0)
        np.testing.assert_array_equal(z["qpos"][i, TRACK_RING - m:].view(np.int32), qpos_hist[t - m:t, e].view(np.int32))      # hist[s]: the state step s left
        np.testing.assert_array_equal(z["command"][i], f32(blocks[e // E]["command"]))
    return z


def test_track_falls_end_to_end(tmp_path, monkeypatch):
    """A randomly initialised policy on the duck, 2 commands x 32 envs, 80 steps, ring 8.  The eager run's recording, pushed through the
    restatement, has the accumulator's bits; the report's "falls" objects are `reduce_falls` of the restatement and the saved clips the
    recorded qpos; the graph run has the eager run's bits and objects; the same arguments without --falls give the same report minus the
    "falls" keys and the settings entries, and the same tracking bits."""
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 32, 80
    out, clips = tmp_path / "report.json", str(tmp_path / "falls.npz")
    argv = ["--checkpoint", ckpt, "--command", "0.15", "0", "0", "--command", "0", "0", "1.0", "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "1", "--output", str(out)]
    flags = ["--falls", "--fall_ring", str(TRACK_RING), "--save_falls", clips, "--save_falls_max", "5"]
    rep_e, tr_e, hist = _run(track, monkeypatch, argv + flags, eager=True)
    assert not rep_e["settings"]["graph"] and len(hist) == T
    want, qpos_hist, _ = _restate_run(track, rep_e, tr_e, hist)
    nq = int(tr_e.env.batch.model.nq)
    ref = track.reduce_falls(want, rep_e["commands"], E, rep_e["settings"]["dt"], TRACK_RING, nq)
    for row, w in zip(rep_e["commands"], ref):
        assert tuple(row) == track.ROW_KEYS + ("falls",) and tuple(row["falls"]) == track.FALL_KEYS
        assert row["falls"] == w and row["falls"]["episodes"] == E
        assert row["falls"]["fall_rate"] == row["fall_rate"]                       # the tracking accumulator's FALLS
    falls = sum(r["falls"]["falls"] for r in rep_e["commands"])
    print("falls per row:", [r["falls"]["falls"] for r in rep_e["commands"]], "profile counts:", [r["falls"]["profile"]["count"] for r in rep_e["commands"]])
    assert falls >= 1                                                              # the env's own random pushes fell somebody
    assert json.load(open(out)) == json.loads(json.dumps(rep_e))
    z = _check_clips(clips, want, qpos_hist, rep_e["commands"], E, nq, 5)
    assert float(z["dt"]) == rep_e["settings"]["dt"] and len(z["env"]) >= 1
    track_e = tr_e.acc.cpu().numpy()

    rep_g, tr_g, _ = _run(track, monkeypatch, argv + flags)
    assert rep_g["settings"]["graph"]
    np.testing.assert_array_equal(tr_g.fall_acc.cpu().numpy().view(np.int32), tr_e.fall_acc.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(tr_g.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    assert [r["falls"] for r in rep_g["commands"]] == [r["falls"] for r in rep_e["commands"]]

    calls = []
    real = engine.Batch.fall_accumulate
    monkeypatch.setattr(engine.Batch, "fall_accumulate", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    rep_p, tr_p, _ = _run(track, monkeypatch, argv)
    assert calls == [] and tr_p.fall_acc is None and tr_p.torque_limit is None
    np.testing.assert_array_equal(tr_p.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    new_settings = ["falls", "fall_ring", "fall_tilt", "fall_tilt_tol", "save_falls", "save_falls_max"]
    assert [k for k in rep_g["settings"] if k not in rep_p["settings"]] == new_settings
    assert rep_p["settings"] == {k: v for k, v in rep_g["settings"].items() if k not in new_settings}
    assert rep_p["commands"] == [{k: v for k, v in r.items() if k != "falls"} for r in rep_g["commands"]]


def test_track_falls_with_a_push_grid(tmp_path, monkeypatch):
    """2 commands x (2 magnitudes x 2 directions) x 32 envs, kicked at step 5, 40 steps: one object per cell and one per row, clips per cell."""
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 32, 40
    clips = str(tmp_path / "falls.npz")
    argv = ["--checkpoint", ckpt, "--command", "0.15", "0", "0", "--command", "0", "0", "1.0", "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "1", "--output", str(tmp_path / "r.json"), "--push_grid", "magnitude=0:1.5:2,direction=0:180:2", "--push_at", "5",
            "--falls", "--fall_ring", str(TRACK_RING), "--save_falls", clips, "--save_falls_max", "3"]
    rep, tr, hist = _run(track, monkeypatch, argv, eager=True)
    assert rep["settings"]["num_envs"] == 2 * 4 * E
    want, qpos_hist, _ = _restate_run(track, rep, tr, hist)
    nq, dt = int(tr.env.batch.model.nq), rep["settings"]["dt"]
    cells = [cell for row in rep["commands"] for cell in row["pushes"]]
    assert len(cells) == 8 and all(tuple(c) == track.PUSH_CELL_KEYS + ("falls",) for c in cells)
    assert [c["falls"] for c in cells] == track.reduce_falls(want, cells, E, dt, TRACK_RING, nq)
    assert [r["falls"] for r in rep["commands"]] == track.reduce_falls(want, rep["commands"], 4 * E, dt, TRACK_RING, nq)
    for row in rep["commands"]:
        assert tuple(row) == track.ROW_KEYS + track.PUSH_ROW_KEYS + ("falls",)
        assert sum(c["falls"]["falls"] for c in row["pushes"]) == row["falls"]["falls"] and row["falls"]["episodes"] == 4 * E
    print("falls per cell:", [c["falls"]["falls"] for c in cells])
    assert sum(c["falls"]["falls"] for c in cells if c["magnitude"] > 0) >= 1      # a 1.5 m/s kick fells somebody
    block_cmds = [dict(command=row["command"]) for row in rep["commands"] for _ in row["pushes"]]
    z = _check_clips(clips, want, qpos_hist, block_cmds, E, nq, 3)
    assert len(z["env"]) >= 1


def test_track_falls_under_a_command_schedule(tmp_path, monkeypatch):
    """--then 0 0 0 --switch_at 10: the command errors in the ring are against the command in force at each sample's step."""
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 32, 40
    argv = ["--checkpoint", ckpt, "--command", "0.15", "0", "0", "--command", "0", "0", "1.0", "--then", "0", "0", "0", "--switch_at", "10",
            "--envs_per_command", str(E), "--episode_length", str(T), "--seed", "1", "--output", str(tmp_path / "r.json"),
            "--falls", "--fall_ring", str(TRACK_RING)]
    rep, tr, hist = _run(track, monkeypatch, argv, eager=True)
    want, qpos_hist, cmd = _restate_run(track, rep, tr, hist)
    b = tr.env.batch
    nq, nobs = int(b.model.nq), b.nobs
    rows = rep["commands"]
    assert len(rows) == 2 and all(tuple(r) == track.ROW_KEYS + track.SCHEDULE_ROW_KEYS + ("falls",) for r in rows)
    assert [r["falls"] for r in rows] == track.reduce_falls(want, rows, E, rep["settings"]["dt"], TRACK_RING, nq)
    froms = f32([[0.15, 0, 0], [0, 0, 1.0]])
    np.testing.assert_array_equal(cmd[9, :, :3], np.repeat(froms, E, axis=0))     # the recording itself: the from-command up to step 9 ...
    np.testing.assert_array_equal(cmd[10:, :, :3], 0.0)                           # ... and 0 0 0 from step 10
    priv = np.stack([h[0] for h in hist])
    slots = want[:, G.FALL_HEAD:].reshape(2 * E, TRACK_RING, G.FALL_SAMPLE + nq)
    before = after = 0
    for e in range(2 * E):
        for S in slots[e][:min(int(want[e, G.FALL_SAMPLES]), TRACK_RING)]:
            t = int(S[G.FALL_S_STEP])
            c = froms[e // E] if t < 10 else f32([0, 0, 0])
            Q = priv[t, e, nobs:]
            assert S[G.FALL_S_LIN_ERR] == RC.planar32(f32(Q[9] - c[0]), f32(Q[10] - c[1])) and S[G.FALL_S_ANG_ERR] == np.abs(f32(Q[2] - c[2])), (e, t)
            before, after = before + (t < 10), after + (t >= 10)
    print("ring samples before / after the switch:", before, after)
    assert after > 0


def test_refusals_launch_nothing():
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine, joystick
    n, ring = 16, 4
    env = joystick.Joystick(task="flat_terrain", num_envs=n)
    b = env.batch
    L = engine.load_library()
    env.reset(1)
    b.step(torch.zeros(n, 14, device="cuda"))
    rf = b.fall_row_floats(ring)
    assert rf == L.odk_fall_row_floats(b._b, ring) == G.FALL_HEAD + ring * (G.FALL_SAMPLE + int(b.model.nq))
    assert L.odk_fall_row_floats(b._b, 0) < 0 and L.odk_fall_row_floats(b._b, G.FALL_MAX_RING + 1) < 0 and L.odk_fall_row_floats(None, ring) < 0
    assert L.odk_fall_row_floats(b._b, G.FALL_MAX_RING) == G.FALL_HEAD + G.FALL_MAX_RING * (G.FALL_SAMPLE + int(b.model.nq))
    acc = torch.full((n, rf), 9.0, device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    lim = torch.ones(14, device="cuda")
    cmd = torch.zeros(n, 7, device="cuda")
    good = dict(priv_dev=b.priv.data_ptr(), done_dev=b.done.data_ptr(), truncation_dev=b.truncation.data_ptr(), track_acc_dev=tacc.data_ptr(),
                torque_limit_dev=lim.data_ptr(), acc_dev=acc.data_ptr())

    def raw(batch=b._b, null=None, tol=0.3, ring=ring, stride=rf):
        a = {k: (None if k == null else C.c_void_p(v)) for k, v in good.items()}
        return L.odk_fall_accumulate(batch, a["priv_dev"], a["done_dev"], a["truncation_dev"], a["track_acc_dev"], a["torque_limit_dev"], C.c_float(tol), ring,
                                     a["acc_dev"], stride, b._stream())

    def refused(what, **kw):
        assert raw(**kw) == G.ERR_INVALID, what
        msg = L.odk_last_error().decode()
        assert "odk_fall_accumulate" in msg and what in msg, msg

    assert b.commands is None
    refused("no commands bound")
    b.bind_commands(cmd)
    for null in ("acc_dev", "priv_dev", "done_dev", "truncation_dev", "track_acc_dev"):
        refused(null, null=null)
    refused("batch", batch=None)
    refused("ring = 0", ring=0)
    refused(f"ring = {G.FALL_MAX_RING + 1}", ring=G.FALL_MAX_RING + 1)
    refused("ring = -1", ring=-1)
    refused(f"row_stride = {rf - 1}", stride=rf - 1)
    refused("row_stride", ring=ring + 1)                       # the same row is too short for a longer ring
    refused("tilt_tol", tol=-0.1)
    refused("tilt_tol", tol=float("nan"))
    refused("tilt_tol", tol=float("inf"))
    # the Python surface: OdkErrors before anything is launched
    bad = [(torch.full((n, rf - 1), 9.0, device="cuda"), tacc, 0.3, ring, lim), (acc, tacc, 0.3, 0, lim), (acc, tacc, 0.3, G.FALL_MAX_RING + 1, lim),
           (acc, tacc, -1.0, ring, lim), (acc, tacc, float("nan"), ring, lim), (acc.cpu(), tacc, 0.3, ring, lim), (acc, tacc.cpu(), 0.3, ring, lim),
           (acc, tacc, 0.3, ring, torch.ones(13, device="cuda")), (acc, tacc, 0.3, ring, np.ones(14, np.float32)), (acc.double(), tacc, 0.3, ring, lim)]
    for args in bad:
        with pytest.raises(engine.OdkError, match="fall_accumulate|fall_row_floats"):
            b.fall_accumulate(*args)
    b.bind_commands(None)
    with pytest.raises(engine.OdkError, match="fall_accumulate: no commands bound"):
        b.fall_accumulate(acc, tacc, 0.3, ring, lim)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy(), 9.0)
    # and the good call, with and without the optional limit, writes
    b.bind_commands(cmd)
    acc.zero_()
    b.fall_accumulate(acc, tacc, 0.3, ring)
    b.fall_accumulate(acc, tacc, 0.3, ring, lim)
    torch.cuda.synchronize()
    assert float(acc[:, G.FALL_SAMPLES].sum()) > 0.0
    b.bind_commands(None)
    b.close()
