"""GPU checks of the imitation-fidelity accumulator (odk_imitation_accumulate / Batch.imitation_accumulate) and of `track
--imitation_report`: every slot against a numpy restatement on synthetic privileged rows (four robots: nu 12, 14, 15 and 16; a map that is
partial and not ascending; a partly filled last block and wave; folded and unfolded lags), rows that are no sample keeping their bits, the
report of a real run against the same restatement over the recorded outputs, eager against graph, with and without pushes, gait and
posture, a captured graph that follows a later joint map, and the refusals.

One refusal of the C entry has no test: a model with more than 16 actuators.  No such model loads (MAXU = 16 in csrc/odk_model.h: the
loader refuses it by name), so no batch of one exists to hand to the call."""
import functools
import json
import os
import pickle

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

G = RC.HEADER         # include/odk.h's constants, by engine's names

DUCK_MAP = [0, 1, 2, 3, 4, -1, -1, -1, -1, 11, 12, 13, 14, 15]
PERIOD = 12


def restate(priv, done, ended, nobs, nu, imap, kc, period):
    """odk_imitation_accumulate restated over float32 inputs: priv [T, n, npriv], done [T, n], ended [T, n] (the tracking accumulator's
    ENDED column as the launch of step t saw it), imap [nu] (frame joint per actuator, -1: none), kc [nu] float32 home pose.  jq, dp, dv,
    the command gate and the contact thresholds are float32, in the kernel's order; the sums are float64.  Returns the [n, 160]
    accumulator, per actuator the sum of |dp| (the scale of POS_ERR_SUM's bound) and what the data exercised: folded lags below zero, lags
    above zero, lags of zero, and robot touchdowns before any reference touchdown (not counted)."""
    planar32 = RC.planar32
    T, n = done.shape
    A = np.zeros((n, G.IMIT_NACC), np.float64)
    absdp = np.zeros((n, G.IMIT_STRIDE), np.float64)
    seen = dict(negative=0, positive=0, zero=0, before_reference=0)
    kc = np.asarray(kc, np.float32)
    imap = np.asarray(imap)
    us = np.nonzero(imap >= 0)[0]
    ri = imap[us]
    f32 = np.float32
    for e in range(n):
        R = A[e]
        for t in range(T):
            if ended[t, e] != 0 or done[t, e] != 0:
                continue
            P = priv[t, e]
            Q = P[nobs:]
            F = Q[26 + 3 * nu:]
            first = R[G.IMIT_SAMPLES] == 0
            R[G.IMIT_SAMPLES] += 1
            c = P[6:9]
            cn = np.sqrt(f32(f32(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]))
            R[G.IMIT_GATED] += 1.0 if cn > f32(0.01) else 0.0
            sr = planar32(F[34], F[35])
            ds = f32(planar32(Q[9], Q[10]) - sr)
            R[G.IMIT_SPEED_ERR_SQ_SUM] += np.float64(ds) ** 2
            R[G.IMIT_REF_SPEED_SUM] += np.float64(sr)
            jq = (Q[15 + us] + kc[us]).astype(f32)                # float32 + float32: one rounding, as the kernel's
            rq = F[ri]
            dp = (jq - rq).astype(f32)
            dv = (Q[15 + nu + us] - F[16 + ri]).astype(f32)
            dp64, dv64, jq64, rq64 = (x.astype(np.float64) for x in (dp, dv, jq, rq))
            R[G.IMIT_JOINT_POS_SQ_SUM] += (dp64 ** 2).sum()
            R[G.IMIT_JOINT_VEL_SQ_SUM] += (dv64 ** 2).sum()
            R[G.IMIT_POS_ERR_SUM + us] += dp64
            absdp[e, us] += np.abs(dp64)
            R[G.IMIT_POS_ERR_SQ + us] += dp64 ** 2
            R[G.IMIT_POS_ERR_PEAK + us] = np.maximum(R[G.IMIT_POS_ERR_PEAK + us], np.abs(dp64))
            R[G.IMIT_VEL_ERR_SQ + us] += dv64 ** 2
            R[G.IMIT_RANGE_MIN + us] = jq64 if first else np.minimum(R[G.IMIT_RANGE_MIN + us], jq64)
            R[G.IMIT_RANGE_MAX + us] = jq64 if first else np.maximum(R[G.IMIT_RANGE_MAX + us], jq64)
            R[G.IMIT_REF_RANGE_MIN + us] = rq64 if first else np.minimum(R[G.IMIT_REF_RANGE_MIN + us], rq64)
            R[G.IMIT_REF_RANGE_MAX + us] = rq64 if first else np.maximum(R[G.IMIT_REF_RANGE_MAX + us], rq64)
            for f in range(2):
                con, ref = bool(Q[16 + 3 * nu + f] != 0), bool(F[32 + f] > f32(0.5))
                R[G.IMIT_BOTH + f] += con and ref
                R[G.IMIT_ROBOT_ONLY + f] += con and not ref
                R[G.IMIT_REF_ONLY + f] += (not con) and ref
                if ref and not first and R[G.IMIT_PREV_REF + f] == 0:      # the reference first
                    R[G.IMIT_REF_TOUCHDOWNS + f] += 1
                    R[G.IMIT_REF_AGE + f] = 1
                elif R[G.IMIT_REF_AGE + f] > 0:
                    R[G.IMIT_REF_AGE + f] += 1
                if con and not first and R[G.IMIT_PREV_CONTACT + f] == 0:
                    if R[G.IMIT_REF_AGE + f] > 0:
                        lag = R[G.IMIT_REF_AGE + f] - 1
                        if period > 0 and 2 * lag > period:
                            lag -= period
                        R[G.IMIT_TOUCHDOWNS + f] += 1
                        R[G.IMIT_LAG_SUM + f] += lag
                        R[G.IMIT_LAG_ABS_SUM + f] += abs(lag)
                        seen["negative" if lag < 0 else "positive" if lag > 0 else "zero"] += 1
                    else:
                        seen["before_reference"] += 1
                R[G.IMIT_PREV_CONTACT + f] = con
                R[G.IMIT_PREV_REF + f] = ref
    return A, absdp, seen


def compare(got, want, absdp, label):
    """Counts, peaks, ranges, bookkeeping and the integer lag sums exact; the float32 running sums within RC.compare_sums' bound: of
    non-negative terms but for POS_ERR_SUM, the one signed sum, whose scale is sum |dp|."""
    lanes = range(G.IMIT_STRIDE)
    sums = [G.IMIT_SPEED_ERR_SQ_SUM, G.IMIT_REF_SPEED_SUM, G.IMIT_JOINT_POS_SQ_SUM, G.IMIT_JOINT_VEL_SQ_SUM]
    sums += [s + u for s in (G.IMIT_POS_ERR_SQ, G.IMIT_VEL_ERR_SQ) for u in lanes]
    scales = {c: want[:, c] for c in sums}
    scales.update({G.IMIT_POS_ERR_SUM + u: absdp[:, u] for u in lanes})
    RC.compare_sums(got, want, G.IMIT_SAMPLES, scales, label)


def _entry(coeffs_lowest_first, period, fps):
    return dict(period=period, fps=fps, coefficients={f"dim_{k}": [np.float64(c) for c in row] for k, row in enumerate(coeffs_lowest_first)})


def _write_synthetic(path, J, seed=0):
    """A reference-motion pickle of J frame joints in the reference's format: a 3 x 2 x 4 command grid, 20 steps per period (0.4 s at 50
    fps), degree 15, |c| <= 0.05 (tests/test_gpu_reference_motion.py's)."""
    rng = np.random.default_rng(seed)
    grid = ([-0.1, 0.05, 0.2], [-0.1, 0.1], [-0.5, 0.0, 0.4, 0.8])
    data = {f"{dx}_{dy}_{dth}": _entry(rng.uniform(-0.05, 0.05, (2 * J + 8, 16)), 0.4, 50) for dx in grid[0] for dy in grid[1] for dth in grid[2]}
    with open(path, "wb") as f:
        pickle.dump(data, f)
    return str(path)


def _batch(robot, nu, n, tmp, imap):
    """A Joystick batch of `robot` with the imitation reward on: the duck on the shipped table and its own map, another robot on a synthetic
    reference motion of its actuator count with the map given."""
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    from open_duck_playground_amd.reference_motion import ReferenceMotion
    cfg = engine.default_config()
    assert cfg.use_imitation == 1
    if robot == "duck":
        model = load_task_model("flat_terrain")
        b = engine.Batch(model, n, cfg)
    else:
        model = Model.from_xml(os.path.join(RC.ASSETS, robot))
        motion = ReferenceMotion.from_pickle(_write_synthetic(os.path.join(tmp, f"{robot}.pkl"), nu, seed=nu))
        b = engine.Batch(model, n, cfg, prm=motion.prm())
        if imap is not None:
            b.set_imitation_joints(imap)
    assert model.nu == nu == b.model.nu
    return model, b


# robot, nu, the map given to Batch.set_imitation_joints (None: the batch's default), period_steps
CASES = {
    "duck": ("duck", 14, None, PERIOD),                                               # its default map: the head's four lanes idle
    "biped12": ("biped12.xml", 12, [11, 10, -1, 8, 7, 6, 5, 4, -1, 2, 1, 0], PERIOD),   # partial and not ascending: frame joints reversed
    "tail_biped": ("tail_biped.xml", 15, list(range(12)) + [-1, -1, -1], PERIOD),     # the legs; the tail is left out
    "biped_arms": ("biped_arms.xml", 16, [(5 * u + 3) % 16 for u in range(16)], PERIOD),   # every lane live, a permutation of the frame
    "duck_unfolded": ("duck", 14, None, 0),                                           # period_steps = 0: no lag is folded
}
N_ENVS, T_STEPS = 70, 40      # 70 envs: four full 256-thread blocks of 16 envs and one with 6; its second wave holds 2 envs


def synthetic_rows(rng, T, n, nobs, npriv, nu):
    """[T, n, npriv] float32 privileged rows, random but for: commands either 0 or of norm >= 0.05 (the gate is 0.01); the robot's contacts
    0 or 1 and the reference's in 0 .. 0.3 or 0.7 .. 1 (the threshold is 0.5), both a 12-step cycle with 6 steps of stance, the
    reference's starting anywhere in its cycle and the robot's shifted against it by -5 .. 5 steps per env and foot, with a few random
    flips: every env sees several touchdowns of both kinds, with lags of both signs after folding."""
    priv = rng.normal(0.0, 1.0, (T, n, npriv)).astype(np.float32)
    move = rng.uniform(size=(T, n)) < 0.7
    c = rng.uniform(0.05, 0.6, (T, n, 3)) * rng.choice([-1.0, 1.0], (T, n, 3))
    priv[:, :, 6:9] = (c * move[..., None]).astype(np.float32)
    steps = np.arange(T)[:, None, None]
    phase = rng.integers(0, PERIOD, (1, n, 2))
    shift = rng.integers(-5, 6, (1, n, 2))
    ref = (steps + phase) % PERIOD < 6
    con = (steps + phase - shift) % PERIOD < 6
    con ^= rng.uniform(size=con.shape) < 0.04
    ref ^= rng.uniform(size=ref.shape) < 0.02
    priv[:, :, nobs + 16 + 3 * nu:nobs + 18 + 3 * nu] = con.astype(np.float32)
    F0 = nobs + 26 + 3 * nu
    priv[:, :, F0 + 32:F0 + 34] = np.where(ref, rng.uniform(0.7, 1.0, ref.shape), rng.uniform(0.0, 0.3, ref.shape)).astype(np.float32)
    return priv


def synthetic_inputs(nobs, npriv, nu):
    """The host half of `synthetic`, a function of the sizes alone: 70 envs, 40 steps of `synthetic_rows`; first episodes end at step 0,
    mid-run or never, by done with and without truncation.  Returns (priv [T, n, npriv], done, trunc, ended [T, n], end_at [n])."""
    n, T = N_ENVS, T_STEPS
    rng = np.random.default_rng(500 + nu)
    priv = synthetic_rows(rng, T, n, nobs, npriv, nu)
    # first episodes: never ending; done at step 0 without / with truncation; done mid-run without / with truncation
    end_at, done, trunc, ended = RC.first_episodes(rng, T, n, ends=(T + 1, 0, 0, 23, 31), truncated=(2, 4))
    return priv, done, trunc, ended, end_at


@functools.lru_cache(maxsize=None)
def synthetic(case):
    """One run per case, shared by the tests below: `synthetic_inputs` written straight into the batch's buffers -- no odk_step --, the
    tracking accumulator's ENDED column set as odk_tracking_accumulate would have."""
    import tempfile
    from open_duck_playground_amd import engine
    robot, nu, given, period = CASES[case]
    n = N_ENVS
    with tempfile.TemporaryDirectory() as tmp:
        model, b = _batch(robot, nu, n, tmp, given)
    imap = DUCK_MAP if given is None else list(given)
    nobs, npriv = b.nobs, b.npriv
    assert tuple(b.priv.shape) == (n, npriv) and nobs + 26 + 3 * nu + 40 <= npriv
    kc = RC.home_pose(model, nu)
    priv, done, trunc, ended, end_at = synthetic_inputs(nobs, npriv, nu)
    want, absdp, seen = restate(priv, done, ended, nobs, nu, imap, kc, period)
    got, guard_tail, snaps = RC.drive_rows(b, lambda acc, tacc: b.imitation_accumulate(acc, tacc, period), engine.IMIT_NACC, priv, done, trunc, ended)
    res = dict(got=got, want=want, absdp=absdp, seen=seen, guard=guard_tail, snaps=snaps, imap=imap, end_at=end_at, nu=nu, period=period)
    b.close()
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_every_slot_matches_a_numpy_restatement_on_synthetic_rows(case):
    GATED, LAG_SUM, LAG_ABS_SUM, REF_TOUCHDOWNS, TOUCHDOWNS = G.IMIT_GATED, G.IMIT_LAG_SUM, G.IMIT_LAG_ABS_SUM, G.IMIT_REF_TOUCHDOWNS, G.IMIT_TOUCHDOWNS
    POS_ERR_SQ, RANGE_MIN, RANGE_MAX, REF_RANGE_MIN, REF_RANGE_MAX = G.IMIT_POS_ERR_SQ, G.IMIT_RANGE_MIN, G.IMIT_RANGE_MAX, G.IMIT_REF_RANGE_MIN, G.IMIT_REF_RANGE_MAX
    r = synthetic(case)
    got, want, imap, seen, nu = r["got"], r["want"], r["imap"], r["seen"], r["nu"]
    compare(got, want, r["absdp"], f"{case} nu={nu}")
    np.testing.assert_array_equal(r["guard"], 7.0)
    # the run covers what it claims to
    N = want[:, G.IMIT_SAMPLES]
    assert set(N.astype(int)) == {0, 23, 31, T_STEPS}
    assert np.all(got[N == 0] == 0.0)
    assert np.all(got[:, G.IMIT_REF_AGE + 2:G.IMIT_POS_ERR_SUM] == 0.0)      # no slot lives there
    print(f"{case}: lags {seen}")
    assert seen["positive"] > 20 and seen["zero"] > 0 and seen["before_reference"] > 0
    if r["period"] > 0:
        assert seen["negative"] > 20                                   # folded: past half a period counts as early
        assert np.all(np.abs(want[:, LAG_SUM:LAG_SUM + 2]) <= want[:, LAG_ABS_SUM:LAG_ABS_SUM + 2])
        assert np.any(want[:, LAG_SUM:LAG_SUM + 2] < 0)
    else:
        assert seen["negative"] == 0
        np.testing.assert_array_equal(got[:, LAG_SUM:LAG_SUM + 2], got[:, LAG_ABS_SUM:LAG_ABS_SUM + 2])
        folded = synthetic("duck")["got"]                              # the same rows (the seed goes by nu) under a period of 12
        np.testing.assert_array_equal(got[:, TOUCHDOWNS:TOUCHDOWNS + 2], folded[:, TOUCHDOWNS:TOUCHDOWNS + 2])
        assert np.all(got[:, LAG_SUM:LAG_SUM + 2] >= folded[:, LAG_SUM:LAG_SUM + 2]) and np.any(got[:, LAG_SUM:LAG_SUM + 2] > folded[:, LAG_SUM:LAG_SUM + 2])
    whole = N == T_STEPS                                               # the envs that run all 40 steps: several touchdowns of both kinds per foot
    assert np.all(got[whole][:, [REF_TOUCHDOWNS, REF_TOUCHDOWNS + 1, TOUCHDOWNS, TOUCHDOWNS + 1]] >= 2)
    assert 0 < got[N > 0, GATED].min() and np.all(got[N > 0, GATED] < N[N > 0])      # both sides of the gate in every env
    live = N > 0
    for u in range(G.IMIT_STRIDE):
        cols = [s + u for s in (G.IMIT_POS_ERR_SUM, POS_ERR_SQ, G.IMIT_POS_ERR_PEAK, G.IMIT_VEL_ERR_SQ, RANGE_MIN, RANGE_MAX, REF_RANGE_MIN, REF_RANGE_MAX)]
        if u >= nu or imap[u] < 0:
            assert np.all(got[:, cols] == 0.0), u                      # a lane past nu, or an actuator the map leaves out, stays 0
        else:
            assert np.all(got[live, POS_ERR_SQ + u] > 0.0) and np.all(got[live, RANGE_MIN + u] < got[live, RANGE_MAX + u])
            assert np.all(got[live, REF_RANGE_MIN + u] < got[live, REF_RANGE_MAX + u])


@pytest.mark.parametrize("case", ["duck", "biped12"])
def test_a_row_that_is_no_sample_keeps_its_bits(case):
    """Rows of envs past their first episode (and of the done step that ends it): what step end_at - 1 left is what every later step
    leaves; and one launch over an accumulator full of a bit pattern changes no bit of the rows with `done` or ENDED set."""
    import tempfile
    import torch
    from open_duck_playground_amd import engine
    r = synthetic(case)
    snaps, end_at = r["snaps"].view(np.int32), r["end_at"]
    assert RC.assert_frozen_after_end(snaps, end_at) > 100
    e = int(np.argmax(end_at > T_STEPS))      # while a live row changes at every step
    S, NACC = engine.IMIT_SAMPLES, engine.IMIT_NACC
    assert all(snaps[t, e, S] != snaps[t - 1, e, S] for t in range(1, T_STEPS))

    robot, nu, given, period = CASES[case]
    n = N_ENVS
    with tempfile.TemporaryDirectory() as tmp:
        _, b = _batch(robot, nu, n, tmp, given)
    rng = np.random.default_rng(9)
    b.priv.copy_(torch.tensor(synthetic_rows(rng, 1, n, b.nobs, b.npriv, nu)[0], device="cuda"))
    done = (np.arange(n) % 3 == 1).astype(np.float32)
    ended = (np.arange(n) % 4 == 2).astype(np.float32)
    b.done.copy_(torch.tensor(done, device="cuda"))
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    tacc[:, engine.TRACK_ENDED] = torch.tensor(ended, device="cuda")
    pattern = (np.arange(n * NACC, dtype=np.int64) * 2654435761 % 2 ** 31).astype(np.int32).reshape(n, NACC)      # NaNs, denormals, anything
    acc = torch.tensor(pattern, device="cuda").view(torch.float32)
    b.imitation_accumulate(acc, tacc, period)
    torch.cuda.synchronize()
    after = acc.view(torch.int32).cpu().numpy()
    frozen = (done != 0) | (ended != 0)
    assert frozen.sum() > 20 and (~frozen).sum() > 20
    np.testing.assert_array_equal(after[frozen], pattern[frozen])
    assert np.all(np.any(after[~frozen] != pattern[~frozen], axis=1))      # a sample row did change
    b.close()


EXACT_FIELDS = ("samples", "gated_share", "period_steps", "joint", "frame_joint", "peak_error", "range", "reference_range", "amplitude_ratio", "foot",
                "contact_agreement", "stance_share", "reference_stance_share", "touchdowns", "reference_touchdowns", "touchdown_lag_steps",
                "touchdown_lag_s", "touchdown_lag_abs_steps", "contact_term")


def test_track_imitation_report_end_to_end(tmp_path, monkeypatch):
    """A randomly initialised policy on the duck, two commands, 8 envs each, 60 steps; envs fall, so done and ENDED rows occur.  The eager
    run's recording, pushed through the numpy restatement and `reduce_imitation`, reproduces the accumulator (the bounds of the synthetic
    test) and the report; the graph run's imitation and tracking accumulators have the eager run's bits; without the flag the tracking
    accumulator has the same bits and the report its old keys."""
    from open_duck_playground_amd import engine, track
    from open_duck_playground_amd.reference_motion import ReferenceMotion
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 8, 60
    out = tmp_path / "report.json"
    argv = ["--checkpoint", ckpt, "--command", "0.1", "0", "0", "--command", "0", "0", "0", "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "1", "--output", str(out)]
    on = ["--imitation_report"]
    rep_e, tr_e, hist = RC.run_track_with_ended(track, monkeypatch, argv + on, eager=True)
    period = ReferenceMotion.from_npz().nb_steps_in_period
    assert not rep_e["settings"]["graph"] and rep_e["settings"]["imitation_report"] is True and len(hist) == T
    assert rep_e["settings"]["imitation_period_steps"] == tr_e.period_steps == period > 0
    priv, done, ended = (np.stack([h[i] for h in hist]) for i in range(3))
    np.testing.assert_array_equal(ended, np.concatenate([np.zeros((1, 2 * E)), (np.cumsum(done != 0, 0) > 0)[:-1]]))
    assert done.any() and ended.any()                                  # envs fell: rows that are no sample occur
    model = tr_e.env.mj_model
    nobs = tr_e.env.batch.nobs
    imap, joints, period_env = track.imitation_joint_info(tr_e.env)
    assert imap == DUCK_MAP and period_env == period and len(joints) == 14
    kc = np.asarray(model.a["key_ctrl"], np.float64).reshape(-1)[:14].astype(np.float32)
    want, absdp, seen = restate(priv, done, ended, nobs, 14, imap, kc, period)
    got_e = tr_e.imitation_acc.cpu().numpy()
    compare(got_e, want, absdp, "track --imitation_report, eager")
    track_e = tr_e.acc.cpu().numpy()
    SAMPLES, GATED = engine.IMIT_SAMPLES, engine.IMIT_GATED
    np.testing.assert_array_equal(got_e[:, SAMPLES], track_e[:, engine.TRACK_SAMPLES])     # an imitation sample is a velocity sample
    assert got_e[:, SAMPLES].sum() > 0
    # the command gate: block 0 moves, block 1 stands
    np.testing.assert_array_equal(got_e[:E, GATED], got_e[:E, SAMPLES])
    np.testing.assert_array_equal(got_e[E:, GATED], 0.0)

    # the report is reduce_imitation of that accumulator; against the restatement the exact slots give equal figures and every mean is a
    # ratio of two sums (or its root): twice the sum bound -- for the signed bias at the scale of the mean |dp|
    rel = 2 * (T + 4) * 2.0 ** -23
    commands = [r["command"] for r in rep_e["commands"]]
    ref = track.reduce_imitation(want, commands, E, rep_e["settings"]["dt"], imap, joints, period)
    for c, (row, w) in enumerate(zip(rep_e["commands"], ref)):
        assert tuple(row) == track.ROW_KEYS + ("imitation",)
        g = row["imitation"]
        assert tuple(g) == track.IMITATION_KEYS and g["samples"] == w["samples"] > 0 and g["period_steps"] == period
        assert [j["frame_joint"] for j in g["joints"]] == [r for r in imap if r >= 0] and [f["foot"] for f in g["feet"]] == ["left", "right"]
        assert g["gated_share"] == (1.0 if c == 0 else 0.0)
        blk = slice(c * E, (c + 1) * E)
        pairs = [("", g, w)] + [(f"joints[{k}].", a, b) for k, (a, b) in enumerate(zip(g["joints"], w["joints"]))]
        pairs += [(f"feet[{k}].", a, b) for k, (a, b) in enumerate(zip(g["feet"], w["feet"]))]
        for prefix, a, b in pairs:
            assert list(a) == list(b)
            for key in a:
                if key in ("joints", "feet"):
                    continue
                if key in EXACT_FIELDS or b[key] is None:
                    assert a[key] == b[key], (prefix + key, a[key], b[key])
                elif key == "bias":
                    u = joints.index(a["joint"])
                    assert abs(a[key] - b[key]) <= rel * absdp[blk, u].sum() / w["samples"], (prefix + key, a[key], b[key])
                else:
                    assert a[key] == pytest.approx(b[key], rel=rel, abs=0), (prefix + key, a[key], b[key])
    assert json.load(open(out)) == json.loads(json.dumps(rep_e))

    # the graph: one more launch in the captured step, the same bits
    rep_g, tr_g, _ = RC.run_track_with_ended(track, monkeypatch, argv + on)
    assert rep_g["settings"]["graph"]
    np.testing.assert_array_equal(tr_g.imitation_acc.cpu().numpy().view(np.int32), got_e.view(np.int32))
    np.testing.assert_array_equal(tr_g.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    assert [r["imitation"] for r in rep_g["commands"]] == [r["imitation"] for r in rep_e["commands"]]

    # without the flag: no accumulator, no launch, the old report, the same tracking bits
    calls = []
    real = engine.Batch.imitation_accumulate
    monkeypatch.setattr(engine.Batch, "imitation_accumulate", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    rep_p, tr_p, _ = RC.run_track_with_ended(track, monkeypatch, argv)
    assert calls == [] and tr_p.imitation_acc is None
    np.testing.assert_array_equal(tr_p.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    assert tuple(rep_p) == track.REPORT_KEYS and "imitation_report" not in rep_p["settings"]
    assert all(tuple(r) == track.ROW_KEYS for r in rep_p["commands"])
    assert [k for k in rep_g["settings"] if k not in rep_p["settings"]] == ["imitation_report", "imitation_period_steps"]
    for a, bb in zip(rep_p["commands"], rep_g["commands"]):
        assert a == {k: v for k, v in bb.items() if k != "imitation"}


def test_track_imitation_report_with_a_push_gait_and_posture(tmp_path, monkeypatch):
    """One command, two pushes, 4 envs per cell, --gait --posture: every cell and the command row get an "imitation" object, the cells'
    samples add up to the row's, and the other objects and the push, gait, posture and tracking accumulators are those of a run without
    the flag."""
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    argv = ["--checkpoint", ckpt, "--command", "0.1", "0", "0", "--push", "0", "0", "--push", "1.5", "0", "--push_at", "10", "--envs_per_command", "4",
            "--episode_length", "40", "--seed", "2", "--gait", "--posture", "--output", str(tmp_path / "r.json")]
    rep_s, tr_s, _ = RC.run_track_with_ended(track, monkeypatch, argv + ["--imitation_report"])
    rep_p, tr_p, _ = RC.run_track_with_ended(track, monkeypatch, argv)
    assert rep_s["settings"]["imitation_report"] is True and "imitation_report" not in rep_p["settings"]
    (row,), (plain,) = rep_s["commands"], rep_p["commands"]
    assert tuple(row) == track.ROW_KEYS + track.PUSH_ROW_KEYS + ("gait", "posture", "imitation")
    assert tuple(plain) == track.ROW_KEYS + track.PUSH_ROW_KEYS + ("gait", "posture")
    assert len(row["pushes"]) == 2
    for cell, old in zip(row["pushes"], plain["pushes"]):
        assert tuple(cell) == track.PUSH_CELL_KEYS + ("gait", "posture", "imitation")
        assert {k: v for k, v in cell.items() if k != "imitation"} == old
        assert tuple(cell["imitation"]) == track.IMITATION_KEYS
    assert {k: v for k, v in row.items() if k not in ("imitation", "pushes")} == {k: v for k, v in plain.items() if k != "pushes"}
    assert sum(c["imitation"]["samples"] for c in row["pushes"]) == row["imitation"]["samples"] == row["velocity_samples"] > 0
    assert row["imitation"]["samples"] == row["gait"]["samples"] == row["posture"]["samples"]
    for name in ("push_acc", "gait_acc", "posture_acc", "acc"):
        np.testing.assert_array_equal(getattr(tr_s, name).cpu().numpy().view(np.int32), getattr(tr_p, name).cpu().numpy().view(np.int32), err_msg=name)
    assert tuple(tr_s.imitation_acc.shape) == (8, engine.IMIT_NACC) and tr_p.imitation_acc is None


def test_a_captured_graph_follows_a_later_joint_map(tmp_path):
    """biped12: the launch is captured under one map; after `set_imitation_joints` the replay of the same graph compares with the new one."""
    import torch
    from open_duck_playground_amd import engine
    n, nu = 21, 12
    map_a = [11, 10, -1, 8, 7, 6, 5, 4, -1, 2, 1, 0]
    map_b = [-1, 3, 9, -1, 0, 1, 2, 15, 14, -1, 12, 5]
    model, b = _batch("biped12.xml", nu, n, str(tmp_path), map_a)
    kc = RC.home_pose(model, nu)
    rng = np.random.default_rng(77)
    T = 6
    priv = synthetic_rows(rng, T, n, b.nobs, b.npriv, nu)
    done = np.zeros((T, n), np.float32)
    done[3, ::4] = 1.0
    ended = np.concatenate([np.zeros((1, n)), (np.cumsum(done != 0, 0) > 0)[:-1]]).astype(np.float32)
    priv_d, done_d, ended_d = (torch.tensor(x, device="cuda") for x in (priv, done, ended))
    acc = torch.zeros(n, engine.IMIT_NACC, device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.imitation_accumulate(acc, tacc, PERIOD)      # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.imitation_accumulate(acc, tacc, PERIOD)

    def replayed():
        acc.zero_()
        for t in range(T):
            b.priv.copy_(priv_d[t]); b.done.copy_(done_d[t])
            tacc[:, engine.TRACK_ENDED] = ended_d[t]
            graph.replay()
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    for label, imap in (("captured map", map_a), ("later map", map_b)):
        b.set_imitation_joints(imap)
        want, absdp, _ = restate(priv, done, ended, b.nobs, nu, imap, kc, PERIOD)
        got = replayed()
        compare(got, want, absdp, f"graph, {label}")
        for u in range(nu):
            assert (got[:, engine.IMIT_POS_ERR_SQ + u].max() > 0) == (imap[u] >= 0), (label, u)
    b.close()


def test_refusals_launch_nothing(tmp_path):
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    n = 16
    L = engine.load_library()
    duck = load_task_model("flat_terrain")
    b = engine.Batch(duck, n, engine.default_config())
    b.reset(1)
    b.step(torch.zeros(n, 14, device="cuda"))
    pattern = torch.full((n, engine.IMIT_NACC), 3.25, device="cuda")
    acc = pattern.clone()
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")

    def raw(batch, period=PERIOD, null=None):
        bb = batch if batch is not None else b
        good = dict(priv_dev=bb.priv.data_ptr(), done_dev=bb.done.data_ptr(), truncation_dev=bb.truncation.data_ptr(), track_acc_dev=tacc.data_ptr(),
                    acc_dev=acc.data_ptr())
        a = {k: (None if k == null else C.c_void_p(v)) for k, v in good.items()}
        rc = L.odk_imitation_accumulate(batch._b if batch is not None else None, a["priv_dev"], a["done_dev"], a["truncation_dev"], a["track_acc_dev"],
                                        C.c_int(period), a["acc_dev"], bb._stream())
        return rc, L.odk_last_error().decode()

    # each null pointer, by name
    for null in ("acc_dev", "priv_dev", "done_dev", "truncation_dev", "track_acc_dev"):
        rc, msg = raw(b, null=null)
        assert rc == engine.ERR_INVALID and "odk_imitation_accumulate" in msg and null in msg, (null, msg)
    rc, msg = raw(None)
    assert rc == engine.ERR_INVALID and "odk_imitation_accumulate" in msg and "batch" in msg
    # a negative period
    rc, msg = raw(b, period=-1)
    assert rc == engine.ERR_INVALID and "period_steps = -1" in msg, msg
    with pytest.raises(engine.OdkError, match="odk_imitation_accumulate: period_steps = -3"):
        b.imitation_accumulate(acc, tacc, -3)
    # bad tensors are OdkErrors before anything is launched
    good_acc = torch.zeros(n, engine.IMIT_NACC, device="cuda")
    bad = [(torch.zeros(n, engine.IMIT_NACC - 1, device="cuda"), tacc), (torch.zeros(n, engine.IMIT_NACC), tacc), (good_acc.double(), tacc),
           (good_acc, torch.zeros(n, engine.TRACK_NACC + 1, device="cuda")), (good_acc, tacc.cpu())]
    for args in bad:
        with pytest.raises(engine.OdkError, match="imitation_accumulate"):
            b.imitation_accumulate(*args, PERIOD)
    # the imitation reward off: the frame is all zeros
    cfg = engine.default_config()
    cfg.use_imitation = 0
    b.set_config(cfg)
    rc, msg = raw(b)
    assert rc == engine.ERR_INVALID and "use_imitation = 0" in msg, msg
    with pytest.raises(engine.OdkError, match="odk_imitation_accumulate: use_imitation = 0"):
        b.imitation_accumulate(acc, tacc, PERIOD)
    b.set_config(engine.default_config())
    # the Standing task: no frame in the row
    st = engine.Batch(duck, n, engine.default_config(standing=True))
    rc, msg = raw(st)
    assert rc == engine.ERR_INVALID and "Standing" in msg and "frame" in msg, msg
    st.close()
    # a robot that is not the duck, before it is given a map
    _, other = _batch("biped12.xml", 12, n, str(tmp_path), None)
    rc, msg = raw(other)
    assert rc == engine.ERR_INVALID and "no imitation joint map" in msg and "odk_batch_set_imitation_joints" in msg, msg
    with pytest.raises(engine.OdkError, match="no imitation joint map"):
        other.imitation_accumulate(acc, tacc, PERIOD)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy().view(np.int32), pattern.cpu().numpy().view(np.int32))      # untouched by every refusal
    # ... and the good calls count: the other robot once it has a map (an all -1 map compares nothing), the duck
    acc.zero_()
    other.set_imitation_joints([-1] * 12)
    other.imitation_accumulate(acc, tacc, 0)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    SAMPLES, JOINT_POS_SQ_SUM = engine.IMIT_SAMPLES, engine.IMIT_JOINT_POS_SQ_SUM
    assert np.all(got[:, SAMPLES] == 1.0) and np.all(got[:, engine.IMIT_POS_ERR_SUM:] == 0.0) and np.all(got[:, JOINT_POS_SQ_SUM] == 0.0)
    other.close()
    acc.zero_()
    b.imitation_accumulate(acc, tacc, PERIOD)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    live = got[:, SAMPLES] > 0
    assert live.any() and np.all(got[live, JOINT_POS_SQ_SUM] > 0.0)
    b.close()
