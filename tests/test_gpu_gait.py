"""GPU checks of the gait and actuator-load accumulator (odk_gait_accumulate / Batch.gait_accumulate) and of `track --gait`: every slot
against a float64 numpy restatement on synthetic privileged rows (three robots: nu 14, 15 and 16; a tail wave; a partial block), the report
of a real run against the same restatement over the recorded outputs, eager against graph, with and without pushes, and the refusals."""
import json

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

G = RC.HEADER         # include/odk.h's constants, by engine's names


def restate(priv, done, ended, nobs, nu, limit):
    """odk_gait_accumulate restated in float64 over float32 inputs: priv [T, n, npriv], done [T, n], ended [T, n] (the tracking accumulator's
    ENDED column as the launch of step t saw it), limit [nu] float32 or None.  Returns the [n, 144] accumulator."""
    T, n = done.shape
    A = np.zeros((n, G.GAIT_NACC), np.float64)
    lim32 = None if limit is None else np.float32(limit)
    lanes = lambda slot: slice(slot, slot + nu)      # a per-actuator array's live entries
    for e in range(n):
        prev, air, N = [False, False], [0, 0], 0
        R = A[e]
        for t in range(T):
            if ended[t, e] != 0 or done[t, e] != 0:
                continue
            P32 = priv[t, e]
            P = P32.astype(np.float64)
            Q = P[nobs:]
            a1, a2 = P[13 + 2 * nu:13 + 3 * nu], P[13 + 3 * nu:13 + 4 * nu]
            q, v, h, f = Q[15:15 + nu], Q[15 + nu:15 + 2 * nu], Q[15 + 2 * nu], Q[16 + 2 * nu:16 + 3 * nu]
            con = Q[16 + 3 * nu:18 + 3 * nu] != 0
            fv = Q[18 + 3 * nu:24 + 3 * nu].reshape(2, 3)
            R[G.GAIT_SAMPLES] += 1
            R[G.GAIT_SPEED_SUM] += np.hypot(Q[9], Q[10])
            R[G.GAIT_ABS_POWER_SUM] += np.abs(f * v).sum()
            R[G.GAIT_DOUBLE] += con[0] and con[1]
            R[G.GAIT_FLIGHT] += (not con[0]) and (not con[1])
            for k in range(2):
                if con[k]:
                    R[G.GAIT_CONTACT + k] += 1
                    R[G.GAIT_SLIP_SUM + k] += np.hypot(fv[k, 0], fv[k, 1])
                    if N > 0 and not prev[k]:
                        R[G.GAIT_TOUCHDOWNS + k] += 1
                        R[G.GAIT_SWING_STEPS_SUM + k] += air[k]
                    air[k] = 0
                else:
                    air[k] += 1
                prev[k] = bool(con[k])
                R[G.GAIT_PREV_CONTACT + k], R[G.GAIT_AIR_RUN + k] = prev[k], air[k]
            R[G.GAIT_HEIGHT_SUM] += h
            R[G.GAIT_HEIGHT_SQ_SUM] += h * h
            R[G.GAIT_ROLLPITCH_RATE_SQ_SUM] += Q[0] * Q[0] + Q[1] * Q[1]
            R[G.GAIT_ACTION_RATE_SUM] += ((a1 - a2) ** 2).sum()
            R[lanes(G.GAIT_TORQUE_SQ)] += f * f
            R[lanes(G.GAIT_TORQUE_PEAK)] = np.maximum(R[lanes(G.GAIT_TORQUE_PEAK)], np.abs(f))
            R[lanes(G.GAIT_VEL_PEAK)] = np.maximum(R[lanes(G.GAIT_VEL_PEAK)], np.abs(v))
            if lim32 is not None:      # the comparison as the kernel makes it, in float32
                f32 = np.abs(P32[nobs + 16 + 2 * nu:nobs + 16 + 3 * nu])
                R[lanes(G.GAIT_SAT)] += (lim32 > 0) & (f32 >= np.float32(0.99) * lim32)
            R[lanes(G.GAIT_ABS_POWER)] += np.abs(f * v)
            R[lanes(G.GAIT_RANGE_MIN)] = q if N == 0 else np.minimum(R[lanes(G.GAIT_RANGE_MIN)], q)
            R[lanes(G.GAIT_RANGE_MAX)] = q if N == 0 else np.maximum(R[lanes(G.GAIT_RANGE_MAX)], q)
            N += 1
    return A


def compare(got, want, nu, label):
    """Counts, peaks, ranges and bookkeeping exact; the float32 running sums, all of non-negative terms, within RC.compare_sums' bound."""
    sums = [G.GAIT_SPEED_SUM, G.GAIT_ABS_POWER_SUM, G.GAIT_SLIP_SUM, G.GAIT_SLIP_SUM + 1, G.GAIT_HEIGHT_SUM, G.GAIT_HEIGHT_SQ_SUM,
            G.GAIT_ROLLPITCH_RATE_SQ_SUM, G.GAIT_ACTION_RATE_SUM] + [s + u for s in (G.GAIT_TORQUE_SQ, G.GAIT_ABS_POWER) for u in range(nu)]
    RC.compare_sums(got, want, G.GAIT_SAMPLES, {c: want[:, c] for c in sums}, label)


CONTACT_HEAD = [0, 1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1]     # a touchdown on the second sample, then back-to-back swings of length 1, then one of 3


@pytest.mark.parametrize("robot,nu,null_limit", [("duck", 14, False), ("tail_biped.xml", 15, False), ("biped_arms.xml", 16, True)])
def test_every_slot_matches_a_numpy_restatement_on_synthetic_rows(robot, nu, null_limit):
    """37 envs (two full waves of four rows... and a tail wave with one live row; three blocks of 16 envs, the last one partial), 24 steps of
    seeded random privileged rows written straight into the batch's outputs -- no odk_step.  Contact per foot follows one of four scripts
    (CONTACT_HEAD then random; never; always; random), first episodes end at step 0, mid-run or never, by done with and without truncation,
    and the test sets the tracking accumulator's ENDED column as odk_tracking_accumulate would have."""
    import torch
    n, T = N_ENVS, T_STEPS
    env = RC.robot_env(robot, n)
    b = env.batch
    assert b.model.nu == nu
    nobs, npriv = b.nobs, b.npriv
    assert tuple(b.priv.shape) == (n, npriv) and nobs + 24 + 3 * nu <= npriv
    priv, done, trunc, ended, end_at, limit = synthetic_inputs(nobs, npriv, nu, null_limit)
    want = restate(priv, done, ended, nobs, nu, limit)

    lim_dev = None if limit is None else torch.tensor(limit, device="cuda")
    got, guard_tail, snaps = RC.drive_rows(b, lambda acc, tacc: b.gait_accumulate(acc, tacc, lim_dev), G.GAIT_NACC, priv, done, trunc, ended)
    compare(got, want, nu, f"{robot} nu={nu}")
    np.testing.assert_array_equal(guard_tail, 7.0)
    RC.assert_frozen_after_end(snaps, end_at)
    # the run covers what it claims to
    N = want[:, G.GAIT_SAMPLES]
    assert set(N.astype(int)) == {0, 11, 17, T}
    assert np.all(got[N == 0] == 0.0)
    first = [e for e in range(n) if e % 4 == 0 and N[e] >= 11]      # left foot on the scripted sequence
    assert first and all(want[e, G.GAIT_TOUCHDOWNS] >= 4 and want[e, G.GAIT_SWING_STEPS_SUM] >= 4 for e in first)
    never = [e for e in range(n) if e % 4 == 1 and N[e] > 0]
    assert never and all(want[e, G.GAIT_CONTACT] == 0 and want[e, G.GAIT_TOUCHDOWNS] == 0 and want[e, G.GAIT_AIR_RUN] == N[e] for e in never)
    always = [e for e in range(n) if e % 4 == 2 and N[e] > 0]
    assert always and all(want[e, G.GAIT_CONTACT] == N[e] and want[e, G.GAIT_TOUCHDOWNS] == 0 and want[e, G.GAIT_AIR_RUN] == 0 for e in always)
    assert (want[:, G.GAIT_DOUBLE] > 0).any() and (want[:, G.GAIT_FLIGHT] > 0).any()
    SAT = G.GAIT_SAT
    if null_limit:
        assert np.all(got[:, SAT:SAT + G.GAIT_STRIDE] == 0.0)
    else:
        assert want[0, SAT] >= 1 and np.all(want[:, SAT + 1] == 0) and np.all(want[:, SAT + 3] == 0) and want[:, SAT + 2].sum() > want[:, SAT].sum()
    b.close()


N_ENVS, T_STEPS = 37, 24


def synthetic_inputs(nobs, npriv, nu, null_limit):
    """The host half of the synthetic test, a function of the sizes alone: (priv [T, n, npriv], done, trunc, ended [T, n], end_at [n], limit
    [nu] or None)."""
    n, T = N_ENVS, T_STEPS
    rng = np.random.default_rng(100 + nu)
    priv = rng.normal(0.0, 1.0, (T, n, npriv)).astype(np.float32)
    priv[:, :, nobs + 15 + 2 * nu] = rng.uniform(0.1, 0.2, (T, n)).astype(np.float32)          # a root height is positive
    scripts = np.zeros((4, T), np.float32)
    scripts[0, :len(CONTACT_HEAD)] = CONTACT_HEAD
    scripts[0, len(CONTACT_HEAD):] = rng.integers(0, 2, T - len(CONTACT_HEAD))
    scripts[2] = 1.0
    for e in range(n):
        for k, s in enumerate((e % 4, (e // 4) % 4)):
            priv[:, e, nobs + 16 + 3 * nu + k] = rng.integers(0, 2, T) if s == 3 else scripts[s]
    # first episodes: never ending; done at step 0 without / with truncation; done mid-run without / with truncation
    end_at, done, trunc, ended = RC.first_episodes(rng, T, n, ends=(T + 1, 0, 0, 11, 17), truncated=(2, 4))
    limit = None
    if not null_limit:
        limit = np.ones(nu, np.float32)
        limit[1], limit[2], limit[3] = 0.0, 0.5, 100.0               # never counted; saturates often; never reached
        sat = np.float32(0.99) * np.float32(1.0)
        fcol = nobs + 16 + 2 * nu
        priv[1, 0, fcol] = sat                                       # exactly at the threshold: counted
        priv[1, 4, fcol] = -np.nextafter(sat, np.float32(0))         # one ulp under it: not counted
        priv[2, 0, fcol + 1] = 50.0                                  # a large force on the actuator without a limit
    return priv, done, trunc, ended, end_at, limit


def test_track_gait_end_to_end(tmp_path, monkeypatch):
    """A randomly initialised policy on the duck, two commands, 8 envs each, 40 steps.  The eager run's recording, pushed through the numpy
    restatement and `reduce_gait`, reproduces the accumulator (the bounds of the synthetic test) and the report; the graph run's gait
    accumulator has the eager run's bits; without --gait the tracking accumulator has the same bits and the report its old keys."""
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 8, 40
    out = tmp_path / "report.json"
    argv = ["--checkpoint", ckpt, "--command", "0.1", "0", "0", "--command", "0", "0", "0.5", "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "1", "--output", str(out)]
    rep_e, tr_e, hist = RC.run_track(track, monkeypatch, argv + ["--gait"], eager=True)
    assert not rep_e["settings"]["graph"] and rep_e["settings"]["gait"] is True and len(hist) == T
    priv, done = np.stack([h[0] for h in hist]), np.stack([h[1] for h in hist])
    ended = np.concatenate([np.zeros((1, 2 * E)), (np.cumsum(done != 0, 0) > 0)[:-1]]).astype(np.float32)
    model = tr_e.env.mj_model
    nobs = tr_e.env.batch.nobs
    limit = track.torque_limits(model)
    want = restate(priv, done, ended, nobs, 14, limit)
    got_e = tr_e.gait_acc.cpu().numpy()
    compare(got_e, want, 14, "track --gait, eager")
    track_e = tr_e.acc.cpu().numpy()
    np.testing.assert_array_equal(got_e[:, engine.GAIT_SAMPLES], track_e[:, engine.TRACK_SAMPLES])     # a gait sample is a velocity sample
    assert got_e[:, engine.GAIT_SAMPLES].sum() > 0

    # the report is reduce_gait of that accumulator; against the restatement every figure is a ratio of two sums (or its root): twice the sum bound
    tol = 2 * (T + 4) * 2.0 ** -23
    ref = track.reduce_gait(want, rep_e["commands"], E, rep_e["settings"]["dt"], model)
    names = [str(x) for x in model.a["names_actuator"]]
    for row, w in zip(rep_e["commands"], ref):
        assert tuple(row) == track.ROW_KEYS + ("gait",)
        g = row["gait"]
        assert tuple(g) == track.GAIT_KEYS and list(g["actuators"]) == names and g["samples"] == w["samples"] > 0
        flat_g, flat_w = _flatten(g), _flatten(w)
        assert list(flat_g) == list(flat_w)
        for k in flat_g:
            if k == "root_height_std":      # a difference of two means: the bound applies to the variance, at the scale of the mean square
                ms = w["root_height_mean"] ** 2 + w["root_height_std"] ** 2
                assert abs(flat_g[k] ** 2 - flat_w[k] ** 2) <= 2 * tol * ms, (k, flat_g[k], flat_w[k])
            elif flat_w[k] is None:
                assert flat_g[k] is None, k
            else:
                assert flat_g[k] == pytest.approx(flat_w[k], rel=tol, abs=0), (k, flat_g[k], flat_w[k])
        assert g["actuators"][names[0]]["torque_limit"] == float(limit[0])
    assert json.load(open(out)) == json.loads(json.dumps(rep_e))

    # the graph: one more launch in the captured step, the same bits
    rep_g, tr_g, _ = RC.run_track(track, monkeypatch, argv + ["--gait"])
    assert rep_g["settings"]["graph"]
    np.testing.assert_array_equal(tr_g.gait_acc.cpu().numpy().view(np.int32), got_e.view(np.int32))
    np.testing.assert_array_equal(tr_g.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    assert [r["gait"] for r in rep_g["commands"]] == [r["gait"] for r in rep_e["commands"]]

    # without --gait: no accumulator, no launch, the old report, the same tracking bits
    calls = []
    real = engine.Batch.gait_accumulate
    monkeypatch.setattr(engine.Batch, "gait_accumulate", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    rep_p, tr_p, _ = RC.run_track(track, monkeypatch, argv)
    assert calls == [] and tr_p.gait_acc is None and tr_p.torque_limit is None
    np.testing.assert_array_equal(tr_p.acc.cpu().numpy().view(np.int32), track_e.view(np.int32))
    assert tuple(rep_p) == track.REPORT_KEYS and "gait" not in rep_p["settings"]
    assert all(tuple(r) == track.ROW_KEYS for r in rep_p["commands"])
    assert [k for k in rep_g["settings"] if k not in rep_p["settings"]] == ["gait"]
    for a, bb in zip(rep_p["commands"], rep_g["commands"]):
        assert a == {k: v for k, v in bb.items() if k != "gait"}


def _flatten(g):
    flat = {}
    for k, v in g.items():
        if k == "actuators":
            for nm, a in v.items():
                for kk, vv in a.items():
                    for i, x in enumerate(vv if isinstance(vv, list) else [vv]):
                        flat[f"{nm}.{kk}.{i}"] = x
        else:
            for i, x in enumerate(v if isinstance(v, list) else [v]):
                flat[k if not isinstance(v, list) else f"{k}.{i}"] = x
    return flat


def test_track_gait_with_a_push_grid(tmp_path, monkeypatch):
    """One command, two pushes, 4 envs per cell: every cell and the command row get a "gait" object, the cells' samples add up to the row's,
    and the push and tracking accumulators have the bits of a run without --gait."""
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    argv = ["--checkpoint", ckpt, "--command", "0.1", "0", "0", "--push", "0", "0", "--push", "1.5", "0", "--push_at", "10", "--envs_per_command", "4",
            "--episode_length", "40", "--seed", "2", "--output", str(tmp_path / "r.json")]
    rep_g, tr_g, _ = RC.run_track(track, monkeypatch, argv + ["--gait"])
    rep_p, tr_p, _ = RC.run_track(track, monkeypatch, argv)
    assert rep_g["settings"]["gait"] is True and "gait" not in rep_p["settings"]
    (row,), (plain,) = rep_g["commands"], rep_p["commands"]
    assert tuple(row) == track.ROW_KEYS + track.PUSH_ROW_KEYS + ("gait",) and tuple(plain) == track.ROW_KEYS + track.PUSH_ROW_KEYS
    assert len(row["pushes"]) == 2
    for cell, old in zip(row["pushes"], plain["pushes"]):
        assert tuple(cell) == track.PUSH_CELL_KEYS + ("gait",) and tuple(cell["gait"]) == track.GAIT_KEYS
        assert {k: v for k, v in cell.items() if k != "gait"} == old
    assert sum(c["gait"]["samples"] for c in row["pushes"]) == row["gait"]["samples"] == row["velocity_samples"] > 0
    np.testing.assert_array_equal(tr_g.push_acc.cpu().numpy().view(np.int32), tr_p.push_acc.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(tr_g.acc.cpu().numpy().view(np.int32), tr_p.acc.cpu().numpy().view(np.int32))
    assert tuple(tr_g.gait_acc.shape) == (8, engine.GAIT_NACC) and tr_p.gait_acc is None


def test_refusals_launch_nothing():
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine, joystick
    n = 16
    env = joystick.Joystick(task="flat_terrain", num_envs=n)
    b = env.batch
    L = engine.load_library()
    env.reset(1)
    b.step(torch.zeros(n, 14, device="cuda"))
    acc = torch.zeros(n, engine.GAIT_NACC, device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    lim = torch.ones(14, device="cuda")
    good = dict(priv_dev=b.priv.data_ptr(), done_dev=b.done.data_ptr(), truncation_dev=b.truncation.data_ptr(), track_acc_dev=tacc.data_ptr(),
                torque_limit_dev=lim.data_ptr(), acc_dev=acc.data_ptr())
    for null in ("acc_dev", "priv_dev", "done_dev", "truncation_dev", "track_acc_dev"):
        a = {k: (None if k == null else C.c_void_p(v)) for k, v in good.items()}
        rc = L.odk_gait_accumulate(b._b, a["priv_dev"], a["done_dev"], a["truncation_dev"], a["track_acc_dev"], a["torque_limit_dev"], a["acc_dev"], b._stream())
        assert rc == engine.ERR_INVALID, null
        msg = L.odk_last_error().decode()
        assert "odk_gait_accumulate" in msg and null in msg, msg
    assert L.odk_gait_accumulate(None, *[C.c_void_p(v) for v in good.values()], b._stream()) == engine.ERR_INVALID
    assert "batch" in L.odk_last_error().decode()
    # the Python surface: bad accumulators and bad limits are OdkErrors before anything is launched
    bad = [(torch.zeros(n, engine.GAIT_NACC - 1, device="cuda"), tacc, lim), (torch.zeros(n, engine.GAIT_NACC), tacc, lim), (acc.double(), tacc, lim),
           (acc, torch.zeros(n, engine.TRACK_NACC + 1, device="cuda"), lim), (acc, tacc.cpu(), lim),
           (acc, tacc, torch.ones(13, device="cuda")), (acc, tacc, torch.ones(14)), (acc, tacc, lim.double()), (acc, tacc, np.ones(14, np.float32))]
    for args in bad:
        with pytest.raises(engine.OdkError, match="gait_accumulate"):
            b.gait_accumulate(*args)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy(), 0.0)
    # needs no bound commands or pushes; the optional limit may be left out
    assert b.commands is None and b.pushes is None
    b.gait_accumulate(acc, tacc)
    b.gait_accumulate(acc, tacc, lim)
    torch.cuda.synchronize()
    assert float(acc[:, engine.GAIT_SAMPLES].sum()) > 0.0
    b.close()
