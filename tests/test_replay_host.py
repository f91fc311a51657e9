"""Host checks of the log replay (open_duck_playground_amd/replay.py; no GPU, no torch): the log readers and their refusals, the alignment
a_k = O_{k+1}[last_act] and the canonical table, the float32 restatements of odk_log_apply / odk_replay_accumulate on hand-made rows, score
and ranking, the cross-entropy search on a synthetic bowl, the command line's refusals, the two symbols and their constants against
include/odk.h, and the committed oracle log against a fresh run of the float64 oracle."""
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from open_duck_playground_amd import engine, replay, track

NU = 14
F = replay.obs_fields(NU)


def _rows(T=6, nu=NU, env="joystick", seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.3, size=(T, replay.obs_width(nu, env))).astype(np.float32)


def test_readers(tmp_path):
    rows = _rows()
    for name in ("log.pkl", "log.npz"):
        p = str(tmp_path / name)
        replay.write_log(p, rows)
        back = replay.read_log(p)
        assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), rows.view(np.int32))
    data = pickle.load(open(tmp_path / "log.pkl", "rb"))      # the reference's format: a list of one 1-D array per control step
    assert isinstance(data, list) and len(data) == 6 and data[0].shape == (101,)
    # float64 rows (mujoco_infer.py's own) are read too
    with open(tmp_path / "f64.pkl", "wb") as f:
        pickle.dump([r.astype(np.float64) for r in rows], f)
    assert np.array_equal(replay.read_log(str(tmp_path / "f64.pkl")), rows)
    # the safe unpickler: numpy reconstructors only
    with open(tmp_path / "evil.pkl", "wb") as f:
        pickle.dump([os.getcwd], f)
    with pytest.raises(ValueError, match="refused"):
        replay.read_log(str(tmp_path / "evil.pkl"))
    np.savez(tmp_path / "other.npz", observations=rows)
    with pytest.raises(ValueError, match="`obs` array"):
        replay.read_log(str(tmp_path / "other.npz"))
    with open(tmp_path / "ragged.pkl", "wb") as f:
        pickle.dump([rows[0], rows[1][:50]], f)
    with pytest.raises(ValueError, match="differ in length"):
        replay.read_log(str(tmp_path / "ragged.pkl"))
    bad = rows.copy(); bad[2, 3] = np.nan
    replay.write_log(str(tmp_path / "nan.npz"), bad)
    with pytest.raises(ValueError, match="not finite"):
        replay.read_log(str(tmp_path / "nan.npz"))


def test_width_refusals_name_both_widths():
    assert (replay.obs_width(14), replay.obs_width(14, "standing"), replay.obs_width(12), replay.obs_width(12, "standing")) == (101, 85, 89, 75)
    assert replay.obs_width(14) == 17 + 6 * 14 and replay.obs_width(14, "standing") == 15 + 5 * 14
    with pytest.raises(ValueError, match=r"85 floats wide.*observes 101.*--env standing observes 85"):
        replay.log_table(_rows(env="standing"), 14, "joystick")
    with pytest.raises(ValueError, match=r"101 floats wide.*standing env.*observes 85.*--env joystick observes 101"):
        replay.log_table(_rows(), 14, "standing")
    with pytest.raises(ValueError, match=r"101 floats wide.*12 actuators observes 89"):
        replay.log_table(_rows(), 12)
    with pytest.raises(ValueError, match="replays no step"):
        replay.log_table(_rows(T=1), 14)


@pytest.mark.parametrize("env,nu", [("joystick", 14), ("standing", 14), ("joystick", 12)])
def test_alignment_and_canonical_table(env, nu):
    """a log of T rows replays T - 1 steps; row k of the table is what O_{k+1} shows: a_k = O_{k+1}[last_act]"""
    rows = _rows(T=7, nu=nu, env=env)
    f, o = replay.obs_fields(nu, env), engine.log_offsets(nu)
    t = replay.log_table(rows, nu, env)
    assert t.shape == (6, engine.log_row(nu)) == (6, 15 + 3 * nu) and t.dtype == np.float32
    assert f["contact"] + 2 + (2 if env == "joystick" else 0) == rows.shape[1]      # the layout ends where the row does (Joystick: + the phase)
    for k in range(6):
        nxt = rows[k + 1]
        assert np.array_equal(t[k, 7:7 + nu], nxt[f["last_act"]:f["last_act"] + nu])
        assert np.array_equal(t[k, 0:7], nxt[6:13])
        assert np.array_equal(t[k, o["pos"]:o["pos"] + nu], nxt[13:13 + nu])
        assert np.array_equal(t[k, o["gyro"]:o["gyro"] + 3], nxt[0:3]) and np.array_equal(t[k, o["accel"]:o["accel"] + 3], nxt[3:6])
        assert np.array_equal(t[k, o["contact"]:o["contact"] + 2], nxt[f["contact"]:f["contact"] + 2])
        # the velocity column is the logged float32 itself, bit for bit
        assert np.array_equal(t[k, o["vel"]:o["vel"] + nu].view(np.int32), nxt[13 + nu:13 + 2 * nu].view(np.int32))
    assert o == {"command": 0, "action": 7, "pos": 7 + nu, "vel": 7 + 2 * nu, "gyro": 7 + 3 * nu, "accel": 10 + 3 * nu, "contact": 13 + 3 * nu}


def test_why_the_velocity_is_not_unscaled_on_the_host():
    """x 0.05 in float32 maps neighbouring floats onto one another, so obs / 0.05 does not give the velocity back: a plant replayed on its
    own log would not score 0.  The kernel multiplies the privileged velocity by dof_vel_scale instead, which has the logged bits."""
    s = np.float32(0.05)
    v = np.random.default_rng(0).uniform(-5, 5, size=20000).astype(np.float32)
    back = ((v * s).astype(np.float32) / s).astype(np.float32)
    share = float((back != v).mean())
    assert 0.02 < share < 0.5, share
    assert np.array_equal((v * s).astype(np.float32), (v * s).astype(np.float32))


def test_as_logged_puts_the_action_of_step_k_into_row_k_plus_1():
    nu = NU
    first = np.zeros(101, np.float32); first[F["last_act"]:F["last_act"] + nu] = -1; first[F["last_last_act"]:F["last_last_act"] + nu] = -2
    first[F["last_last_last_act"]:F["last_last_last_act"] + nu] = -3
    acts = np.arange(4, dtype=np.float32)[:, None] * np.ones((1, nu), np.float32)
    obs = np.full((4, 101), 7.0, np.float32)
    rows = replay.as_logged(first, obs, acts, nu)
    assert rows.shape == (5, 101) and np.array_equal(rows[0], first)
    la = lambda k, name: rows[k, F[name]]
    assert [la(k, "last_act") for k in range(1, 5)] == [0, 1, 2, 3]
    assert [la(k, "last_last_act") for k in range(1, 5)] == [-1, 0, 1, 2]
    assert [la(k, "last_last_last_act") for k in range(1, 5)] == [-2, -1, 0, 1]
    assert rows[2, 0] == 7.0 and rows[2, F["motor_targets"]] == 7.0
    assert np.array_equal(replay.log_table(rows, nu)[:, 7:7 + nu], acts)


def test_excitation_is_the_issues():
    a = replay.excitation(14, 60, 0)
    assert a.shape == (60, 14) and a.dtype == np.float32 and np.abs(a).max() <= 0.3
    rng = np.random.default_rng(0)
    hz, ph = rng.uniform(0.5, 2.0, size=14), rng.uniform(0, 2 * np.pi, size=14)
    k = 30
    np.testing.assert_allclose(a[k], 0.3 * np.sin(2 * np.pi * hz * k * 0.02 + ph), atol=1e-6)      # past the ramp
    np.testing.assert_allclose(a[4], 0.3 * (5 / 25) * np.sin(2 * np.pi * hz * 4 * 0.02 + ph), atol=1e-6)
    assert np.array_equal(a, replay.excitation(14, 60, 0)) and not np.array_equal(a, replay.excitation(14, 60, 1))


def _track(n):
    return np.zeros((n, engine.TRACK_NACC), np.float32)


def test_log_apply_restatement_clock_and_clamp():
    table = replay.log_table(_rows(T=5), NU)      # 4 rows
    tr = _track(6)
    tr[:, engine.TRACK_STEPS] = [0, 2, 3, 4, 9, 3]      # 3: the last row; 4, 9: past the end, clamped
    tr[5, engine.TRACK_ENDED] = 1                      # ended in step 2 (STEPS - 1): keeps that row
    act, cmd = replay.log_apply_np(table, tr)
    for e, k in enumerate([0, 2, 3, 3, 3, 2]):
        assert np.array_equal(act[e], table[k, 7:7 + NU]) and np.array_equal(cmd[e], table[k, 0:7]), e
    tr[0, engine.TRACK_ENDED], tr[0, engine.TRACK_STEPS] = 1, 0      # (cannot happen -- ENDED implies STEPS >= 1 -- and still reads inside the table)
    assert np.array_equal(replay.log_apply_np(table, tr)[0][0], table[0, 7:7 + NU])


def test_replay_accumulate_restatement_on_hand_made_rows():
    nu, nobs, npriv = NU, 101, 212
    rows = np.zeros((4, nobs), np.float32)      # 3 table rows
    rows[1:, F["pos"]:F["pos"] + nu] = 0.25
    rows[1:, F["vel"]:F["vel"] + nu] = 0.5       # observation units: 10 rad/s
    rows[1:, 0:3] = 1.0; rows[1:, 3:6] = 2.0
    rows[1:, F["contact"]:F["contact"] + 2] = (1.0, 0.0)
    table = replay.log_table(rows, nu)
    n = 5
    priv = np.zeros((n, npriv), np.float32)
    priv[:, nobs + 15:nobs + 15 + nu] = 0.75                      # dp = 0.5
    priv[:, nobs + 15 + nu:nobs + 15 + 2 * nu] = 30.0             # x 0.05 = 1.5: dv = 1.0 in observation units
    priv[:, nobs:nobs + 3] = 3.0; priv[:, nobs + 3:nobs + 6] = 5.0      # dg = 2, da = 3
    priv[:, nobs + 16 + 3 * nu:nobs + 18 + 3 * nu] = (1.0, 1.0)   # foot 0 agrees, foot 1 does not
    tr = _track(n); done = np.zeros(n, np.float32)
    tr[:, engine.TRACK_STEPS] = [0, 2, 3, 1, 1]      # env 2: k >= nrow
    tr[3, engine.TRACK_ENDED] = 1                    # env 3: past its first episode
    done[4] = 1                                      # env 4: this step ends the episode (the observation is the auto-reset's)
    acc = np.zeros((n, 16, engine.REPLAY_NSLOT), np.float32)
    acc[2:] = 7.0                                    # what must keep its bits
    out = replay.replay_accumulate_np(acc, priv, done, tr, table, nobs, 0.05)
    assert out is acc and (acc[2:] == 7.0).all()
    for e in (0, 1):
        A = acc[e]
        assert (A[:nu, engine.REPLAY_POS_ERR_SUM] == 0.5).all() and (A[:nu, engine.REPLAY_POS_ERR_SQ] == 0.25).all()
        assert (A[:nu, engine.REPLAY_POS_ERR_PEAK] == 0.5).all()
        np.testing.assert_allclose(A[:nu, engine.REPLAY_VEL_ERR_SQ], 1.0, rtol=1e-6)
        assert (A[:3, engine.REPLAY_GYRO_ERR_SQ] == 4.0).all() and (A[:3, engine.REPLAY_ACCEL_ERR_SQ] == 9.0).all()
        assert A[0, engine.REPLAY_CONTACT_AGREE] == 1.0 and A[1, engine.REPLAY_CONTACT_AGREE] == 0.0 and A[0, engine.REPLAY_SAMPLES] == 1.0
        assert not A[nu:].any() and not A[3:, engine.REPLAY_GYRO_ERR_SQ].any() and not A[1:, engine.REPLAY_SAMPLES].any()
    replay.replay_accumulate_np(acc, priv, done, tr, table, nobs, 0.05)      # a second sample: sums add, the peak stays
    assert acc[0, 0, engine.REPLAY_POS_ERR_SUM] == 1.0 and acc[0, 0, engine.REPLAY_POS_ERR_PEAK] == 0.5 and acc[0, 0, engine.REPLAY_SAMPLES] == 2.0
    # the score of it: pos 0.25 + vel (1.0 / 0.05^2 rad^2/s^2) x 0.05^2
    s = replay.score(acc[:2], nu, 0.05)
    np.testing.assert_allclose(s, 0.25 + 1.0, rtol=1e-6)
    m = replay.channel_means(acc[:2], nu, 0.05)
    np.testing.assert_allclose(m["vel"], 400.0, rtol=1e-6); np.testing.assert_allclose(m["gyro"], 4.0); np.testing.assert_allclose(m["contact"], 0.5)
    np.testing.assert_allclose(replay.score(acc[:2], nu, 0.05, replay.parse_weights(["gyro=2", "vel=0", "contact=1"], 0.05)), 0.25 + 8.0 + 0.5, rtol=1e-6)
    j = replay.joint_report(acc[0], nu, 0.05, [f"j{u}" for u in range(nu)])
    assert len(j) == nu and j[3]["joint"] == "j3" and j[3]["pos_rms"] == 0.5 and j[3]["pos_bias"] == 0.5 and j[3]["pos_peak"] == 0.5
    np.testing.assert_allclose(j[3]["vel_rms"], 20.0, rtol=1e-6)


def test_score_of_an_env_without_a_sample_and_default_weights():
    acc = np.zeros((2, 16, engine.REPLAY_NSLOT), np.float32)
    acc[1, 0, engine.REPLAY_SAMPLES] = 3
    s = replay.score(acc, NU, 0.05)
    assert np.isinf(s[0]) and s[1] == 0.0
    w = replay.default_weights(0.05)
    assert w["pos"] == 1.0 and w["vel"] == 0.05 ** 2 and w["gyro"] == w["accel"] == w["contact"] == 0.0
    for bad in (["speed=1"], ["pos"], ["pos=-1"], ["pos=x"], ["pos=inf"]):
        with pytest.raises(ValueError, match="--weight"):
            replay.parse_weights(bad, 0.05)


def test_ranking_is_lexicographic():
    """a candidate that ended early ranks behind every one that lasted, whatever its score; among the early enders the longer survivor first"""
    scores = [5.0, 0.0, 1.0, 0.5, 0.1, 3.0]
    lasted = [True, False, True, False, False, True]
    steps = [60, 10, 60, 40, 40, 60]
    assert replay.rank_order(scores, lasted, steps).tolist() == [2, 5, 0, 4, 3, 1]
    tr = _track(3)
    tr[:, engine.TRACK_STEPS] = [60, 17, 60]; tr[1, engine.TRACK_ENDED] = 1; tr[2, engine.TRACK_ENDED] = 1      # env 2 ended IN the last step
    l, s = replay.survival(tr, 60)
    assert l.tolist() == [True, False, False] and s.tolist() == [60, 17, 60]


def test_cem_finds_the_cell_of_a_quadratic_bowl_with_a_categorical_axis():
    true = dict(kp=0.8, frictionloss=1.5, delay=1)
    calls = []

    def evaluate(c):
        calls.append({k: np.array(v) for k, v in c.items()})
        s = (c["kp"] - true["kp"]) ** 2 + 0.1 * (c["frictionloss"] - true["frictionloss"]) ** 2 + 0.05 * (c["delay"] != true["delay"])
        lasted = c["kp"] > 0.55                      # the weakest plants fall, the sooner the weaker
        return s, lasted, np.where(lasted, 60, (c["kp"] * 100).astype(int))
    axes = replay.parse_fit("kp=0.5:1.5,frictionloss=0.3:3,delay=0:2")
    res = replay.cem(evaluate, axes, 256, 6, seed=0)
    b = res["best"]
    assert b["plant"]["delay"] == 1 and abs(b["plant"]["kp"] - 0.8) < 0.02 and abs(b["plant"]["frictionloss"] - 1.5) < 0.1 and b["lasted"]
    assert len(res["history"]) == 6 == len(calls) and all(len(c["kp"]) == 256 for c in calls)
    g0 = calls[0]      # generation 0: uniform in the box, the delay over its three values
    assert g0["kp"].min() >= 0.5 and g0["kp"].max() <= 1.5 and g0["kp"].std() > 0.25 and set(g0["delay"].tolist()) == {0, 1, 2}
    for c in calls:    # clipped to the box
        assert c["kp"].min() >= 0.5 and c["frictionloss"].max() <= 3.0 and c["frictionloss"].min() >= 0.3
    assert res["history"][-1]["elite_std"]["kp"] < res["history"][0]["elite_std"]["kp"]
    shares = res["delay_shares"]
    assert shares[1] > 0.8 and min(shares.values()) >= 0.05 / 1.1 and abs(sum(shares.values()) - 1) < 1e-12      # floored at 0.05, renormalised
    assert (calls[-1]["delay"] != 1).any()             # the floor keeps the other delays alive
    assert 0 < res["fell_share"] < 0.2 and res["history"][0]["fell_share"] > res["history"][-1]["fell_share"]
    again = replay.cem(evaluate, axes, 256, 6, seed=0)
    assert again["best"] == res["best"] and replay.cem(evaluate, axes, 256, 6, seed=1)["best"] != res["best"]
    # a box of early enders only: the longest survivor wins, no penalty constant
    res = replay.cem(lambda c: (np.zeros(64), np.zeros(64, bool), (c["kp"] * 100).astype(int)), replay.parse_fit("kp=0.1:0.5"), 64, 3, seed=0)
    assert not res["best"]["lasted"] and res["best"]["plant"]["kp"] > 0.45 and res["fell_share"] == 1.0


def _args(*argv):
    return replay.build_parser().parse_args(list(argv))


def test_command_line_refusals():
    for argv, why in (
            (("--log", "x.pkl", "--fit", "kp=0.5:1.5", "--fit_grid", "kp=0.5:1.5:3"), "exclude each other"),
            (("--log", "x.pkl", "--fit", "stiffness=0.5:1.5"), "unknown axis 'stiffness'"),
            (("--log", "x.pkl", "--fit_grid", "stiffness=0.5:1.5:3"), "unknown axis 'stiffness'"),
            (("--log", "x.pkl", "--fit", "delay=0:3"), "delay=3 is outside the action-history ring"),
            (("--log", "x.pkl", "--fit_grid", "delay=0:3:4"), "delay=3 is outside the action-history ring"),
            (("--log", "x.pkl", "--fit", "delay=0:1.5"), "whole number"),
            (("--log", "x.pkl", "--fit", "kp=0.5:1.5", "--plant", "delay=5"), "outside the action-history ring"),
            (("--log", "x.pkl", "--fit", "kp=0.5:1.5", "--plant", "delay=random"), "sampled delay"),
            (("--log", "x.pkl", "--fit", "kp=1.5:0.5"), "LO is above HI"),
            (("--log", "x.pkl", "--fit", "kp=0.5"), "not kp=LO:HI"),
            (("--log", "x.pkl", "--fit", "kp=0:1"), "finite scale > 0"),
            (("--log", "x.pkl", "--fit", "kp=0.5:1,kp=0.5:1"), "given twice"),
            (("--log", "x.pkl",), "give --fit"),
            (("--fit", "kp=0.5:1.5"), "give a --log"),
            (("--log", "x.pkl", "--fit", "kp=0.5:1.5", "--weight", "speed=1"), "--weight"),
            (("--log", "x.pkl", "--fit", "kp=0.5:1.5", "--num_envs", "8"), "--num_envs >= 16"),
            (("--synthesize", "o.pkl", "--fit", "kp=0.5:1.5"), "does not combine")):
        with pytest.raises(SystemExit) as err:
            replay.check_args(_args(*argv))
        assert why in str(err.value), (argv, str(err.value))
    ok = replay.check_args(_args("--log", "x.pkl", "--fit", "kp=0.5:1.5,delay=0:2", "--plant", "mass=1.1"))
    assert ok["fit"] == [("kp", 0.5, 1.5), ("delay", 0, 2)] and ok["base"] == dict(kp=1.0, mass=1.1, frictionloss=1.0, armature=1.0, delay=0)
    grid = replay.check_args(_args("--log", "x.pkl", "--fit_grid", "kp=0.6:1.0:5,frictionloss=0.5:2:4,delay=0:2:3"))["grid"]
    assert len(grid) == 60 and grid[0]["delay"] == 0 and grid[1]["delay"] == 1 and grid[3]["frictionloss"] == 1.0      # sweeps.parse_axis_grid's order
    with pytest.raises(SystemExit, match="101 floats wide|No such file"):
        replay.run(_args("--log", "/nonexistent/x.pkl", "--fit", "kp=0.5:1.5"))


def test_a_fitted_plant_is_a_plant_string_that_track_accepts():
    p = dict(kp=0.8123456789012345, mass=1.0, frictionloss=1.5, armature=0.7, delay=2)
    s = replay.plant_string(p)
    assert track.parse_plant(s) == p
    assert replay.in_training_ranges(p) == dict(kp=False, mass=True, frictionloss=False, armature=False, delay=True)
    assert replay.in_training_ranges(dict(kp=1.0, mass=1.0, frictionloss=1.0, armature=1.0, delay=0)) == {k: True for k in track.PLANT_AXES}


def test_symbols_and_constants_against_the_header():
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    for sym in ("odk_log_apply", "odk_replay_accumulate"):
        assert sym in engine.EXPORTED_SYMBOLS and re.search(rf"\bint {sym}\(", text)
    assert re.search(r"#define ODK_LOG_ROW\(nu\) \(15 \+ 3 \* \(nu\)\)", text) and engine.log_row(14) == 57
    enums = {k: v for k, v in engine.header_constants().items() if re.fullmatch(r"(?:REPLAY|LOG)_[A-Z_]+", k)}
    assert enums.pop("REPLAY_NSLOT") == engine.REPLAY_NSLOT
    assert len(enums) == 10
    for name, v in enums.items():
        assert getattr(engine, name) == v, name
    assert sorted(n for n in vars(engine) if re.fullmatch(r"(?:REPLAY|LOG)_[A-Z_]+", n) and n != "REPLAY_NSLOT") == sorted(enums)
    src = open(os.path.join(ROOT, "open_duck_playground_amd", "csrc", "odk_reports.hip")).read()
    assert "log_apply_kernel" in src and "replay_kernel" in src


def _golden_tool():
    spec = importlib.util.spec_from_file_location("make_replay_golden", os.path.join(ROOT, "tools", "make_replay_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_committed_oracle_log_is_what_the_oracle_gives(oracle_mod):
    """tests/golden/replay_oracle_log.npz against a fresh run of the float64 oracle on kp x 0.8, frictionloss x 1.5.  The tolerance: the rows
    are float32 copies of float64 results, and the same C source under another compiler may contract or order differently; 1e-5 rad is 150
    float32 ulps at 1 rad and a tenth of the nearest grid neighbour's RMS residual (3e-3 rad)."""
    tool = _golden_tool()
    want = replay.read_log(os.path.join(GOLDEN, "replay_oracle_log.npz"))
    assert want.shape == (61, 101) and os.path.getsize(os.path.join(GOLDEN, "replay_oracle_log.npz")) < 40000
    got = tool.oracle_log(oracle_mod)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    assert np.array_equal(replay.log_table(want, 14)[:, 7:21], replay.excitation(14, 60, 0))      # a_k sits in row k + 1
    assert replay.start_deviation(want, 14) == 0.0 and not want[0, F["last_act"]:F["motor_targets"]].any()
    # and the oracle's own bowl: the plant scores 0 on its log, a neighbour does not
    rows, fell = tool.oracle_replay(oracle_mod, replay.excitation(14, 60, 0), kp=0.85, frictionloss=1.5)
    assert not fell and tool.position_score(got, want) < 1e-10 < 1e-6 < tool.position_score(rows, want)
