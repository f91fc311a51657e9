"""GPU checks of the log replay (`python -m open_duck_playground_amd.replay`, include/odk.h "Log replay"): odk_log_apply and
odk_replay_accumulate bit for bit against their float32 numpy restatements (replay.log_apply_np / replay.replay_accumulate_np); a plant
replayed on its own log scores exactly 0 and every other cell of a grid more; the committed float64-oracle log is fitted to its true cell; the
cross-entropy search beats the grid's resolution; the tool end to end.

Shapes: 64 envs are 16 waves of four 16-lane rows, 6 envs leave the last wave partial; biped12 has 12 actuators (lanes 12..15 idle).

MEASURED (first run, profiles/replay/NOTES.md): the oracle log's true cell scores 1.61e-14 against 9.65e-06 for the nearest axis neighbour, a
factor of 6.0e8 (the CPU experiment predicted about 1000); ORACLE_FACTOR is that measurement with a 3x margin (the kernels are deterministic
run to run, the spread is across builds)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

ORACLE_FACTOR = 2.0e8      # measured 6.01e8 on the first run, / 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _fake_log(nu, nrows, env="joystick", seed=3):
    """rows [nrows, nobs] whose actions are the excitation and whose recorded side is small random numbers: every residual is non-zero"""
    from open_duck_playground_amd import replay
    rng = np.random.default_rng(seed)
    f = replay.obs_fields(nu, env)
    rows = np.zeros((nrows, replay.obs_width(nu, env)), np.float32)
    rows[1:, f["last_act"]:f["last_act"] + nu] = replay.excitation(nu, nrows - 1, seed)
    for k, n, s in (("pos", nu, 0.05), ("vel", nu, 0.05), ("gyro", 3, 0.2), ("accel", 3, 1.0)):
        rows[1:, f[k]:f[k] + n] = rng.normal(0.0, s, size=(nrows - 1, n))
    rows[1:, f["contact"]:f["contact"] + 2] = rng.integers(0, 2, size=(nrows - 1, 2))
    rows[:, f["command"]:f["command"] + 7] = rng.uniform(-0.1, 0.1, size=7)
    if "motor_targets" in f:
        rows[0, f["motor_targets"]:f["motor_targets"] + nu] = 0.0
    return rows


def test_log_apply_bits():
    """12 steps of a 10-row table (steps 10 and 11 read the clamped last row), 6 envs (a partial last wave), env 2's track row preset to
    ENDED with STEPS 5 (it keeps reading row 4): action and bound command against the restatement, bit for bit, before every step"""
    import torch
    from open_duck_playground_amd import engine, replay
    n, nu = 6, 14
    env = replay.make_env("flat_terrain", "joystick", n, 12)
    b = env.batch
    table = replay.log_table(_fake_log(nu, 11), nu)
    assert table.shape == (10, engine.log_row(nu))
    dev = b.obs.device
    t_table = torch.from_numpy(table).to(dev)
    cmd = torch.full((n, 7), 9.0, device=dev); action = torch.full((n, nu), 9.0, device=dev)
    track = torch.zeros(n, engine.TRACK_NACC, device=dev)
    track[2, engine.TRACK_ENDED], track[2, engine.TRACK_STEPS] = 1.0, 5.0
    env.set_commands(cmd)
    with pytest.raises(engine.OdkError, match="shape"):
        b.log_apply(t_table[:, :-1].contiguous(), track, action)
    b.log_apply(t_table, track, action)      # what the reset must find
    env.reset(1)
    seen = []
    for k in range(12):
        b.log_apply(t_table, track, action)
        want_a, want_c = replay.log_apply_np(table, track.cpu().numpy())
        np.testing.assert_array_equal(_bits(action.cpu().numpy()), _bits(want_a), err_msg=f"step {k}: action")
        np.testing.assert_array_equal(_bits(cmd.cpu().numpy()), _bits(want_c), err_msg=f"step {k}: command")
        seen.append(want_a[0].copy())
        np.testing.assert_array_equal(want_a[2], table[4, 7:7 + nu])
        b.step(action)
        b.tracking_accumulate(track)
    np.testing.assert_array_equal(seen[11], table[9, 7:7 + nu])      # (env 0 may have ended on the random actions: then it holds its last row)
    env.set_commands(None)
    b.close()


def _accumulate_case(xml, nu, nlog, steps, n=64, flip=5):
    """eager run with the restatement beside it, then the captured run: (gpu eager acc, restated acc, gpu captured acc, track)"""
    from open_duck_playground_amd import replay
    rows = _fake_log(nu, nlog)
    plants = replay.plant_columns([dict(replay.replay_plant(), kp=s) for s in (0.7, 0.9, 1.0, 1.2) for _ in range(n // 4)], n)

    def upside_down(batch):
        qpos, qvel, warm = batch.get_state()
        qpos[flip, 3:7] = (0.0, 1.0, 0.0, 0.0)      # half a turn about x: the up vector points down, the episode ends in step 0
        batch.set_state(qpos, qvel, warm)

    out = {}
    for graph in (False, True):
        r = replay.Replayer(rows, "flat_terrain", "joystick", n, 0, xml, use_graph=graph)
        mt = replay.obs_fields(nu)["motor_targets"]      # the log starts standing: the motors hold the home pose (as replay.record's row 0)
        r.rows[0, mt:mt + nu] = np.asarray(r.batch.model.a["key_ctrl"], np.float32).reshape(-1)[:nu]
        if graph:
            acc, track = r.run(plants, steps=steps, after_start=upside_down)
            assert r.graph is not None
            out["captured"], out["track"] = acc, track
        else:
            b = r.batch
            r.set_plants(plants); r.track.zero_(); r.acc.zero_(); r._first_command()
            r.env.reset(0); r._start(); upside_down(b)
            want = np.zeros((n, 16, 8), np.float32)
            for _ in range(steps):
                b.log_apply(r.table, r.track, r.action)
                b.step(r.action)
                replay.replay_accumulate_np(want, b.priv.cpu().numpy(), b.done.cpu().numpy(), r.track.cpu().numpy(), r.table_np, b.nobs, r.vel_scale)
                b.replay_accumulate(r.acc, r.track, r.table)
                b.tracking_accumulate(r.track)
            out["eager"], out["want"] = r.acc.cpu().numpy(), want
        r.close()
    return out


@pytest.mark.parametrize("xml,nu", [(None, 14), (os.path.join(ROOT, "tests", "assets", "biped12.xml"), 12)], ids=["duck", "biped12"])
def test_replay_accumulate_bits(xml, nu):
    """64 envs with four kp scales, 40 steps of a 45-row log, env 5 upside down (its episode ends in step 0: its row stays zero); every slot of
    every lane against the restatement, and the captured run against the eager one, bit for bit"""
    from open_duck_playground_amd import engine
    o = _accumulate_case(xml, nu, 45, 40)
    np.testing.assert_array_equal(_bits(o["eager"]), _bits(o["want"]))
    np.testing.assert_array_equal(_bits(o["captured"]), _bits(o["eager"]))
    acc, track = o["eager"], o["track"]
    assert not acc[5].any() and track[5, engine.TRACK_ENDED] == 1 and track[5, engine.TRACK_STEPS] == 1
    assert not acc[:, nu:].any()                                         # the lanes past nu
    assert not acc[:, 3:, engine.REPLAY_GYRO_ERR_SQ].any() and not acc[:, 2:, engine.REPLAY_CONTACT_AGREE].any() and not acc[:, 1:, engine.REPLAY_SAMPLES].any()
    ended = track[:, engine.TRACK_ENDED]
    print("first-episode steps:", track[:, engine.TRACK_STEPS].astype(int).tolist())
    assert (ended == 0).any()
    np.testing.assert_array_equal(acc[:, 0, engine.REPLAY_SAMPLES], track[:, engine.TRACK_STEPS] - ended)      # a done step is no sample
    assert (acc[:, :nu, engine.REPLAY_POS_ERR_SQ][ended == 0] > 0).all()
    assert not np.array_equal(acc[0], acc[16]) and not np.array_equal(acc[16], acc[32]) and not np.array_equal(acc[32], acc[48])      # four plants


def test_nothing_is_added_past_the_end_of_the_log():
    """the same 40 steps on a 30-row log (29 table rows): bit for bit the restatement, and 29 samples in every env that lasted"""
    from open_duck_playground_amd import engine
    o = _accumulate_case(None, 14, 30, 40)
    np.testing.assert_array_equal(_bits(o["eager"]), _bits(o["want"]))
    np.testing.assert_array_equal(_bits(o["captured"]), _bits(o["eager"]))
    lasted = (o["track"][:, engine.TRACK_ENDED] == 0) & (o["track"][:, engine.TRACK_STEPS] == 40)
    assert lasted.any() and (o["eager"][lasted, 0, engine.REPLAY_SAMPLES] == 29).all()


GRID = "kp=0.6:1.0:5,frictionloss=0.5:2:4,delay=0:2:3"


@pytest.fixture(scope="module")
def own_log():
    """(rows, grid, index of the true cell): 60 steps of the excitation recorded on the grid's own cell kp 0.8, frictionloss 1.5, delay 1"""
    from open_duck_playground_amd import replay
    grid = replay.parse_fit_grid(GRID, replay.replay_plant())
    true = [i for i, p in enumerate(grid) if abs(p["kp"] - 0.8) < 1e-9 and p["frictionloss"] == 1.5 and p["delay"] == 1]
    assert len(grid) == 60 and len(true) == 1
    rows = replay.record("flat_terrain", plant=grid[true[0]], steps=60)
    assert rows.shape == (61, 101)
    return rows, grid, true[0]


def test_a_plant_replayed_on_its_own_log_scores_zero(own_log):
    """one env per cell of the 60-cell grid: the true cell's score is exactly 0.0, every other cell's is > 0, no cell falls"""
    from open_duck_playground_amd import engine, replay
    rows, grid, true = own_log
    r = replay.Replayer(rows, "flat_terrain", "joystick", len(grid))
    scores, lasted, steps, acc, _ = r.evaluate(replay.plant_columns(grid, r.n))
    r.close()
    print("scores:", " ".join(f"{s:.3e}" for s in scores))
    assert lasted.all() and (steps == 60).all()
    assert scores[true] == 0.0
    others = np.delete(scores, true)
    assert (others > 0).all(), others.min()
    assert (acc[true, :14, engine.REPLAY_POS_ERR_PEAK] == 0).all()      # the peak residual of every joint


def test_the_oracle_log_is_fitted_to_its_true_cell():
    """the committed float64-oracle log (kp 0.8, frictionloss 1.5, delay 0) over kp=0.7:0.9:5 x frictionloss=1:2:3: the argmin is the true
    cell, and its score lies below each of its four axis neighbours' by at least ORACLE_FACTOR"""
    from open_duck_playground_amd import replay
    rows = replay.read_log(os.path.join(GOLDEN, "replay_oracle_log.npz"))
    grid = replay.parse_fit_grid("kp=0.7:0.9:5,frictionloss=1:2:3", replay.replay_plant())
    r = replay.Replayer(rows, "flat_terrain", "joystick", len(grid))
    scores, lasted, _, _, _ = r.evaluate(replay.plant_columns(grid, r.n))
    r.close()
    at = lambda kp, fl: next(i for i, p in enumerate(grid) if abs(p["kp"] - kp) < 1e-9 and p["frictionloss"] == fl)
    true = at(0.8, 1.5)
    near = [at(0.75, 1.5), at(0.85, 1.5), at(0.8, 1.0), at(0.8, 2.0)]
    print("oracle log: true", scores[true], "neighbours", scores[near], "factor", scores[near].min() / scores[true])
    assert lasted.all()
    assert int(np.argmin(scores)) == true
    assert scores[near].min() >= ORACLE_FACTOR * scores[true]


def test_the_search_beats_the_grid(own_log):
    """256 candidates, 4 generations, seed 0, delay fixed at its true value: the best score found lies below the scores of the true plant's
    four axis neighbours at +-0.05 kp and +-0.25 frictionloss, evaluated here on the same log"""
    from open_duck_playground_amd import replay
    rows, grid, true = own_log
    base = dict(replay.replay_plant(), delay=1)
    r = replay.Replayer(rows, "flat_terrain", "joystick", 256)
    res = replay.cem(lambda c: r.evaluate({k: (c[k] if k in c else np.full(r.n, base[k])) for k in replay.PLANT_AXES})[:3],
                     replay.parse_fit("kp=0.5:1.5,frictionloss=0.3:3"), r.n, 4, 0)
    tp = grid[true]
    near = [dict(tp, kp=tp["kp"] - 0.05), dict(tp, kp=tp["kp"] + 0.05), dict(tp, frictionloss=1.25), dict(tp, frictionloss=1.75)]
    ns = r.evaluate(replay.plant_columns(near, r.n))[0][:4]
    r.close()
    print("search: best", res["best"], "neighbours", ns, "history", [h["best_score"] for h in res["history"]])
    assert res["best"]["lasted"] and res["best"]["score"] < ns.min()


def test_replay_end_to_end(tmp_path):
    from open_duck_playground_amd import replay, track
    log, out, best = str(tmp_path / "log.pkl"), str(tmp_path / "fit.json"), str(tmp_path / "best.pkl")
    replay.main(["--synthesize", log, "--plant", "kp=0.8,delay=1", "--excitation", "40"])
    rows = replay.read_log(log)
    assert rows.shape == (41, 101)
    rep = replay.main(["--log", log, "--fit_grid", "kp=0.7:0.9:3,delay=0:2:3", "--output", out, "--save_obs", best])
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep)) and tuple(back) == replay.FIT_KEYS
    plant = track.parse_plant(back["best_plant"])
    assert plant["delay"] == 1 and abs(plant["kp"] - 0.8) < 1e-9 and back["best_score"] == 0.0 and back["fell_share"] == 0.0
    assert len(back["cells"]) == 9 and len(back["joints"]["best"]) == len(back["joints"]["nominal"]) == 14
    assert all(j["pos_rms"] == 0.0 for j in back["joints"]["best"]) and any(j["pos_rms"] > 0 for j in back["joints"]["nominal"])
    assert back["inside_training_ranges"] == dict(kp=False, mass=True, frictionloss=True, armature=True, delay=True)
    np.testing.assert_array_equal(replay.read_log(best), rows)      # the best candidate's simulated rows ARE the log
    rep = replay.main(["--log", log, "--fit", "kp=0.6:1.0,delay=0:2", "--num_envs", "64", "--generations", "2", "--output", out])
    back = json.load(open(out))
    assert tuple(back) == replay.FIT_KEYS and len(back["score_history"]) == 2 and back["cells"] is None
    assert "NOT a confidence interval" in back["identifiability_hint"]["note"] and set(back["identifiability_hint"]["elite_std"]) == {"kp"}
    assert track.parse_plant(back["best_plant"])["delay"] == 1
