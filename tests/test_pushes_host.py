"""CPU checks of caller-given pushes and the push-recovery report: the C-ABI exports, the tensor checks of set_pushes, the push grid and
the cell layout of `track`, the report's reduction of the push accumulator, and -- on the oracle alone -- the emulation the GPU parity
test of bound pushes leans on (a kick added to qvel[0:2] before `step` is the oracle's own push)."""
import ctypes

import numpy as np
import pytest


def test_libodk_exports_the_push_binding_and_the_push_accumulator():
    from open_duck_playground_amd import engine
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ("odk_batch_bind_pushes", "odk_push_accumulate"):
        assert hasattr(lib, name), f"libodk.so does not export {name}"
    assert {"odk_batch_bind_pushes", "odk_push_accumulate"} <= set(engine.EXPORTED_SYMBOLS)
    assert engine.PUSH_NACC == 10
    assert (engine.PUSH_PUSHED, engine.PUSH_PUSH_AT, engine.PUSH_FELL, engine.PUSH_STEPS_TO_FALL, engine.PUSH_LAST_OFF, engine.PUSH_PEAK_LIN_ERR,
            engine.PUSH_PEAK_ANG_ERR, engine.PUSH_PRE_LIN_ERR_SUM, engine.PUSH_PRE_SAMPLES, engine.PUSH_PRE_LIN_ERR_LOW) == tuple(range(10))


def test_the_header_names_the_accumulator_columns_as_the_python_side_does():
    from open_duck_playground_amd import engine, track
    header = engine.header_constants()
    assert header["PUSH_NACC"] == 10
    for name in ("PUSHED", "PUSH_AT", "FELL", "STEPS_TO_FALL", "LAST_OFF", "PEAK_LIN_ERR", "PEAK_ANG_ERR", "PRE_LIN_ERR_SUM", "PRE_SAMPLES", "PRE_LIN_ERR_LOW"):
        assert header["PUSH_" + name] == getattr(engine, "PUSH_" + name), name
    assert track.PUSH_NACC == engine.PUSH_NACC
    assert (track.P_PUSHED, track.P_PUSH_AT, track.P_FELL, track.P_STEPS_TO_FALL, track.P_LAST_OFF, track.P_PEAK_LIN, track.P_PEAK_ANG, track.P_PRE_SUM,
            track.P_PRE_SAMPLES, track.P_PRE_LOW) == tuple(range(10))


def test_set_pushes_rejects_bad_tensors():
    import torch
    from open_duck_playground_amd import engine
    n = 8
    bad = [
        (np.zeros((n, 2), np.float32), "torch tensor"),
        (torch.zeros(n, 1), "shape"),
        (torch.zeros(n + 1, 2), "shape"),
        (torch.zeros(n * 2), "shape"),
        (torch.zeros(n, 2, dtype=torch.float64), "dtype"),
        (torch.zeros(2, n).t(), "contiguous"),
        (torch.zeros(n, 2), "cuda:0"),        # a host tensor: the kernels read device memory
        (torch.zeros(n, 4), "cuda:0"),        # wider rows are a legal shape (row_stride 4); this one is refused for where it lives
    ]
    for t, what in bad:
        with pytest.raises(engine.OdkError, match=what):
            engine.check_pushes(t, n, 0)
    for t, cols, what in ((np.zeros((n, 9), np.float32), 9, "torch tensor"), (torch.zeros(n, 12), 9, "shape"), (torch.zeros(n, 9, dtype=torch.float64), 9, "dtype"),
                          (torch.zeros(9, n).t(), 9, "contiguous"), (torch.zeros(n, 9), 9, "cuda:0")):
        with pytest.raises(engine.OdkError, match=what):
            engine.check_accumulator("acc", t, n, cols, 0)


def test_push_rows_grid_and_cell_layout():
    from open_duck_playground_amd import track
    p = track.push_row([0.0, 0.5])
    assert p["push"] == [0.0, 0.5] and p["magnitude"] == pytest.approx(0.5) and p["direction_deg"] == pytest.approx(90.0)
    assert track.push_row([-1.0, 0.0])["direction_deg"] == pytest.approx(180.0)
    assert track.push_row([0.0, -1.0])["direction_deg"] == pytest.approx(270.0)
    assert track.push_row([0.0, 0.0]) == dict(push=[0.0, 0.0], magnitude=0.0, direction_deg=0.0)
    with pytest.raises(ValueError):
        track.push_row([1.0])
    grid = track.parse_push_grid("magnitude=0:3:3,direction=0:180:2")
    assert [(g["magnitude"], g["direction_deg"]) for g in grid] == [(0.0, 0.0), (0.0, 180.0), (1.5, 0.0), (1.5, 180.0), (3.0, 0.0), (3.0, 180.0)]
    np.testing.assert_allclose([g["push"] for g in grid], [[0, 0], [0, 0], [1.5, 0], [-1.5, 0], [3, 0], [-3, 0]], atol=1e-12)
    # the axes as written: direction first makes the magnitude vary fastest; a grid without a direction pushes along +x
    swapped = track.parse_push_grid("direction=0:90:2,magnitude=1:2:2")
    assert [(g["magnitude"], g["direction_deg"]) for g in swapped] == [(1.0, 0.0), (2.0, 0.0), (1.0, 90.0), (2.0, 90.0)]
    np.testing.assert_allclose(swapped[3]["push"], [0.0, 2.0], atol=1e-12)
    assert [g["push"] for g in track.parse_push_grid("magnitude=0.5:0.5:1")] == [[0.5, 0.0]]
    for spec in ("direction=0:90:2", "speed=0:1:2", "magnitude=0:1", "magnitude=0:1:0", "magnitude=0:1:2,magnitude=0:1:2", "magnitude=-1:1:3", ""):
        with pytest.raises(ValueError):
            track.parse_push_grid(spec)
    # cells: command blocks outermost, then pushes, then the cell's envs
    cmds = [[0.0] * 7, [0.15, 0, 0, 0, 0, 0, 0]]
    pushes = swapped[:3]
    cmd, kicks = track.cell_blocks(cmds, pushes, 2)
    assert cmd.shape == (12, 7) and kicks.shape == (12, 2) and cmd.dtype == np.float32 and kicks.dtype == np.float32
    np.testing.assert_array_equal(cmd[:6], np.float32([cmds[0]] * 6))
    np.testing.assert_array_equal(cmd[6:], np.float32([cmds[1]] * 6))
    want = np.float32([p["push"] for p in pushes for _ in range(2)])
    np.testing.assert_array_equal(kicks[:6], want)
    np.testing.assert_array_equal(kicks[6:], want)


def test_push_command_line_switches():
    from open_duck_playground_amd import track
    a = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0"])
    assert a.push is None and a.push_grid is None and a.push_at == 200 and a.push_tolerance == [0.05, 0.2]
    assert (track.DEFAULT_PUSH_AT, track.DEFAULT_PUSH_TOLERANCE) == (200, (0.05, 0.2))
    a = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0", "--push", "0.5", "0", "--push", "0", "-0.5",
                                         "--push_grid", "magnitude=0:1:3,direction=0:270:4", "--push_at", "50", "--push_tolerance", "0.1", "0.3"])
    assert a.push == [[0.5, 0.0], [0.0, -0.5]] and a.push_grid == "magnitude=0:1:3,direction=0:270:4" and a.push_at == 50
    assert a.push_tolerance == [0.1, 0.3]


def _acc_rows(rows):
    """rows of (pushed, push_at, fell, steps_to_fall, last_off, peak_lin, peak_ang, pre_sum, pre_samples); the sum's low part stays 0"""
    r = np.asarray(rows, np.float32).reshape(-1, 9)
    return np.concatenate([r, np.zeros((len(r), 1), np.float32)], axis=1)


def test_push_report_reduction():
    from open_duck_playground_amd import track
    dt = 0.02
    cmds = [[0.0] * 7]
    pushes = [track.push_entry(m, 0.0) for m in (0.0, 1.0, 2.0)]
    E = 5
    acc = _acc_rows(
        # cell 0: a zero kick -- nobody is pushed; two envs fell on their own (FELL is only set at or after a push)
        [(0, 0, 0, 0, 0, 0, 0, 2.0, 100)] * 3 + [(0, 0, 0, 0, 0, 0, 0, 0.5, 30)] * 2 +
        # cell 1: four pushed at step 20 (one fell 7 steps on, three survive with recovery 0 / 10 / 40), one ended before the push
        [(1, 20, 1, 7, 6, 0.9, 2.0, 0.4, 20), (1, 20, 0, 0, 0, 0.04, 0.1, 0.2, 20), (1, 20, 0, 0, 10, 0.3, 0.5, 0.2, 20),
         (1, 20, 0, 0, 40, 0.5, 0.7, 0.6, 20), (0, 0, 0, 0, 0, 0, 0, 0.1, 10)] +
        # cell 2: everybody falls
        [(1, 20, 1, k, k - 1, 1.0 + k, 3.0, 0.2, 20) for k in (2, 3, 4, 5, 6)])
    out = track.reduce_pushes(acc, cmds, pushes, E, dt)
    assert len(out) == 1 and tuple(out[0]) == track.PUSH_ROW_KEYS
    c0, c1, c2 = out[0]["pushes"]
    for c, p in zip((c0, c1, c2), pushes):
        assert tuple(c) == track.PUSH_CELL_KEYS
        assert c["push"] == p["push"] and c["magnitude"] == p["magnitude"] and c["direction_deg"] == 0.0 and c["envs"] == E
    # nobody pushed: no falls after a push, nothing to recover from, but the policy's own tracking error is there
    assert c0["pushed_envs"] == 0 and c0["fall_rate_after_push"] == 0.0
    for k in ("mean_steps_to_fall", "recovery_steps_median", "recovery_steps_p90", "recovery_time_s", "peak_lin_err_mean", "peak_ang_err_mean"):
        assert c0[k] is None, k
    assert c0["pre_push_lin_err_mean"] == pytest.approx((3 * 2.0 + 2 * 0.5) / (3 * 100 + 2 * 30))
    # medians and the 90th percentile over the survivors only (0, 10, 40): the env that fell had LAST_OFF 6, the unpushed one 0
    assert c1["pushed_envs"] == 4 and c1["fall_rate_after_push"] == pytest.approx(0.25) and c1["mean_steps_to_fall"] == pytest.approx(7.0)
    assert c1["recovery_steps_median"] == pytest.approx(10.0) and c1["recovery_steps_p90"] == pytest.approx(np.percentile([0, 10, 40], 90))
    assert c1["recovery_time_s"] == pytest.approx(10.0 * dt)
    assert c1["peak_lin_err_mean"] == pytest.approx(np.float32([0.9, 0.04, 0.3, 0.5]).astype(np.float64).mean())
    assert c1["peak_ang_err_mean"] == pytest.approx(np.float32([2.0, 0.1, 0.5, 0.7]).astype(np.float64).mean())
    assert c1["pre_push_lin_err_mean"] == pytest.approx(np.float32([0.4, 0.2, 0.2, 0.6, 0.1]).astype(np.float64).sum() / 90)
    # everybody falls: no survivors to take a recovery time from
    assert c2["pushed_envs"] == 5 and c2["fall_rate_after_push"] == 1.0 and c2["mean_steps_to_fall"] == pytest.approx(4.0)
    assert c2["recovery_steps_median"] is None and c2["recovery_steps_p90"] is None and c2["recovery_time_s"] is None
    assert c2["peak_lin_err_mean"] == pytest.approx(5.0)
    assert out[0]["max_push_survived"] == [dict(direction_deg=0.0, magnitude=0.0)]
    import json
    assert json.loads(json.dumps(out)) == out


def test_max_push_survived_per_direction_with_a_gap():
    """per direction the LARGEST magnitude of the grid whose cell has no fall after the push: falls at a smaller magnitude (a gap in the
    middle) do not cap it; a direction in which every magnitude has falls reports None"""
    from open_duck_playground_amd import track
    pushes = track.parse_push_grid("magnitude=0.5:2:4,direction=0:180:3")      # 0.5 1.0 1.5 2.0 x 0 90 180
    E = 2
    ok = (1, 5, 0, 0, 3, 0.2, 0.2, 0.1, 5)
    down = (1, 5, 1, 4, 3, 0.9, 0.9, 0.1, 5)
    falls = {(0.5, 0.0): 0, (1.0, 0.0): 1, (1.5, 0.0): 0, (2.0, 0.0): 2,        # direction 0: a gap at 1.0, survived up to 1.5
             (0.5, 90.0): 1, (1.0, 90.0): 1, (1.5, 90.0): 2, (2.0, 90.0): 2,     # direction 90: falls everywhere
             (0.5, 180.0): 0, (1.0, 180.0): 0, (1.5, 180.0): 0, (2.0, 180.0): 0}  # direction 180: the whole grid survived
    cmds = [[0.0] * 7, [0.1, 0, 0, 0, 0, 0, 0]]
    rows = []
    for c in range(2):
        for p in pushes:
            k = falls[(p["magnitude"], p["direction_deg"])] if c == 0 else 0
            rows += [down] * k + [ok] * (E - k)
    out = track.reduce_pushes(_acc_rows(rows), cmds, pushes, E, 0.02)
    assert out[0]["max_push_survived"] == [dict(direction_deg=0.0, magnitude=1.5), dict(direction_deg=90.0, magnitude=None),
                                           dict(direction_deg=180.0, magnitude=2.0)]
    assert out[1]["max_push_survived"] == [dict(direction_deg=d, magnitude=2.0) for d in (0.0, 90.0, 180.0)]
    rates = {(p["magnitude"], p["direction_deg"]): p["fall_rate_after_push"] for p in out[0]["pushes"]}
    assert rates == {k: v / E for k, v in falls.items()}
    # a kick that reached nobody (every env of the cell ended its first episode before the pushed step) was not survived by anybody:
    # direction 180's largest magnitude with nobody pushed falls back to 1.5; the zero kick, which pushes nobody by definition, counts
    nobody = (0, 0, 0, 0, 0, 0, 0, 0.1, 5)
    rows2 = []
    for p in pushes:
        lost = (p["magnitude"], p["direction_deg"]) == (2.0, 180.0)
        rows2 += [nobody if lost else ok] * E
    out2 = track.reduce_pushes(_acc_rows(rows2), cmds[:1], pushes, E, 0.02)
    assert out2[0]["max_push_survived"] == [dict(direction_deg=0.0, magnitude=2.0), dict(direction_deg=90.0, magnitude=2.0),
                                            dict(direction_deg=180.0, magnitude=1.5)]
    cell = [c for c in out2[0]["pushes"] if (c["magnitude"], c["direction_deg"]) == (2.0, 180.0)][0]
    assert cell["pushed_envs"] == 0 and cell["fall_rate_after_push"] == 0.0
    zero = track.reduce_pushes(_acc_rows([nobody] * E), cmds[:1], [track.push_entry(0.0, 0.0)], E, 0.02)
    assert zero[0]["max_push_survived"] == [dict(direction_deg=0.0, magnitude=0.0)]


def test_a_kick_added_before_the_oracle_step_is_the_oracles_own_push(oracle_mod, model_a, prm_arrays):
    """The method of the GPU parity test of bound pushes, pinned on the oracle alone: at an env step where the oracle's gate fires
    ((push_step + 1) % push_interval_steps == 0), a clone with push_enable = 0 whose qvel[0:2] got `push * mag` before `step` computes
    every output bit for bit as the pushed env does, except the `push` field (odko_env_step reads qvel nowhere before the push)."""
    O = oracle_mod
    om = O.OracleModel(model_a.blob())
    prm = O.OraclePRM(prm_arrays)
    e = O.OracleEnv(om, prm)
    e.reset(11, 3)
    assert e.cfg["push_enable"][0] != 0
    interval = int(e.ints("push_interval_steps")[0])
    e.ints("push_step")[0] = interval - 3          # the gate fires on the third step from here
    rng = np.random.default_rng(5)
    nu = model_a.nu
    fired = 0
    fields = ("command", "last_act", "last_last_act", "last_last_last_act", "motor_targets", "feet_air_time", "swing_peak", "action_history",
              "imu_history", "current_reference_motion", "imitation_phase", "ep_metrics", "obs", "priv", "metrics", "contact", "reward", "done",
              "ep_steps", "truncation", "episode_done", "ep_sum_reward", "ep_length")
    ints = ("last_contact", "key", "step", "push_step", "push_interval_steps", "imitation_i", "rng_ctr")
    for t in range(5):
        act = rng.uniform(-1, 1, nu)
        gate = (int(e.ints("push_step")[0]) + 1) % int(e.ints("push_interval_steps")[0]) == 0
        probe = e.clone()
        e.step(act)
        if not gate:
            assert np.all(np.array(e["push"][:2]) == 0)
            continue
        fired += 1
        push = np.array(e["push"][:2])             # the unit direction the oracle drew (gate = 1: cos, sin of theta)
        assert np.hypot(*push) == pytest.approx(1.0)
        lo, hi = (float(x) for x in e.cfg["push_magnitude_range"][:2])
        mag = _oracle_magnitude(O, probe, lo, hi)
        assert lo <= mag <= hi
        kick = push * mag                          # the test's own `push * mag`
        emu = probe.clone()
        emu.cfg["push_enable"][0] = 0.0
        emu.data["qvel"][0] += kick[0]; emu.data["qvel"][1] += kick[1]
        emu.step(act)
        assert np.all(np.array(emu["push"][:2]) == 0)
        for nm in fields:
            np.testing.assert_array_equal(np.array(emu[nm]), np.array(e[nm]), err_msg=nm)
        for nm in ints:
            np.testing.assert_array_equal(np.array(emu.ints(nm)), np.array(e.ints(nm)), err_msg=nm)
        for nm in ("qpos", "qvel", "qacc_warmstart"):
            np.testing.assert_array_equal(np.array(emu.data[nm]), np.array(e.data[nm]), err_msg=nm)
    assert fired == 1


def _oracle_magnitude(O, env, lo, hi):
    """The push magnitude of the step `env` is about to take, restated from its stream with the oracle's own generator:
    mag = lo + U(draw 3) (hi - lo) (oracle/odk_oracle_env.c:451, joystick.py:381-398)."""
    key = env.ints("key")
    u3 = float(O.lib().lib.odko_rng_uniform(int(key[0]), int(key[1]), int(env.ints("rng_ctr")[0]), 3))
    return lo + u3 * (hi - lo)


def _parity_cases():
    import test_gpu_pushes as G
    return G.PARITY_CASES


@pytest.mark.parametrize("task,standing,dr,seed", _parity_cases())
def test_the_parity_cases_of_bound_pushes_stay_inside_the_set_aside_cap(oracle_mod, task, standing, dr, seed):
    """The share of env steps that the oracle's own sensitivity sets aside in a case of tests/test_gpu_pushes.py
    `test_bound_pushes_match_the_oracle_env` is decided by the oracle alone: computed here, without a GPU, for the case's seed, and held
    to the project's cap.  Passes on any commit that has the cases; it keeps the seeds' claim re-derivable."""
    import test_gpu_pushes as G
    from test_gpu_env import SET_ASIDE
    share = G.oracle_ill_fraction(oracle_mod, task, standing, dr, seed)
    print(f"{task} standing={standing} dr={dr} seed={seed}: set-aside share {share:.4f} (cap {SET_ASIDE['ill_fraction']})")
    assert share <= SET_ASIDE["ill_fraction"]
