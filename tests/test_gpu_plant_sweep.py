"""GPU checks of the plant sweep of `python -m open_duck_playground_amd.track` (`--plant`, `--plant_grid`): without the new flags the report
is the plain Tracker's; a cell is the plant it names (bit for bit a test-built Tracker whose env got nominal times scale through set_param
and the same bound delays), and the all-ones plant with the sampled delay is the run without a plant; the report end to end."""
import json

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

E, T = 16, 40


def _argv(ckpt, *extra):
    return ["--checkpoint", ckpt, "--command", "0", "0", "0", "--command", "0.15", "0", "0", "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "1", *extra]


def _plain_run(track, args, commands, cells_per_command, prepare=None):
    """a test-built Tracker over `commands` with cells_per_command * E envs each, as `run` lays them out; `prepare(env)` sets the plant.
    Returns the tracking accumulator [n, 12]."""
    import torch
    n = len(commands) * cells_per_command * E
    env = track.make_env(args, n, 0)
    net = track.load_networks(args.checkpoint, env, torch.device("cuda", 0))
    env.set_commands(torch.from_numpy(track.command_blocks(commands, cells_per_command * E)).to("cuda"))
    delays = prepare(env) if prepare else None
    tr = track.Tracker(env, net, delays=delays)
    with torch.no_grad():
        tr.reset(args.seed)
        for _ in range(T):
            tr.step()
        acc = tr.acc.cpu().numpy()
    assert tr.graph is not None
    env.set_commands(None)
    env.set_action_delays(None)
    env.batch.close()
    return acc


def test_track_without_plant_flags_is_the_report_of_before(tmp_path, monkeypatch):
    """no --plant*, --randomize or --noise_level: no parameter is set, no delay bound, and the report is the one `reduce_tracking` gives
    for a plain Tracker run of the same layout and seed -- keys, settings and every figure"""
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    calls = []
    for name in ("bind_action_delays", "set_param"):
        real = getattr(engine.Batch, name)
        monkeypatch.setattr(engine.Batch, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    out = tmp_path / "report.json"
    args = track.build_parser().parse_args(_argv(ckpt, "--output", str(out)))
    rep = track.run(args)
    assert calls == []
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep))
    assert tuple(back) == track.REPORT_KEYS and back["settings"]["graph"]
    assert not any(k.startswith(("plant", "robust", "randomize", "noise")) for k in back["settings"])
    for r in back["commands"]:
        assert tuple(r) == track.ROW_KEYS and r["envs"] == E
    commands = [track.command_row([0, 0, 0]), track.command_row([0.15, 0, 0])]
    acc = _plain_run(track, args, commands, 1)
    assert calls == ["bind_action_delays"]                 # (_plain_run's own unbinding)
    assert back["commands"] == json.loads(json.dumps(track.reduce_tracking(acc, commands, E)))


def test_a_cell_is_the_plant_it_names(tmp_path):
    """`--plant kp=0.6,delay=2 --plant kp=1.0` over two commands.  Every cell's row of the report is `reduce_tracking` of a test-built
    Tracker's accumulator, whose env the test itself gave nominal times scale (set_param, all six parameters) and the same bound delays:
    the accumulators are compared bit for bit through their reduction -- and directly, by a second `run` whose Tracker is kept.  The
    all-ones cell with delay=random equals the corresponding block of a run with no plant at all, bit for bit."""
    import torch
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    args = track.build_parser().parse_args(_argv(ckpt, "--plant", "kp=0.6,delay=2", "--plant", "kp=1.0", "--output", str(tmp_path / "r.json")))
    kept = []
    real_tracker = track.Tracker
    track.Tracker = lambda *a, **k: (kept.append(real_tracker(*a, **k)), kept[-1])[1]
    try:
        rep = track.run(args)
    finally:
        track.Tracker = real_tracker
    got = kept[0].acc.cpu().numpy()
    assert kept[0].delays is not None and kept[0].delays.dtype == torch.int32
    np.testing.assert_array_equal(kept[0].delays.cpu().numpy(), np.tile(np.repeat(np.array([2, -1], np.int32), E), 2))
    commands = [track.command_row([0, 0, 0]), track.command_row([0.15, 0, 0])]
    n = 2 * 2 * E
    kp_scale = np.tile(np.repeat(np.array([0.6, 1.0]), E), 2)

    def prepare(env):
        a = env.mj_model.a
        nu = env.mj_model.nu
        trn = np.asarray(a["actuator_trnid"]).reshape(nu, -1)[:, 0]
        dofs, qadr = np.asarray(a["jnt_dofadr"])[trn], np.asarray(a["jnt_qposadr"])[trn]
        rep_n = lambda v: np.repeat(np.asarray(v, np.float64).reshape(1, -1), n, axis=0)
        b = env.batch
        b.set_param(engine.PARAM_BODY_MASS, rep_n(a["body_mass"]))
        b.set_param(engine.PARAM_BODY_IPOS_TORSO, rep_n(np.asarray(a["body_ipos"])[1]))
        b.set_param(engine.PARAM_DOF_FRICTIONLOSS, rep_n(np.asarray(a["dof_frictionloss"])[dofs]))
        b.set_param(engine.PARAM_DOF_ARMATURE, rep_n(np.asarray(a["dof_armature"])[dofs]))
        b.set_param(engine.PARAM_QPOS0, rep_n(np.asarray(a["qpos0"])[qadr]))
        b.set_param(engine.PARAM_KP, rep_n(a["actuator_gainprm0"]) * kp_scale[:, None])
        return torch.tensor(np.tile(np.repeat(np.array([2, -1], np.int32), E), 2), device="cuda")
    want = _plain_run(track, args, commands, 2, prepare)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg="run's accumulator against the test-built Tracker's")
    cells = [cell for row in rep["commands"] for cell in row["plants"]]
    assert len(cells) == 4
    cell_rows = track.reduce_tracking(want, [c for c in commands for _ in range(2)], E)
    for i, (cell, w) in enumerate(zip(cells, cell_rows)):
        assert {k: cell[k] for k in track.ROW_KEYS} == w, i
        assert cell["plant"] == dict(kp=[0.6, 1.0][i % 2], mass=1.0, frictionloss=1.0, armature=1.0, delay=[2, "random"][i % 2])
    # the plants are not the same robot: the weak, late plant differs from the nominal one
    for c in range(2):
        assert not np.array_equal(got[(2 * c) * E:(2 * c + 1) * E], got[(2 * c + 1) * E:(2 * c + 2) * E])
    # no plant at all, same layout and seed: the all-ones cells are its blocks
    none = _plain_run(track, args, commands, 2)
    for c in range(2):
        blk = slice((2 * c + 1) * E, (2 * c + 2) * E)
        np.testing.assert_array_equal(got[blk].view(np.int32), none[blk].view(np.int32), err_msg=f"command {c}: the all-ones plant is the nominal robot")


def test_track_plant_sweep_end_to_end(tmp_path):
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    out = tmp_path / "report.json"
    args = track.build_parser().parse_args(_argv(ckpt, "--plant_grid", "kp=0.5:1.0:2,delay=0:2:3", "--gait", "--falls", "--output", str(out)))
    rep = track.run(args)
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep))
    s = back["settings"]
    assert s["graph"] and s["num_envs"] == 2 * 6 * E and s["envs_per_command"] == E and s["plants_per_command"] == 6
    assert s["plant_grid"] == "kp=0.5:1.0:2,delay=0:2:3" and s["plant"] is None and s["robust_fall_rate"] == 0.05
    assert "inertias NOT rescaled" in s["plant_semantics"] and "nominal mass" in s["plant_semantics"]
    assert tuple(back) == track.REPORT_KEYS and len(back["commands"]) == 2
    for r in back["commands"]:
        assert tuple(r)[:len(track.ROW_KEYS)] == track.ROW_KEYS and set(track.PLANT_ROW_KEYS) <= set(r)
        assert r["envs"] == 6 * E == sum(c["envs"] for c in r["plants"])           # the existing keys pool the command's cells
        assert len(r["plants"]) == 6
        assert [(c["plant"]["kp"], c["plant"]["delay"]) for c in r["plants"]] == [(0.5, 0), (0.5, 1), (0.5, 2), (1.0, 0), (1.0, 1), (1.0, 2)]
        assert "gait" in r and "falls" in r
        for c in r["plants"]:
            assert tuple(c)[:len(track.ROW_KEYS)] == track.ROW_KEYS and c["command"] == r["command"] and c["envs"] == E
            assert tuple(c["plant"]) == track.PLANT_AXES and c["plant"]["mass"] == c["plant"]["frictionloss"] == c["plant"]["armature"] == 1.0
            assert tuple(c["gait"]) == track.GAIT_KEYS and isinstance(c["falls"], dict) and c["falls"]
            assert 0.0 <= c["fall_rate"] <= 1.0 and 0 < c["mean_episode_steps"] <= T
        rb = r["robustness"]
        assert set(rb) == {"robust_fall_rate", "kp", "delay", "survived_range"} and set(rb["survived_range"]) == {"kp", "delay"}
        assert [p["value"] for p in rb["kp"]] == [0.5, 1.0] and [p["value"] for p in rb["delay"]] == [0, 1, 2]
        assert all(tuple(p) == track.ROBUSTNESS_POINT_KEYS for p in rb["kp"] + rb["delay"])
        by = {(c["plant"]["kp"], c["plant"]["delay"]): c for c in r["plants"]}
        for p in rb["kp"]:                                 # the kp line runs at the smallest delay, the delay line at kp 1
            assert all(p[k] == by[(p["value"], 0)][k] for k in track.ROBUSTNESS_POINT_KEYS[1:])
        for p in rb["delay"]:
            assert all(p[k] == by[(1.0, p["value"])][k] for k in track.ROBUSTNESS_POINT_KEYS[1:])
        # cells that differ only in the delay are not the same run
        for kp in (0.5, 1.0):
            figures = [{k: v for k, v in by[(kp, d)].items() if k != "plant"} for d in (0, 1, 2)]
            assert figures[0] != figures[1] and figures[1] != figures[2] and figures[0] != figures[2]
    print(json.dumps(back["commands"][1]["robustness"], indent=1))
