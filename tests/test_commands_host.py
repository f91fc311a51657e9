"""CPU checks of caller-given commands and the velocity-tracking tool: the C-ABI exports, the tensor checks of set_commands, the
command-line parsing, the report's reduction of the accumulator and the --save_obs file."""
import ctypes
import json
import pickle

import numpy as np
import pytest


def test_libodk_exports_the_command_binding_and_the_tracking_accumulator():
    from open_duck_playground_amd import engine
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ("odk_batch_bind_commands", "odk_tracking_accumulate"):
        assert hasattr(lib, name), f"libodk.so does not export {name}"
    assert {"odk_batch_bind_commands", "odk_tracking_accumulate"} <= set(engine.EXPORTED_SYMBOLS)


def test_set_commands_rejects_bad_tensors():
    import torch
    from open_duck_playground_amd import engine
    n = 8
    bad = [
        (np.zeros((n, 7), np.float32), "torch tensor"),
        (torch.zeros(n, 6), "shape"),
        (torch.zeros(n + 1, 7), "shape"),
        (torch.zeros(n, 7, dtype=torch.float64), "dtype"),
        (torch.zeros(7, n).t(), "contiguous"),
        (torch.zeros(n, 7), "cuda:0"),        # a host tensor: the kernels read device memory
    ]
    for t, what in bad:
        with pytest.raises(engine.OdkError, match=what):
            engine.check_commands(t, n, 0)


def test_command_rows_and_grid():
    from open_duck_playground_amd import track
    assert track.command_row([0.15, 0, 0]) == [0.15, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert track.command_row([0, 0, 0.5, 0.1, 0.2, 0.3, 0.4]) == [0.0, 0.0, 0.5, 0.1, 0.2, 0.3, 0.4]
    with pytest.raises(ValueError):
        track.command_row([0.1, 0.2])
    rows = track.parse_grid("vx=-0.1:0.1:3,wz=0:1:2")
    exp = [[vx, 0.0, wz, 0.0, 0.0, 0.0, 0.0] for vx in (-0.1, 0.0, 0.1) for wz in (0.0, 1.0)]
    np.testing.assert_allclose(rows, exp, atol=1e-12)
    np.testing.assert_allclose(track.parse_grid("head_yaw=0.5:0.5:1"), [[0, 0, 0, 0, 0, 0.5, 0]])
    for spec in ("vz=0:1:2", "vx=0:1", "vx=0:1:0", "vx=0:1:2,vx=0:1:2", ""):
        with pytest.raises(ValueError):
            track.parse_grid(spec)
    blocks = track.command_blocks(rows[:2], 3)
    assert blocks.shape == (6, 7) and blocks.dtype == np.float32
    np.testing.assert_array_equal(blocks[:3], np.float32([rows[0]] * 3))
    np.testing.assert_array_equal(blocks[3:], np.float32([rows[1]] * 3))


def test_command_line_switches():
    from open_duck_playground_amd import track
    a = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0", "--command", "0.15", "0", "0",
                                         "--grid", "wz=0:0.5:2", "--envs_per_command", "16", "--episode_length", "50", "--seed", "3",
                                         "--env", "standing", "--task", "flat_terrain_backlash", "--cone", "elliptic", "--hfield_up_normals_only"])
    assert a.command == [[0.0, 0.0, 0.0], [0.15, 0.0, 0.0]] and a.grid == "wz=0:0.5:2"
    assert (a.envs_per_command, a.episode_length, a.seed, a.env, a.task, a.cone, a.hfield_up_normals_only) == (16, 50, 3, "standing", "flat_terrain_backlash", "elliptic", True)


def _synthetic_acc(rng, n):
    from open_duck_playground_amd import track
    acc = np.zeros((n, track.NACC), np.float32)
    steps = rng.integers(1, 100, n).astype(np.float32)
    fell = rng.random(n) < 0.3
    acc[:, track.ENDED] = 1.0
    acc[:, track.STEPS] = steps
    acc[:, track.SAMPLES] = steps - 1
    acc[:, track.FALLS] = fell
    acc[:, track.REWARD] = rng.normal(size=n) * 10
    acc[:, track.SUM:track.SUM + 3] = rng.normal(size=(n, 3)) * (steps - 1)[:, None]
    acc[:, track.SQERR:track.SQERR + 3] = rng.random((n, 3)) * (steps - 1)[:, None]
    return acc


def test_report_reduction_and_schema():
    from open_duck_playground_amd import track
    rng = np.random.default_rng(0)
    cmds = [[0, 0, 0, 0, 0, 0, 0], [0.15, 0, 0, 0, 0, 0, 0], [0, 0, 0.5, 0, 0, 0, 0]]
    E = 5
    acc = _synthetic_acc(rng, len(cmds) * E)
    rows = track.reduce_tracking(acc, cmds, E)
    assert len(rows) == 3
    for c, r in enumerate(rows):
        assert tuple(r) == track.ROW_KEYS
        b = acc[c * E:(c + 1) * E].astype(np.float64)
        s = b[:, track.SAMPLES].sum()
        assert r["command"] == cmds[c]
        np.testing.assert_allclose([r["mean_vx"], r["mean_vy"], r["mean_wz"]], b[:, track.SUM:track.SUM + 3].sum(0) / s, rtol=1e-12)
        np.testing.assert_allclose([r["rms_error_vx"], r["rms_error_vy"], r["rms_error_wz"]], np.sqrt(b[:, track.SQERR:track.SQERR + 3].sum(0) / s), rtol=1e-12)
        assert r["fall_rate"] == pytest.approx(b[:, track.FALLS].mean())
        assert r["mean_episode_reward"] == pytest.approx(b[:, track.REWARD].mean())
        assert r["steps"] == int(b[:, track.STEPS].sum()) and r["velocity_samples"] == int(s) and r["envs"] == E
    rep = track.make_report(dict(episode_length=100, envs_per_command=E), rows)
    back = json.loads(json.dumps(rep))
    assert tuple(back) == track.REPORT_KEYS and back["commands"] == rows
    # an env that never produced a velocity sample (fell on its first step) does not divide by zero
    z = np.zeros((1, track.NACC), np.float32); z[0, track.STEPS] = 1; z[0, track.FALLS] = 1; z[0, track.ENDED] = 1
    r0 = track.reduce_tracking(z, [cmds[0]], 1)[0]
    assert r0["fall_rate"] == 1.0 and r0["velocity_samples"] == 0 and np.isfinite(r0["mean_vx"])


def test_save_obs_round_trips_as_a_list_of_arrays(tmp_path):
    from open_duck_playground_amd import track
    obs = np.random.default_rng(1).normal(size=(4, 101)).astype(np.float32)
    p = tmp_path / "saved_obs.pkl"
    track.save_obs(str(p), obs)
    back = pickle.load(open(p, "rb"))
    assert isinstance(back, list) and len(back) == 4
    for o, b in zip(obs, back):
        assert isinstance(b, np.ndarray) and b.shape == (101,)
        np.testing.assert_array_equal(o, b)
