"""track.report_rows: the rows and cells of the report from synthetic accumulators -- host arithmetic, no GPU"""
import types

import numpy as np
import pytest

NCMD, NCELL, E = 2, 2, 2
COMMANDS = [[0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0]]
DT = 0.02
# the order of a row's and a cell's keys in the report, as the command-line run writes them with `--gait` and two plants / sensor settings
ROW = ("command", "mean_vx", "mean_vy", "mean_wz", "rms_error_vx", "rms_error_vy", "rms_error_wz", "fall_rate", "mean_episode_reward",
       "mean_episode_steps", "steps", "velocity_samples", "envs")
PLANT_ROW = ROW + ("plants", "gait", "robustness")
SENSOR_ROW = ROW + ("sensors", "gait", "sensor_robustness")
PLANT_CELL, SENSOR_CELL = ROW + ("plant", "gait"), ROW + ("sensor", "gait")


@pytest.fixture(scope="module")
def accs():
    """(tracking [8, 12], gait [8, GAIT_NACC]) float32: every env its own sums, every first episode ended, the first env of every cell fell"""
    from open_duck_playground_amd import track
    rng = np.random.default_rng(11)
    n = NCMD * NCELL * E
    acc = np.zeros((n, track.NACC), np.float32)
    acc[:, track.ENDED] = 1
    acc[:, track.STEPS] = 20 + 3 * np.arange(n)
    acc[:, track.SAMPLES] = acc[:, track.STEPS] - 1
    acc[::E, track.FALLS] = 1
    acc[:, track.REWARD] = rng.uniform(1.0, 9.0, n)
    acc[:, track.SUM:track.SUM + 3] = rng.uniform(-2.0, 2.0, (n, 3))
    acc[:, track.SQERR:track.SQERR + 3] = rng.uniform(0.0, 1.0, (n, 3))
    assert all(len(set(acc[:, k].tolist())) == n for k in (track.STEPS, track.REWARD, track.SUM, track.SQERR))
    gait = rng.uniform(0.0, 1.0, (n, track.GAIT_NACC)).astype(np.float32)
    gait[:, track.G_SAMPLES] = acc[:, track.SAMPLES]
    return acc, gait


def _gait_report(model):
    from open_duck_playground_amd import track
    return track.Report("gait", None, None, {}, reduce=lambda a, cmds, epb: track.reduce_gait(a, cmds, epb, DT, model))


def _axis(kind):
    from open_duck_playground_amd import sensors, track
    plants = [track.parse_plant("kp=0.6"), track.parse_plant("kp=1.0")] if kind == "plants" else []
    settings = [sensors.parse_sensor("imu_delay=0"), sensors.parse_sensor("imu_delay=2")] if kind == "sensors" else []
    return track.cell_axis(types.SimpleNamespace(), [], plants, settings), plants or settings


@pytest.mark.parametrize("kind,label,robustness,row_keys,cell_keys", [("plants", "plant", "robustness", PLANT_ROW, PLANT_CELL),
                                                                      ("sensors", "sensor", "sensor_robustness", SENSOR_ROW, SENSOR_CELL)])
def test_rows_and_cells_of_a_cell_axis(accs, model_a, kind, label, robustness, row_keys, cell_keys):
    from open_duck_playground_amd import sensors, track
    acc, gait = accs
    axis, cells = _axis(kind)
    assert (axis.row_key, axis.label_key, axis.robustness_key, len(axis.cells)) == (kind, label, robustness, NCELL)
    assert axis.threshold == track.DEFAULT_ROBUST_FALL_RATE == axis.settings["robust_fall_rate"] and axis.settings[kind + "_per_command"] == NCELL
    rows = track.report_rows(acc, [(_gait_report(model_a), gait)], COMMANDS, axis, E)
    assert len(rows) == NCMD
    for c, row in enumerate(rows):
        assert tuple(row) == row_keys and len(row[kind]) == NCELL
        # the command row pools its 2E envs
        lo = c * NCELL * E
        pooled = track.reduce_tracking(acc[lo:lo + NCELL * E], [COMMANDS[c]], NCELL * E)[0]
        assert {k: row[k] for k in ROW} == pooled and row["envs"] == NCELL * E and row["command"] == COMMANDS[c]
        assert row["gait"] == track.reduce_gait(gait[lo:lo + NCELL * E], [COMMANDS[c]], NCELL * E, DT, model_a)[0]
        assert row["fall_rate"] == 0.5 and row["steps"] == int(acc[lo:lo + NCELL * E, track.STEPS].sum())
        for p, cell in enumerate(row[kind]):
            at = (NCELL * c + p) * E      # cell (c, p) is envs (2c + p) E .. + E
            assert tuple(cell) == cell_keys
            assert {k: cell[k] for k in ROW} == track.reduce_tracking(acc[at:at + E], [COMMANDS[c]], E)[0]
            assert cell["gait"] == track.reduce_gait(gait[at:at + E], [COMMANDS[c]], E, DT, model_a)[0]
            assert cell[label] == cells[p] and cell[label] is not cells[p]
            assert cell["envs"] == E and cell["fall_rate"] == 0.5 and cell["velocity_samples"] == int(acc[at:at + E, track.SAMPLES].sum())
            assert cell["gait"]["samples"] == cell["velocity_samples"]
        # the robustness object: of the row's finished cells, and the row's last key
        if kind == "plants":
            want = track.reduce_robustness(row[kind], track.DEFAULT_ROBUST_FALL_RATE)
            assert [p["value"] for p in want["kp"]] == [0.6, 1.0]
        else:
            want = track.reduce_robustness(row[kind], track.DEFAULT_ROBUST_FALL_RATE, key="sensor", nominals=sensors.nominal_sensor(), order=sensors.sensor_order)
            assert [p["value"] for p in want["imu_delay"]] == [0, 2]
        assert row[robustness] == want and list(row)[-1] == robustness
        assert [p["mean_episode_reward"] for p in want[list(want)[1]]] == [cell["mean_episode_reward"] for cell in row[kind]]
    # the distinct envs make distinct cells: no cell was placed twice
    figures = [cell["mean_episode_reward"] for row in rows for cell in row[kind]]
    assert len(set(figures)) == NCMD * NCELL
    assert track.block_commands(rows, axis) == [COMMANDS[0], COMMANDS[0], COMMANDS[1], COMMANDS[1]]


def test_rows_without_a_cell_axis(accs, model_a):
    from open_duck_playground_amd import track
    acc, gait = accs
    assert track.cell_axis(types.SimpleNamespace(), [], [], []) is None
    commands = [COMMANDS[c // NCELL] for c in range(NCMD * NCELL)]      # the same 8 envs as 4 commands of E envs
    rows = track.report_rows(acc, [(_gait_report(model_a), gait)], commands, None, E)
    assert len(rows) == NCMD * NCELL and ROW == track.ROW_KEYS
    for c, row in enumerate(rows):
        assert tuple(row) == track.ROW_KEYS + ("gait",)
        assert {k: row[k] for k in ROW} == track.reduce_tracking(acc[c * E:(c + 1) * E], [commands[c]], E)[0]
        assert row["gait"] == track.reduce_gait(gait[c * E:(c + 1) * E], [commands[c]], E, DT, model_a)[0]
    assert track.block_commands(rows, None) == commands
    assert tuple(track.report_rows(acc, [], commands, None, E)[0]) == track.ROW_KEYS
