"""CPU checks of the path report and the waypoint follower of `track --path` / `track --waypoints`: the C-ABI exports and the slot names,
the course parser with every refusal by its message, the course table's layout and the clamped map, the reductions of hand-built path
accumulators (None cases, medians, falls by leg), the closed-form ideal arc against a float64 Euler integration, the key sets of a plain
run, and the tensor and parameter checks of the three `Batch` methods."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("odk_path_begin", "odk_path_accumulate", "odk_waypoint_command_apply")
SLOTS = dict(START_X=0, START_Y=1, START_HX=2, START_HY=3, X=4, Y=5, HX=6, HY=7, LENGTH=8, TURN=9, SAMPLES=10, FELL=11, FELL_LEG=12, WP_INDEX=13,
             XTRACK_SAMPLES=14, XTRACK_SQ=15, XTRACK_PEAK=16, GOAL_DIST=17, REACHED=18)
NACC, MAX_WP, COURSE_FLOATS = 32, 8, 17


def test_libodk_exports_the_three_launches_and_the_header_names_their_slots():
    from open_duck_playground_amd import engine, track
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    if not os.path.exists(engine.POISON_LIB_PATH):
        engine.build_library(poison=True)
    poison = ctypes.CDLL(engine.POISON_LIB_PATH)
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert hasattr(poison, name), name
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\bint {name}\(const odk_batch\* b,", text), name
    names = {k[5:]: v for k, v in engine.header_constants().items() if k.startswith("PATH_")}
    assert names.pop("NACC") == NACC and engine.PATH_NACC == NACC
    assert names.pop("MAX_WAYPOINTS") == MAX_WP and engine.PATH_MAX_WAYPOINTS == MAX_WP
    assert "#define ODK_PATH_COURSE_FLOATS (1 + 2 * ODK_PATH_MAX_WAYPOINTS)" in text
    assert names.pop("COURSE_FLOATS") == COURSE_FLOATS and engine.PATH_COURSE_FLOATS == COURSE_FLOATS
    assert names == SLOTS                                        # the header names these slots and no others
    for name, slot in names.items():
        assert getattr(engine, "PATH_" + name) == slot, name
    used = sorted(s + i for name, s in SLOTS.items() for i in range(MAX_WP if name == "REACHED" else 1))
    assert used == list(range(SLOTS["REACHED"] + MAX_WP)) and used[-1] < NACC      # no two slots overlap, and the row holds them
    assert track.PATH_MAX_WAYPOINTS == MAX_WP


def test_parse_waypoints_and_the_course_table():
    from open_duck_playground_amd import track
    pts = track.parse_waypoints("0.5,0 | 0.5,0.5 | 0,0.5 | 0,0")
    assert pts == [[0.5, 0.0], [0.5, 0.5], [0.0, 0.5], [0.0, 0.0]]
    assert track.parse_waypoints(" -1e-1 , 2 ") == [[-0.1, 2.0]]
    eight = [[0.1 * k, -0.1 * k] for k in range(8)]
    tab = track.course_table([pts, [[0.25, -0.5]], eight])
    assert tab.dtype == np.float32 and tab.shape == (3, COURSE_FLOATS)
    np.testing.assert_array_equal(tab[0], np.float32([4, 0.5, 0, 0.5, 0.5, 0, 0.5, 0, 0] + [0] * 8))
    np.testing.assert_array_equal(tab[1], np.float32([1, 0.25, -0.5] + [0] * 14))
    np.testing.assert_array_equal(tab[2], np.float32([8] + [x for p in eight for x in p]))
    with pytest.raises(ValueError, match="no course given"):
        track.course_table([])
    with pytest.raises(ValueError, match="1 to 8 points, this one has 9"):
        track.course_table([eight + [[1.0, 1.0]]])
    with pytest.raises(ValueError, match="1 to 8 points, this one has 0"):      # a count outside the range never reaches the device
        track.course_table([[]])
    with pytest.raises(ValueError, match="point 1 is not two finite numbers"):
        track.course_table([[[0, 0], [0, 1e39]]])
    # the env-to-course map is `schedule_blocks`; an entry outside the table follows the nearest course, as the kernels clamp it
    np.testing.assert_array_equal(track.schedule_blocks(3, 2), [0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(track.course_of_envs([-5, 0, 1, 2, 3, 2 ** 31 - 1], 3), [0, 0, 1, 2, 2, 2])
    assert track.course_length([[3, 4]]) == 5.0 and track.course_length([[0.5, 0], [0.5, 0.5], [0, 0.5], [0, 0]]) == 2.0
    assert track.course_length([[0, 0]]) == 0.0


NINE = " | ".join(f"{k},0" for k in range(9))
REFUSALS = [
    (["--waypoints", " | "], "a course has 1 to 8 points, this one has 0"),
    (["--waypoints", ""], "a course has 1 to 8 points, this one has 0"),
    (["--waypoints", NINE], "a course has 1 to 8 points, this one has 9"),
    (["--waypoints", "0.5,0 | x,1"], "the point 'x,1' is not two numbers"),
    (["--waypoints", "0.5 0"], "'0.5 0' is not `x,y`"),
    (["--waypoints", "0.5,0,1"], "is not `x,y`"),
    (["--waypoints", "0.5,nan"], "point 0 is not two finite numbers"),
    (["--waypoints", "0.5,0", "--waypoints", "1,inf"], "point 0 is not two finite numbers"),
    (["--waypoints", "0.5,0", "--sequence", "0: 0 0 0"], "--waypoints does not combine with --sequence / --then.*both write the command buffer"),
    (["--waypoints", "0.5,0", "--command", "0", "0", "0", "--then", "0.1", "0", "0"], "--waypoints does not combine with --sequence / --then"),
    (["--waypoints", "0.5,0", "--command", "0.1", "0", "0"], "--waypoints does not combine with --command / --grid: the course is the command"),
    (["--waypoints", "0.5,0", "--grid", "vx=0:0.1:2"], "--waypoints does not combine with --command / --grid"),
    (["--waypoints", "0.5,0", "--push", "1", "0"], "--waypoints does not combine with --push / --push_grid.*one command per episode"),
    (["--waypoints", "0.5,0", "--push_grid", "magnitude=0:1:2"], "--waypoints does not combine with --push / --push_grid"),
    (["--waypoints", "0.5,0", "--posture"], "--waypoints does not combine with --posture.*one command per episode"),
    (["--waypoints", "0.5,0", "--waypoint_radius", "-0.1"], "--waypoint_radius is a finite number >= 0"),
    (["--waypoints", "0.5,0", "--waypoint_speed", "nan"], "--waypoint_speed is a finite number >= 0"),
    (["--waypoints", "0.5,0", "--waypoint_turn_rate", "inf"], "--waypoint_turn_rate is a finite number >= 0"),
    (["--waypoints", "0.5,0", "--waypoint_gain", "0"], "--waypoint_gain is a finite number > 0"),
    (["--waypoints", "0.5,0", "--waypoint_slow_dist", "0"], "--waypoint_slow_dist is a finite number > 0"),
]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_say_what_is_wrong(flags, message):
    """Each as `run` raises it: SystemExit before any batch is made (no GPU here, so getting that far would be another error)."""
    from open_duck_playground_amd import track
    args = track.build_parser().parse_args(["--checkpoint", "c.pt", "--episode_length", "100"] + flags)
    with pytest.raises(SystemExit, match=message):
        track.waypoints_from_args(args)
    with pytest.raises(SystemExit, match=message):
        track.run(args)


def test_speed_and_turn_rate_stay_inside_the_command_range():
    from open_duck_playground_amd import track
    rng = [[-0.15, 0.15], [-0.2, 0.2], [-1.0, 1.0]] + [[0.0, 0.0]] * 4      # the duck's Joystick cmd_range
    assert track.waypoint_limits_refusal(0.1, 0.6, rng) is None
    assert track.waypoint_limits_refusal(0.15, 1.0, rng) is None             # the ends belong to the range
    assert track.waypoint_limits_refusal(0.0, 0.0, rng) is None
    why = track.waypoint_limits_refusal(0.2, 0.6, rng)
    assert re.search(r"--waypoint_speed 0\.2 is beyond the env's command range for vx, -0\.15 \.\. 0\.15 m/s", why)
    why = track.waypoint_limits_refusal(0.1, 1.5, rng)
    assert re.search(r"--waypoint_turn_rate 1\.5 is beyond the env's command range for wz, -1\.0 \.\. 1\.0 rad/s", why)
    assert "wz" in track.waypoint_limits_refusal(0.1, 0.6, [[0, 0.15], [0, 0], [-0.5, 1.0]])      # a lopsided range: both signs are commanded
    standing = [[0.0, 0.0]] * 3 + [[-0.3, 0.3]] * 4                         # Standing has no move command: any speed is refused
    assert "vx, 0.0 .. 0.0" in track.waypoint_limits_refusal(0.1, 0.0, standing)


def test_the_flags_and_their_defaults():
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt"]
    args = track.build_parser().parse_args(base + ["--command", "0", "0", "0"])
    assert args.path is False and args.waypoints is None
    assert (args.waypoint_radius, args.waypoint_speed, args.waypoint_turn_rate, args.waypoint_gain, args.waypoint_slow_dist) == (0.05, 0.1, 0.6, 2.0, 0.1)
    assert track.waypoints_from_args(args) is None
    args = track.build_parser().parse_args(base + ["--waypoints", "0.5,0 | 0.5,0.5", "--waypoints", "0,1", "--waypoint_radius", "0.1", "--waypoint_speed", "0.12",
                                                   "--plant", "kp=0.8", "--gait", "--falls", "--imitation_report", "--path"])
    way = track.waypoints_from_args(args)
    assert way["courses"] == [[[0.5, 0.0], [0.5, 0.5]], [[0.0, 1.0]]] and way["radius"] == 0.1 and way["speed"] == 0.12 and way["turn_rate"] == 0.6
    assert way["gain"] == 2.0 and way["slow_dist"] == 0.1 and way["flags"] == dict(waypoints=["0.5,0 | 0.5,0.5", "0,1"])
    assert len(track.plants_from_args(args)) == 1                           # plants combine
    args = track.build_parser().parse_args(base + ["--waypoints=-0.05,0.05 | -0.1,0"])      # a leading minus sign needs the `=` form
    assert track.waypoints_from_args(args)["courses"] == [[[-0.05, 0.05], [-0.1, 0.0]]]
    help_text = " ".join(track.build_parser().format_help().split())
    for word in ("--path", "--waypoints", "--waypoint_radius", "--waypoint_speed", "--waypoint_turn_rate", "--waypoint_gain", "--waypoint_slow_dist",
                 "BUILD-DEFINED", "start frame"):
        assert word in help_text, word
    import inspect
    params = inspect.signature(track.Tracker.__init__).parameters
    assert params["path"].default is False and params["waypoints"].default is None


def test_a_plain_runs_key_sets_are_unchanged():
    from open_duck_playground_amd import track
    assert track.REPORT_KEYS == ("settings", "commands")
    assert track.ROW_KEYS == ("command", "mean_vx", "mean_vy", "mean_wz", "rms_error_vx", "rms_error_vy", "rms_error_wz", "fall_rate", "mean_episode_reward",
                              "mean_episode_steps", "steps", "velocity_samples", "envs")
    rows = track.reduce_tracking(np.zeros((4, 12), np.float32), [[0.0] * 7, [0.1] + [0.0] * 6], 2)
    assert all(tuple(r) == track.ROW_KEYS for r in rows)                    # no "path", no "course"
    assert track.PATH_KEYS == ("samples", "forward_m", "lateral_m", "heading_change_rad", "path_length_m", "straightness", "ideal", "error_vs_ideal_m")
    assert track.COURSE_KEYS == ("points", "completed_fraction", "waypoints", "cross_track_rms_m", "cross_track_peak_m", "final_goal_distance_m",
                                 "length_ratio", "falls_by_leg")
    assert track.COURSE_POINT_KEYS == ("point", "reached_fraction", "time_to_reach_s")
    # a Namespace of before these flags (what the existing tests build) asks for neither report
    old = types.SimpleNamespace(command=[[0.0, 0.0, 0.0]], grid=None, episode_length=10)
    assert track.waypoints_from_args(old) is None and not getattr(old, "path", False)


def _row(**slots):
    r = np.zeros(NACC, np.float32)
    for name, v in slots.items():
        v = np.atleast_1d(np.float32(v))
        r[SLOTS[name]:SLOTS[name] + len(v)] = v
    return r


def test_reduce_path_on_hand_built_rows():
    """A block of three envs that started at (1, 2) facing +y (heading (0, 1)): forward is world +y, lateral (left) is world -x.  Env 0 walked
    1 m forward and 0.25 m to its left along a path of 1.25 m; env 1 stood still (no straightness); env 2 ended before its first sample."""
    from open_duck_playground_amd import track
    dt = 0.02
    start = dict(START_X=1, START_Y=2, START_HX=0, START_HY=1)
    acc = np.stack([_row(**start, X=0.75, Y=3, LENGTH=1.25, TURN=0.5, SAMPLES=100), _row(**start, X=1, Y=2, LENGTH=0.004, TURN=-0.25, SAMPLES=50),
                    _row(**start, X=1, Y=2)])
    (g,) = track.reduce_path(acc, [[0.5, 0.0, 0.0, 0, 0, 0, 0]], 3, dt)
    assert tuple(g) == track.PATH_KEYS and json.loads(json.dumps(g)) == g
    ap = pytest.approx
    assert g["samples"] == 150
    assert g["forward_m"] == dict(mean=ap(1 / 3), std=ap(np.std([1, 0, 0])))
    assert g["lateral_m"] == dict(mean=ap(0.25 / 3), std=ap(np.std([0.25, 0, 0])))
    assert g["heading_change_rad"]["mean"] == ap(0.25 / 3) and g["path_length_m"]["mean"] == ap(1.254 / 3)
    assert g["straightness"] == dict(mean=ap(np.hypot(1, 0.25) / 1.25), std=0.0)      # over the one env that moved at least a centimetre
    # the ideal: 0.5 m/s straight for each env's own SAMPLES * dt = 2 s, 1 s, 0 s
    assert g["ideal"] == dict(forward_m=ap((1.0 + 0.5 + 0.0) / 3), lateral_m=0.0, heading_change_rad=0.0)
    assert g["error_vs_ideal_m"] == ap((0.25 + 0.5 + 0.0) / 3)
    # nobody moved: no straightness; a schedule or waypoint row: no ideal
    (h,) = track.reduce_path(acc[1:], [[0.0] * 7], 2, dt, constant=False)
    assert tuple(h) == track.PATH_KEYS and h["straightness"] is None and h["ideal"] is None and h["error_vs_ideal_m"] is None
    # blocks in order, each against its own command
    both = track.reduce_path(np.concatenate([acc, acc]), [[0.5] + [0.0] * 6, [0.0, 0.0, 0.5] + [0.0] * 4], 3, dt)
    assert both[0] == g and both[1]["ideal"]["forward_m"] == 0.0 and both[1]["ideal"]["heading_change_rad"] == ap(0.5 * (2 + 1 + 0) / 3)


def test_reduce_course_on_hand_built_rows():
    """One course of three points (polyline 0.5 + 0.5 + 0.5 m), five envs, dt 0.02: env 0 and env 1 complete it (reached at steps 30 / 60 / 95
    and 40 / 80 / 120); env 2 reaches the first waypoint at step 50 and falls heading for the second; env 3 falls heading for the first; env 4
    falls in step 0 before any sample."""
    from open_duck_playground_amd import track
    dt = 0.02
    pts = [[0.5, 0.0], [0.5, 0.5], [0.0, 0.5]]
    acc = np.stack([
        _row(LENGTH=1.8, WP_INDEX=3, XTRACK_SAMPLES=95, XTRACK_SQ=0.095, XTRACK_PEAK=0.05, GOAL_DIST=0.04, REACHED=(30, 60, 95)),
        _row(LENGTH=1.5, WP_INDEX=3, XTRACK_SAMPLES=120, XTRACK_SQ=0.12, XTRACK_PEAK=0.08, GOAL_DIST=0.02, REACHED=(40, 80, 120)),
        _row(LENGTH=0.7, WP_INDEX=1, XTRACK_SAMPLES=70, XTRACK_SQ=0.07, XTRACK_PEAK=0.2, GOAL_DIST=0.6, REACHED=(50, 0, 0), FELL=1, FELL_LEG=1),
        _row(LENGTH=0.1, WP_INDEX=0, XTRACK_SAMPLES=15, XTRACK_SQ=0.015, XTRACK_PEAK=0.03, GOAL_DIST=0.7, FELL=1, FELL_LEG=0),
        _row(FELL=1, FELL_LEG=0)])
    (g,) = track.reduce_course(acc, [pts], 5, dt)
    assert tuple(g) == track.COURSE_KEYS and json.loads(json.dumps(g)) == g
    assert all(tuple(w) == track.COURSE_POINT_KEYS for w in g["waypoints"])
    ap = pytest.approx
    assert g["points"] == pts and g["completed_fraction"] == ap(2 / 5)
    assert [w["point"] for w in g["waypoints"]] == pts
    assert [w["reached_fraction"] for w in g["waypoints"]] == [ap(3 / 5), ap(2 / 5), ap(2 / 5)]
    assert [w["time_to_reach_s"] for w in g["waypoints"]] == [ap(40 * dt), ap(70 * dt), ap(107.5 * dt)]      # medians of 30 40 50 | 60 80 | 95 120
    assert g["cross_track_rms_m"] == ap(np.sqrt(0.3 / 300)) and g["cross_track_peak_m"] == ap(0.2)
    assert g["final_goal_distance_m"] == ap((0.04 + 0.02 + 0.6 + 0.7) / 4)      # over the envs with a sample
    assert g["length_ratio"] == ap((1.8 / 1.5 + 1.5 / 1.5) / 2)                 # among the completers
    assert g["falls_by_leg"] == [2, 1, 0, 0]
    # nobody got anywhere: every figure over an empty set is None; a fall after the course was finished goes to the last entry
    (h,) = track.reduce_course(np.stack([_row(FELL=1), _row()]), [pts], 2, dt)
    assert h["completed_fraction"] == 0.0 and all(w["reached_fraction"] == 0.0 and w["time_to_reach_s"] is None for w in h["waypoints"])
    assert h["cross_track_rms_m"] is None and h["cross_track_peak_m"] is None and h["final_goal_distance_m"] is None and h["length_ratio"] is None
    assert h["falls_by_leg"] == [1, 0, 0, 0]
    (k,) = track.reduce_course(np.stack([_row(WP_INDEX=1, REACHED=(7,), LENGTH=0.3, FELL=1, FELL_LEG=1)]), [[[0.0, 0.0]]], 1, dt)
    assert k["completed_fraction"] == 1.0 and k["falls_by_leg"] == [0, 1] and k["length_ratio"] is None      # a course of zero length has no ratio
    # two courses: blocks in course order
    two = track.reduce_course(np.concatenate([acc, acc[:5]]), [pts, pts[:1]], 5, dt)
    assert two[0] == g and len(two[1]["waypoints"]) == 1 and two[1]["completed_fraction"] == ap(3 / 5)


@pytest.mark.parametrize("wz", [0.0, 1e-9, -1e-9, 0.5, -0.5])
def test_the_ideal_arc_equals_an_euler_integration(wz):
    """x' = vx cos psi - vy sin psi, y' = vx sin psi + vy cos psi, psi' = wz, integrated in float64 by Euler steps of h = 1e-4 s over 20 s.
    psi is linear in t, so it is exact at every time, and each step moves along the heading at its midpoint: with the heading at the step's
    start the sum is off by h / 2 |f(0) - f(T)| (Euler-Maclaurin), up to 1.6e-5 m here, which could not hold the closed form to 1e-6 m.
    What remains is second order, h^2 T |v| wz^2 / 24 < 1e-9 m, plus the rounding of 2e5 additions, < 1e-10 m: the closed form must agree
    within 1e-6 m."""
    from open_duck_playground_amd import track
    vx, vy, T, h = 0.15, -0.05, 20.0, 1e-4
    n = int(round(T / h))
    psi = wz * (np.arange(n) + 0.5) * h                   # the heading at each step's midpoint (psi is linear in t: exact)
    x = float(np.sum(vx * np.cos(psi) - vy * np.sin(psi)) * h)
    y = float(np.sum(vx * np.sin(psi) + vy * np.cos(psi)) * h)
    gx, gy, gpsi = track.ideal_pose([vx, vy, wz, 0, 0, 0, 0], T)
    assert abs(gx - x) < 1e-6 and abs(gy - y) < 1e-6 and gpsi == wz * T
    # arrays of times: each env its own
    ax, ay, _ = track.ideal_pose([vx, vy, wz], np.array([0.0, T]))
    assert ax[0] == 0.0 and ay[0] == 0.0 and ax[1] == gx and ay[1] == gy


def test_the_ideal_arc_is_continuous_at_zero_yaw_rate():
    from open_duck_playground_amd import track
    line = track.ideal_pose([0.15, -0.05, 0.0], 20.0)
    assert line[0] == pytest.approx(3.0, abs=1e-12) and line[1] == pytest.approx(-1.0, abs=1e-12)
    for wz in (1e-12, -1e-12, 1e-9, 1e-7):
        arc = track.ideal_pose([0.15, -0.05, wz], 20.0)
        # the arc leaves the line by |v| wz t^2 / 2 to first order
        assert np.hypot(arc[0] - line[0], arc[1] - line[1]) <= 1.01 * np.hypot(0.15, 0.05) * abs(wz) * 400 / 2 + 1e-12


def test_the_batch_methods_reject_bad_tensors_and_parameters():
    """The checks run before the library is touched, so a stand-in batch (no GPU) reaches them through the real methods."""
    import torch
    from open_duck_playground_amd import engine
    n = 8
    stub = types.SimpleNamespace(nenv=n, device=0, model=types.SimpleNamespace(nu=14), commands=None)
    tacc, acc, course, cmap = torch.zeros(n, engine.TRACK_NACC), torch.zeros(n, NACC), torch.zeros(2, COURSE_FLOATS), torch.zeros(n, dtype=torch.int32)
    bad_acc = ((np.zeros((n, NACC), np.float32), "torch tensor"), (torch.zeros(n, NACC - 1), "shape"), (torch.zeros(n + 1, NACC), "shape"),
               (torch.zeros(n, NACC, dtype=torch.float64), "dtype"), (torch.zeros(NACC, n).t(), "contiguous"), (acc, "cuda:0"))
    for t, what in bad_acc:
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.path_begin(stub, t)
        assert "path_begin: acc" in str(ei.value)
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.path_accumulate(stub, t, tacc)
        assert "path_accumulate: acc" in str(ei.value)
    bad_course = ((np.zeros((2, COURSE_FLOATS), np.float32), "course: expected a torch tensor"), (torch.zeros(2, 16), "course: shape"),
                  (torch.zeros(0, COURSE_FLOATS), "course: shape"), (torch.zeros(COURSE_FLOATS), "course: shape"),
                  (torch.zeros(2, COURSE_FLOATS, dtype=torch.float64), "course: dtype"), (torch.zeros(COURSE_FLOATS, 2).t(), "course: the tensor must be contiguous"),
                  (course, "course: the tensor must live on cuda:0"))
    for t, what in bad_course:
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.waypoint_command_apply(stub, t, cmap, tacc, acc, 0.1, 0.6, 2.0, 0.1)
        assert "waypoint_command_apply" in str(ei.value)
    # the map and the parameters through the functions the methods call (a table that passes must claim to be on the device)
    dev = types.SimpleNamespace(type="cuda", index=0)

    class OnDevice:
        def __init__(self, t):
            self.t = t
        shape = property(lambda self: self.t.shape)
        dtype = property(lambda self: self.t.dtype)
        device = dev
        dim = lambda self: self.t.dim()
        is_contiguous = lambda self: self.t.is_contiguous()

    real = torch.is_tensor
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(torch, "is_tensor", lambda x: isinstance(x, OnDevice) or real(x))
        assert engine.check_courses("x", OnDevice(course), OnDevice(cmap), n, 0) == 2
        for m, what in ((torch.zeros(n + 1, dtype=torch.int32), "course_of_env: shape"), (torch.zeros(n, dtype=torch.int64), "course_of_env: dtype"),
                        (torch.zeros(2 * n, dtype=torch.int32)[::2], "course_of_env: the tensor must be contiguous")):
            with pytest.raises(engine.OdkError, match=what):
                engine.check_courses("x", OnDevice(course), OnDevice(m), n, 0)
        with pytest.raises(engine.OdkError, match="course_of_env: the tensor must live on cuda:0"):
            engine.check_courses("x", OnDevice(course), cmap, n, 0)
        with pytest.raises(engine.OdkError, match="course_of_env: expected a torch tensor"):
            engine.check_courses("x", OnDevice(course), None, n, 0)
    finally:
        mp.undo()
    for v in (-0.1, float("nan"), float("inf"), "fast", None):
        with pytest.raises(engine.OdkError, match="f: speed = .*(a finite number >= 0|is not a number)"):
            engine.check_path_parameter("f", "speed", v)
    with pytest.raises(engine.OdkError, match="a finite number > 0"):
        engine.check_path_parameter("f", "gain", 0.0, True)
    assert engine.check_path_parameter("f", "speed", 0) == 0.0 and engine.check_path_parameter("f", "gain", 2, True) == 2.0
