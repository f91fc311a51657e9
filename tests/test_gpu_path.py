"""GPU checks of the path report and the waypoint follower (odk_path_begin, odk_path_accumulate, odk_waypoint_command_apply and their
`Batch` methods) and of `track --path` / `track --waypoints`: every float against a float32 numpy restatement written from the text of
include/odk.h, bit for bit -- the start poses of placed states, the follower's command on synthetic states in which every branch is
somebody's, the accumulator over a real rollout with falls, survivors and reached waypoints -- then the closed loop (eager, captured, and
against a replayed command buffer), the report and the refusals.

One refusal of the C entries has no test: a model whose first joint is not a free joint (ODK_ERR_UNSUPPORTED).  No such model loads (the
loader takes a floating base with serial chains below it and refuses anything else), so no batch of one exists to hand to the calls."""
import ctypes as C
import json

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

G = RC.HEADER         # include/odk.h's constants: G.PATH_*, G.TRACK_*
f32 = np.float32


def pose32(q):
    """The pose of include/odk.h from qpos[0:7]: (x, y, hx, hy), every operation one float32 operation."""
    w, x, y, z = (f32(v) for v in q[3:7])
    hx = f32(1) - f32(2) * (y * y + z * z)
    hy = f32(2) * (x * y + w * z)
    n = RC.planar32(hx, hy)
    if n < f32(1e-6):
        return f32(q[0]), f32(q[1]), f32(1), f32(0)
    return f32(q[0]), f32(q[1]), f32(hx / n), f32(hy / n)


def begin32(qpos, acc0):
    """odk_path_begin over qpos [n, nq] into a copy of acc0 ([rows >= n, 32]: rows past n keep their floats)."""
    A = np.array(acc0, f32)
    for e in range(len(qpos)):
        p = pose32(qpos[e])
        A[e] = 0
        A[e, G.PATH_START_X:G.PATH_START_X + 4] = p
        A[e, G.PATH_X:G.PATH_X + 4] = p
    return A


def course_of(tab, cmap, e):
    """(count, points [8, 2]) of env e's course, the map entry and the count clamped as the kernels clamp them"""
    W = tab[min(max(int(cmap[e]), 0), len(tab) - 1)]
    return min(max(int(W[0]), 0), G.PATH_MAX_WAYPOINTS), W[1:].reshape(G.PATH_MAX_WAYPOINTS, 2)


def start_frame(A, p):
    """(xs, ys): the start-frame position of pose p against row A's start"""
    shx, shy = A[G.PATH_START_HX], A[G.PATH_START_HY]
    rx, ry = f32(p[0] - A[G.PATH_START_X]), f32(p[1] - A[G.PATH_START_Y])
    return f32(f32(rx * shx) + f32(ry * shy)), f32(f32(shx * ry) - f32(shy * rx))


def accumulate32(A, steps, ended, qpos, done, trunc, tab, cmap, radius):
    """One odk_path_accumulate launch followed by odk_tracking_accumulate's ENDED / STEPS bookkeeping, in place: A [n, 32], steps and ended
    [n], qpos [n, nq] (the state this step left), done / trunc [n]; tab None: the odometry mode."""
    radius = f32(radius)
    for e in range(len(qpos)):
        if ended[e]:
            continue
        R, st = A[e], steps[e]
        steps[e] += f32(1)
        if done[e] != 0:
            if trunc[e] == 0:
                R[G.PATH_FELL], R[G.PATH_FELL_LEG] = f32(1), R[G.PATH_WP_INDEX]
            ended[e] = True
            continue
        p = pose32(qpos[e])
        R[G.PATH_LENGTH] = f32(R[G.PATH_LENGTH] + RC.planar32(f32(p[0] - R[G.PATH_X]), f32(p[1] - R[G.PATH_Y])))
        R[G.PATH_TURN] = f32(R[G.PATH_TURN] + f32(f32(R[G.PATH_HX] * p[3]) - f32(R[G.PATH_HY] * p[2])))
        R[G.PATH_SAMPLES] = f32(R[G.PATH_SAMPLES] + f32(1))
        R[G.PATH_X:G.PATH_X + 4] = p
        if tab is None:
            continue
        count, pts = course_of(tab, cmap, e)
        i = max(int(R[G.PATH_WP_INDEX]), 0)
        if i >= count:
            continue
        xs, ys = start_frame(R, p)
        wx, wy = pts[i]
        px, py = pts[i - 1] if i > 0 else (f32(0), f32(0))
        dist = RC.planar32(f32(wx - xs), f32(wy - ys))
        ax, ay, qx, qy = f32(wx - px), f32(wy - py), f32(xs - px), f32(ys - py)
        len2 = f32(f32(ax * ax) + f32(ay * ay))
        u = f32(0)
        if len2 > 0:
            u = f32(f32(f32(qx * ax) + f32(qy * ay)) / len2)
            u = min(max(u, f32(0)), f32(1))
        xt = RC.planar32(f32(qx - f32(u * ax)), f32(qy - f32(u * ay)))
        R[G.PATH_XTRACK_SAMPLES] = f32(R[G.PATH_XTRACK_SAMPLES] + f32(1))
        R[G.PATH_XTRACK_SQ] = f32(R[G.PATH_XTRACK_SQ] + f32(xt * xt))
        R[G.PATH_XTRACK_PEAK] = max(R[G.PATH_XTRACK_PEAK], xt)
        gx, gy = pts[count - 1]
        R[G.PATH_GOAL_DIST] = RC.planar32(f32(gx - xs), f32(gy - ys))
        if dist <= radius:
            R[G.PATH_REACHED + i] = f32(st + f32(1))
            R[G.PATH_WP_INDEX] = f32(i + 1)


def command32(Trow, A, q, count, pts, v_cruise, turn_rate, gain, slow_dist):
    """odk_waypoint_command_apply for one env: ((vx, vy, wz) or None for a row that is not written, the set of branches taken)."""
    v_cruise, turn_rate, gain, slow_dist = f32(v_cruise), f32(turn_rate), f32(gain), f32(slow_dist)
    if Trow[G.TRACK_ENDED] != 0:
        return None, {"ended"}
    took = set()
    xs = ys = s = f32(0)
    c, i = f32(1), 0
    if Trow[G.TRACK_STEPS] != 0:
        p = pose32(q)
        xs, ys = start_frame(A, p)
        shx, shy = A[G.PATH_START_HX], A[G.PATH_START_HY]
        c = f32(f32(shx * p[2]) + f32(shy * p[3]))
        s = f32(f32(shx * p[3]) - f32(shy * p[2]))
        i = min(max(int(A[G.PATH_WP_INDEX]), 0), count)
    else:
        took.add("clock0")
    if i >= count:
        return (f32(0), f32(0), f32(0)), took | {"finished"}
    dx, dy = f32(pts[i][0] - xs), f32(pts[i][1] - ys)
    dist = RC.planar32(dx, dy)
    if dist < f32(1e-6):
        f, l = f32(1), f32(0)
        took.add("on_target")
    else:
        f = f32(f32(f32(dx * c) + f32(dy * s)) / dist)
        l = f32(f32(f32(c * dy) - f32(s * dx)) / dist)
        side = "" if l == 0 else ("_left" if l > 0 else "_right")
        took.add(("ahead" if f >= 0 else ("behind" if side else "exactly_behind")) + side)
    turn = l if f >= 0 else (f32(1) if l >= 0 else f32(-1))
    wz = f32(gain * turn)
    if wz > turn_rate:
        wz = turn_rate
        took.add("saturated_left")
    elif wz < -turn_rate:
        wz = f32(-turn_rate)
        took.add("saturated_right")
    else:
        took.add("unsaturated")
    vx = f32(v_cruise * (f if f > 0 else f32(0)))
    if i == count - 1:
        took.add("last_waypoint")
        vx = f32(vx * min(f32(1), f32(dist / slow_dist)))
        if dist < slow_dist:
            took.add("slowed")
    elif dist < slow_dist:
        took.add("near_a_waypoint_that_is_not_the_last")
    return (vx, f32(0), wz), took


BRANCHES = {"ended", "clock0", "finished", "on_target", "ahead", "ahead_left", "ahead_right", "behind_left", "behind_right", "exactly_behind",
            "saturated_left", "saturated_right", "unsaturated", "last_waypoint", "slowed", "near_a_waypoint_that_is_not_the_last"}


def _duck(n, **overrides):
    return RC.robot_env("duck", n, config_overrides=overrides or None)


def quat(yaw=0.0, pitch=0.0, roll=0.0):
    """w x y z of Rz(yaw) Ry(pitch) Rx(roll), float64"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr])


N_SYN = 300      # two blocks of 256 threads, the second partly idle


def test_begin_takes_the_start_pose_of_every_env():
    """300 duck envs with placed poses by e % 6: the reset's own | yawed | tilted in roll and pitch | yawed and tilted | pitched 90 degrees
    (the heading vector vanishes: (1, 0)) | yawed, then pitched 90 degrees.  The accumulator starts as 9.0 everywhere and is two rows longer
    than the batch: every row has the restatement's bits, the guard rows keep theirs."""
    import torch
    n = N_SYN
    env = _duck(n)
    b = env.batch
    env.reset(3)
    torch.cuda.synchronize()
    qpos = b.get_state()[0]
    rng = np.random.default_rng(11)
    for e in range(n):
        k = e % 6
        yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)
        if k:
            qpos[e, 0:2] = rng.uniform(-2, 2, 2)
            qpos[e, 3:7] = quat(yaw if k in (1, 3, 5) else 0.0, np.pi / 2 if k >= 4 else (pitch if k in (2, 3) else 0.0), roll if k in (2, 3) else 0.0)
    b.set_state(qpos)
    acc0 = np.full((n + 2, G.PATH_NACC), 9.0, f32)
    want = begin32(qpos, acc0)
    big = torch.tensor(acc0, device="cuda")
    b.path_begin(big[:n])
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(got[n:], 9.0)
    # the placement covers what it claims to
    h = want[:n, G.PATH_START_HX:G.PATH_START_HX + 2]
    np.testing.assert_allclose(np.hypot(h[:, 0], h[:, 1]), 1.0, atol=1e-6)
    degenerate = np.arange(n) % 6 >= 4
    np.testing.assert_array_equal(h[degenerate], np.tile(f32([1, 0]), (degenerate.sum(), 1)))
    assert np.all(h[np.arange(n) % 6 == 1, 1] != 0) and np.all(want[:n, G.PATH_LENGTH:] == 0) and np.all(want[:n, G.PATH_X:G.PATH_X + 4] == want[:n, G.PATH_START_X:G.PATH_START_X + 4])
    tilted = np.arange(n) % 6 == 2      # no yaw: pitch shortens the heading vector, roll does not move it; normalised it stays +x
    np.testing.assert_allclose(h[tilted], np.tile(f32([1, 0]), (tilted.sum(), 1)), atol=1e-6)
    b.close()


PARAMS = (0.1, 0.6, 2.0, 0.1)      # v_cruise, turn_rate, heading_gain, slow_dist
# the synthetic states, by (e // 3) % 13: bearing of the target in the body frame (degrees), distance, the waypoint index (None: by rotation)
CASES = (("clock0", 70.0, 0.4, None), ("ahead", 0.0, 0.5, None), ("ahead_left", 30.0, 0.4, None), ("ahead_right", -40.0, 0.4, None),
         ("behind_left", 150.0, 0.4, None), ("behind_right", -120.0, 0.4, None), ("exactly_behind", 180.0, 0.25, None), ("on_target", 0.0, 0.0, None),
         ("slow_last", 10.0, 0.04, "last"), ("near_first", 10.0, 0.04, "first"), ("finished", 0.0, 0.3, "count"), ("ended", 20.0, 0.3, None),
         ("gentle", 5.0, 0.4, None))
EXACT = ("ahead", "exactly_behind", "on_target")      # placed in the identity frame with exactly representable numbers


def _synthetic_states():
    n = N_SYN
    rng = np.random.default_rng(5)
    courses = [[[0.5, 0.25]], [[0.5, 0.0], [0.5, 0.5], [-0.25, 0.5]], [[0.25 * (k + 1), 0.125 * (k % 3)] for k in range(8)]]
    tab = np.zeros((3, G.PATH_COURSE_FLOATS), f32)
    for c, pts in enumerate(courses):
        tab[c, 0] = len(pts)
        tab[c, 1:1 + 2 * len(pts)] = f32(pts).reshape(-1)
    cmap = np.array([e % 3 for e in range(n)], np.int32)
    cmap[290:] = [-1, 7, 3, -5, 100, -1, 7, 3, -5, 100]                       # outside 0 .. 2: clamped, never read past the table
    tacc = np.zeros((n, G.TRACK_NACC), f32)
    tacc[:, G.TRACK_SAMPLES:] = rng.normal(size=(n, G.TRACK_NACC - G.TRACK_SAMPLES)).astype(f32)      # the other slots are not the launch's business
    pacc = rng.normal(size=(n, G.PATH_NACC)).astype(f32)                            # nor are the path accumulator's sums
    qpos7 = np.zeros((n, 7))
    for e in range(n):
        name, bearing, dist, which = CASES[(e // 3) % len(CASES)]
        count, pts = course_of(tab, cmap, e)
        i = {"last": count - 1, "first": 0, "count": count, None: (e // (3 * len(CASES))) % count}[which]
        tacc[e, G.TRACK_STEPS], tacc[e, G.TRACK_ENDED] = (0.0 if name == "clock0" else 1.0 + e % 7), (1.0 if name == "ended" else 0.0)
        pacc[e, G.PATH_WP_INDEX] = i
        exact = name in EXACT
        yaw0, s0 = (0.0, np.zeros(2)) if exact else (rng.uniform(-np.pi, np.pi), rng.uniform(-1, 1, 2))
        psi = 0.0 if exact else rng.uniform(-np.pi, np.pi)                    # the start-frame heading
        w = np.float64(pts[min(i, count - 1)])
        th = psi + np.deg2rad(bearing)
        towards = np.array([-1.0 if bearing else 1.0, 0.0]) if exact else np.array([np.cos(th), np.sin(th)])
        at = w - dist * towards                                               # the start-frame position
        R = np.array([[np.cos(yaw0), -np.sin(yaw0)], [np.sin(yaw0), np.cos(yaw0)]])
        qpos7[e, 0:2] = s0 + R @ at
        qpos7[e, 2] = 0.15
        tilt = (0.0, 0.0) if exact else rng.uniform(-0.2, 0.2, 2)
        qpos7[e, 3:7] = quat(yaw0 + psi, *tilt)
        start = (s0[0], s0[1], np.cos(yaw0), np.sin(yaw0))
        pacc[e, G.PATH_START_X:G.PATH_START_X + 4] = np.nan if name == "clock0" else f32(start)      # at clock 0 the start slots are not read
    return dict(tab=tab, cmap=cmap, tacc=tacc, pacc=pacc, qpos7=qpos7.astype(f32))


def test_apply_writes_the_followers_command_on_synthetic_states():
    """300 envs, courses of 1, 3 and 8 points, poses placed so that every branch of the follower is somebody's (CASES), the last ten map
    entries outside the table.  Entries 0..2 of every live row have the restatement's bits; entries 3..6, the rows of ended envs and the guard
    rows keep the 9.0 they held; the clock and the path accumulator are read, not written; and with rows 9 floats apart (the C binding)
    columns 7..8 keep theirs."""
    import torch
    from open_duck_playground_amd import engine
    n, s = N_SYN, _synthetic_states()
    tab, cmap, tacc, pacc = s["tab"], s["cmap"], s["tacc"], s["pacc"]
    env = _duck(n)
    b = env.batch
    env.reset(3)
    torch.cuda.synchronize()
    qpos = b.get_state()[0]
    qpos[:, :7] = s["qpos7"]
    b.set_state(qpos)
    want, written, seen, clock0 = np.full((n, 3), 9.0, f32), np.zeros(n, bool), set(), {}
    for e in range(n):
        cmd, took = command32(tacc[e], pacc[e], qpos[e], *course_of(tab, cmap, e), *PARAMS)
        seen |= took
        if cmd is not None:
            want[e], written[e] = cmd, True
        if "clock0" in took:
            clock0.setdefault(min(max(int(cmap[e]), 0), 2), []).append(cmd)
    assert seen == BRANCHES, (BRANCHES - seen, seen - BRANCHES)               # every branch occurred
    assert sorted(clock0) == [0, 1, 2] and all(len(v) > 1 and len(set(v)) == 1 for v in clock0.values())      # clock 0: the table alone decides
    assert 10 < (~written).sum() < 60 and np.all(want[written, 1] == 0)
    sat = np.abs(want[written, 2]) == f32(PARAMS[1])
    assert sat.sum() > 50 and (~sat).sum() > 50 and (want[written, 0] == 0).sum() > 20 and (want[written, 0] == f32(PARAMS[0])).sum() > 5

    tab_d, cmap_d, tacc_d, pacc_d = (torch.tensor(x, device="cuda") for x in (tab, cmap, tacc, pacc))
    guard = torch.full((n + 2, 7), 9.0, device="cuda")                        # rows past the batch: the second block's idle threads leave them
    cmd = guard[:n]
    b.bind_commands(cmd)
    b.waypoint_command_apply(tab_d, cmap_d, tacc_d, pacc_d, *PARAMS)
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    np.testing.assert_array_equal(got[:n, :3].view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(got[:n, 3:], 9.0)
    np.testing.assert_array_equal(got[n:], 9.0)
    np.testing.assert_array_equal(tacc_d.cpu().numpy().view(np.int32), tacc.view(np.int32))
    np.testing.assert_array_equal(pacc_d.cpu().numpy().view(np.int32), pacc.view(np.int32))

    # rows 9 floats apart, through the C binding
    L = engine.load_library()
    wide = torch.full((n, 9), 9.0, device="cuda")
    assert L.odk_batch_bind_commands(b._b, C.c_void_p(wide.data_ptr()), 9) == 0
    rc = L.odk_waypoint_command_apply(b._b, C.c_void_p(tab_d.data_ptr()), 3, C.c_void_p(cmap_d.data_ptr()), C.c_void_p(tacc_d.data_ptr()),
                                      C.c_void_p(pacc_d.data_ptr()), *(C.c_float(x) for x in PARAMS), b._stream())
    assert rc == 0, L.odk_last_error().decode()
    torch.cuda.synchronize()
    got = wide.cpu().numpy()
    np.testing.assert_array_equal(got[:, :3].view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(got[:, 3:], 9.0)
    b.bind_commands(None)
    b.close()


# ---- a real rollout.  Actions, kicks and the course were chosen on the CPU oracle (oracle.OracleEnv per env, reset seed 1, push_enable 0,
# the kick added to qvel[0:2] before step 5): see test_accumulate_over_a_real_rollout
ROLL_N, ROLL_T, ROLL_EPISODE, ROLL_SEED, KICK_AT, RADIUS = 67, 80, 60, 1, 5, 0.05
COURSE = [[-0.08, 0.0], [-0.18, 0.0], [-0.25, -0.05]]


def _roll_actions(nu):
    """One sequence of uniform actions for all envs, scaled per env from 0 (env 0) to 1 (the last env)."""
    seq = np.random.default_rng(ROLL_SEED).uniform(-1, 1, (ROLL_T, 1, nu)).astype(f32)
    return (seq * np.linspace(0.0, 1.0, ROLL_N, dtype=f32)[None, :, None]).astype(f32)


def _kicks():
    """Every third env is kicked with 0.8 m/s, env e towards e radians in the world frame."""
    k = np.zeros((ROLL_N, 2), f32)
    for e in range(0, ROLL_N, 3):
        k[e] = 0.8 * np.cos(e), 0.8 * np.sin(e)
    return k


def test_accumulate_over_a_real_rollout():
    """67 duck envs, 80 eager steps, episode_length 60.  Env e gets e / 66 times one uniform(-1, 1) action sequence; every third env is kicked
    at step 5 through the bound push buffer.  On the CPU oracle this gives 45 first episodes that fall and 22 that are truncated at step
    59, and the falling robots mostly go backwards: of the course (-0.08, 0) (-0.18, 0) (-0.25, -0.05) with radius 0.05, 33 oracle envs
    reach the first point, 22 the second and 8 all three.  4 falls, 4 survivors, 4 envs at the first point and 1 completer are asked for
    here.  `get_state` after every step feeds the restatement; two accumulators ride the same rollout, one with the course and one
    without (course_dev = NULL), and every slot of every row of both has the restatement's bits after every step."""
    import torch
    from open_duck_playground_amd import engine
    n, T = ROLL_N, ROLL_T
    env = _duck(n, episode_length=ROLL_EPISODE)
    b = env.batch
    tab = np.zeros((1, G.PATH_COURSE_FLOATS), f32)
    tab[0, 0], tab[0, 1:7] = 3, f32(COURSE).reshape(-1)
    cmap = np.zeros(n, np.int32)
    tab_d, cmap_d = torch.tensor(tab, device="cuda"), torch.tensor(cmap, device="cuda")
    b.bind_commands(torch.tensor(np.tile(f32([0.1, 0, 0, 0, 0, 0, 0]), (n, 1)), device="cuda"))
    push, kicks = torch.zeros(n, 2, device="cuda"), torch.tensor(_kicks(), device="cuda")
    b.bind_pushes(push)
    env.reset(ROLL_SEED)
    acc_c, acc_o = torch.full((n, G.PATH_NACC), 7.0, device="cuda"), torch.full((n, G.PATH_NACC), 7.0, device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    b.path_begin(acc_c)
    b.path_begin(acc_o)
    torch.cuda.synchronize()
    want_c = begin32(b.get_state()[0], np.full((n, G.PATH_NACC), 7.0, f32))
    want_o = want_c.copy()
    np.testing.assert_array_equal(acc_c.cpu().numpy().view(np.int32), want_c.view(np.int32))
    steps_c, ended_c, steps_o, ended_o = np.zeros(n, f32), np.zeros(n, bool), np.zeros(n, f32), np.zeros(n, bool)
    acts = torch.tensor(_roll_actions(b.model.nu), device="cuda")
    with torch.no_grad():
        for t in range(T):
            push.copy_(kicks) if t == KICK_AT else push.zero_()
            b.step(acts[t].contiguous())
            before = tacc.clone()
            b.path_accumulate(acc_c, tacc, tab_d, cmap_d, RADIUS)
            b.path_accumulate(acc_o, tacc)
            assert torch.equal(tacc.view(torch.int32), before.view(torch.int32))      # the clock is read, not written
            b.tracking_accumulate(tacc)
            torch.cuda.synchronize()
            done, trunc, qpos = b.done.cpu().numpy(), b.truncation.cpu().numpy(), b.get_state()[0]
            accumulate32(want_c, steps_c, ended_c, qpos, done, trunc, tab, cmap, RADIUS)
            accumulate32(want_o, steps_o, ended_o, qpos, done, trunc, None, None, 0.0)
            np.testing.assert_array_equal(acc_c.cpu().numpy().view(np.int32), want_c.view(np.int32), err_msg=f"course, step {t}")
            np.testing.assert_array_equal(acc_o.cpu().numpy().view(np.int32), want_o.view(np.int32), err_msg=f"odometry, step {t}")
    got, odo, tr = acc_c.cpu().numpy(), acc_o.cpu().numpy(), tacc.cpu().numpy()
    np.testing.assert_array_equal(tr[:, G.TRACK_STEPS], steps_c)
    fell, first, all3 = got[:, G.PATH_FELL] != 0, got[:, G.PATH_REACHED] > 0, got[:, G.PATH_WP_INDEX] == 3
    print(f"fell {int(fell.sum())}, survived {int((~fell).sum())}, reached the first point {int(first.sum())}, the second "
          f"{int((got[:, G.PATH_REACHED + 1] > 0).sum())}, all three {int(all3.sum())}")
    assert fell.sum() >= 4 and (~fell).sum() >= 4 and first.sum() >= 4 and all3.sum() >= 1
    assert np.all(ended_c) and (got[fell, G.PATH_FELL_LEG] > 0).any() and (got[fell, G.PATH_FELL_LEG] == 0).any()
    # the odometry slots do not depend on the course, and without one the course slots stay 0
    np.testing.assert_array_equal(odo[:, :G.PATH_FELL + 1].view(np.int32), got[:, :G.PATH_FELL + 1].view(np.int32))
    assert np.all(odo[:, G.PATH_FELL_LEG:] == 0) and np.all(got[:, G.PATH_REACHED + 3:] == 0)
    assert np.all(got[:, G.PATH_SAMPLES] == tr[:, G.TRACK_SAMPLES]) and got[:, G.PATH_LENGTH].max() > 0.2 and np.all(got[:, G.PATH_XTRACK_SAMPLES] <= got[:, G.PATH_SAMPLES])
    reached = got[:, G.PATH_REACHED:G.PATH_REACHED + 3]
    assert np.all((reached[:, 1] == 0) | (reached[:, 1] > reached[:, 0])) and np.all((reached[:, 2] == 0) | (reached[:, 2] > reached[:, 1]))
    b.bind_pushes(None)
    b.bind_commands(None)
    b.close()


# ---- the closed loop
LOOP_N, LOOP_T, LOOP_SEED, LOOP_RING = 32, 40, 2, 8
LOOP_COURSES = [[[0.1, 0.0], [0.1, 0.1]], [[-0.05, 0.05]]]


def _tracker(track, waypoints, commands=None):
    import torch
    from open_duck_playground_amd.ppo.networks import PPONetworks
    env = _duck(LOOP_N, episode_length=LOOP_T)
    torch.manual_seed(0)
    net = PPONetworks(101, 212, 14).cuda()
    cmd = torch.zeros(LOOP_N, 7, device="cuda") if commands is None else commands
    env.set_commands(cmd)
    falls = dict(ring=LOOP_RING, tilt_tol=track.fall_tilt_tol(0.35))
    way = dict(table=track.course_table(LOOP_COURSES), map=track.schedule_blocks(2, LOOP_N // 2)) if waypoints else None
    return track.Tracker(env, net, gait=True, falls=falls, waypoints=way, use_graph=waypoints == "graph"), cmd


def _closed_loop(track, mode):
    """40 steps of the follower on 32 envs; per step the command buffer and the command entries of the observation the step wrote."""
    import torch
    tr, cmd = _tracker(track, mode)
    hist = []
    with torch.no_grad():
        tr.reset(LOOP_SEED)
        torch.cuda.synchronize()
        at_reset = cmd.cpu().numpy().copy()
        for _ in range(LOOP_T):
            tr.step()
            torch.cuda.synchronize()
            hist.append((cmd.cpu().numpy().copy(), tr.env.batch.obs[:, 6:13].cpu().numpy()))
    out = dict(at_reset=at_reset, cmds=np.stack([h[0] for h in hist]), obs=np.stack([h[1] for h in hist]), graph=tr.graph is not None,
               **{k: getattr(tr, k).cpu().numpy() for k in ("acc", "path_acc", "gait_acc", "fall_acc")})
    tr.env.set_commands(None)
    tr.env.batch.close()
    return out


def test_the_closed_loop_eager_captured_and_replayed():
    """A randomly initialised policy steered over two courses, alongside `gait` and `falls`.  The captured run has the eager run's
    accumulators and command buffers; at every step the command entries of the observation equal the buffer's row (the step followed
    what the launch wrote); and a Tracker without the follower, whose bound buffer is filled from the eager run's recording before the
    reset and before every step, leaves the gait, fall and tracking accumulators with the same bits."""
    import torch
    from open_duck_playground_amd import track
    e = _closed_loop(track, "eager")
    assert not e["graph"]
    np.testing.assert_array_equal(e["at_reset"][:, 3:], 0.0)
    first = e["at_reset"][:, :3]
    assert np.all(first[:16] == f32([0.1, 0, 0])) and np.all(first[16:, 2] == f32(0.6)) and np.all(first[16:, 0] == 0)      # ahead | behind on the left
    for t in range(LOOP_T):
        np.testing.assert_array_equal(e["obs"][t].view(np.int32), e["cmds"][t].view(np.int32), err_msg=f"step {t}")
    assert len({c.tobytes() for c in e["cmds"]}) > LOOP_T // 2 and np.all(e["cmds"][:, :, 1] == 0) and np.all(e["cmds"][:, :, 3:] == 0)
    assert np.abs(e["cmds"][:, :, 2]).max() <= f32(0.6) and e["cmds"][:, :, 0].max() < 0.1001 and e["cmds"][:, :, 0].min() >= 0
    assert e["path_acc"][:, G.PATH_SAMPLES].sum() > 0 and e["gait_acc"].any() and e["fall_acc"].any()
    g = _closed_loop(track, "graph")
    assert g["graph"]
    for k in ("at_reset", "cmds", "obs", "acc", "path_acc", "gait_acc", "fall_acc"):
        np.testing.assert_array_equal(g[k].view(np.int32), e[k].view(np.int32), err_msg=k)
    # the same commands from a plain buffer: the reports beside the follower do not see the difference
    cmd = torch.tensor(e["at_reset"], device="cuda")
    tr, _ = _tracker(track, None, commands=cmd)
    with torch.no_grad():
        tr.reset(LOOP_SEED)
        for t in range(LOOP_T):
            cmd.copy_(torch.tensor(e["cmds"][t], device="cuda"))
            tr.step()
    torch.cuda.synchronize()
    assert tr.path_acc is None and tr.course is None
    for k in ("acc", "gait_acc", "fall_acc"):
        np.testing.assert_array_equal(getattr(tr, k).cpu().numpy().view(np.int32), e[k].view(np.int32), err_msg=k)
    tr.env.set_commands(None)
    tr.env.batch.close()


# ---- track --path / --waypoints
def _run(track, monkeypatch, argv, eager=False):
    """RC.run_track recording the state after the reset and the flags and state after every step."""
    import torch

    def after_reset(tr):
        torch.cuda.synchronize()
        return tr.env.batch.get_state()[0]

    def after_step(tr, _):
        b = tr.env.batch
        return b.done.cpu().numpy(), b.truncation.cpu().numpy(), b.get_state()[0]

    return RC.run_track(track, monkeypatch, argv, eager, after_step=after_step, after_reset=after_reset)


def test_track_path_equals_the_reduction_of_the_restatement(tmp_path, monkeypatch):
    """`--path` on two `--command` rows, 8 envs each, 40 steps: the eager run's recording pushed through the restatement has the path
    accumulator's bits, so each row's "path" is `reduce_path` of it; the captured run has the same bits and rows."""
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T = 8, 40
    cmds = [[0.1, 0.0, 0.0], [0.0, 0.05, 0.5]]
    argv = ["--checkpoint", ckpt, "--command", *map(str, cmds[0]), "--command", *map(str, cmds[1]), "--envs_per_command", str(E), "--episode_length", str(T),
            "--seed", "3", "--path", "--output", str(tmp_path / "r.json")]
    rep, tr, hist = _run(track, monkeypatch, argv, eager=True)
    assert len(hist) == T + 1 and rep["settings"]["path"] is True and not rep["settings"]["graph"]
    want = begin32(hist[0], np.zeros((2 * E, G.PATH_NACC), f32))
    steps, ended = np.zeros(2 * E, f32), np.zeros(2 * E, bool)
    for done, trunc, qpos in hist[1:]:
        accumulate32(want, steps, ended, qpos, done, trunc, None, None, 0.0)
    got = tr.path_acc.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    assert got[:, G.PATH_SAMPLES].sum() > 0 and tr.course is None
    rows = [track.command_row(c) for c in cmds]
    ref = track.reduce_path(want, rows, E, rep["settings"]["dt"])
    for row, cmd, path in zip(rep["commands"], rows, ref):
        assert tuple(row) == track.ROW_KEYS + ("path",) and row["command"] == cmd
        assert tuple(row["path"]) == track.PATH_KEYS and row["path"] == path and row["path"]["samples"] == row["velocity_samples"]
        assert row["path"]["ideal"] is not None and row["path"]["error_vs_ideal_m"] >= 0
    assert json.load(open(tmp_path / "r.json")) == json.loads(json.dumps(rep))
    rep_g, tr_g, _ = _run(track, monkeypatch, argv)
    assert rep_g["settings"]["graph"] and rep_g["commands"] == rep["commands"]
    np.testing.assert_array_equal(tr_g.path_acc.cpu().numpy().view(np.int32), got.view(np.int32))


def test_track_waypoints_has_the_pinned_keys(tmp_path, monkeypatch):
    """Two courses, 8 envs each, with `--gait`: every row has the old keys, then "path" and "course" (the follower drives, so they lead),
    then "gait"; `ideal` is None; the settings carry the follower's."""
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    courses = ["0.1,0 | 0.1,0.1 | 0,0.1", "-0.05,0.05"]
    # (a course that begins with a minus sign goes in with `=`: argparse reads a bare one as a flag)
    argv = ["--checkpoint", ckpt, "--waypoints", courses[0], "--waypoints=" + courses[1], "--envs_per_command", "8", "--episode_length", "40", "--seed", "3",
            "--gait", "--waypoint_radius", "0.04", "--output", str(tmp_path / "r.json")]
    rep, tr, _ = _run(track, monkeypatch, argv)
    st = rep["settings"]
    assert st["graph"] and st["waypoints"] == courses and st["courses"] == 2 and st["num_envs"] == 16 and st["path"] is True and st["gait"] is True
    assert (st["waypoint_radius"], st["waypoint_speed"], st["waypoint_turn_rate"], st["waypoint_gain"], st["waypoint_slow_dist"]) == (0.04, 0.1, 0.6, 2.0, 0.1)
    assert tuple(rep) == track.REPORT_KEYS and len(rep["commands"]) == 2
    for row, text in zip(rep["commands"], courses):
        pts = track.parse_waypoints(text)
        assert tuple(row) == track.ROW_KEYS + ("path", "course", "gait") and row["command"] == [0.0] * 7 and row["envs"] == 8
        assert tuple(row["path"]) == track.PATH_KEYS and row["path"]["ideal"] is None and row["path"]["error_vs_ideal_m"] is None
        assert tuple(row["course"]) == track.COURSE_KEYS and row["course"]["points"] == pts and len(row["course"]["falls_by_leg"]) == len(pts) + 1
        assert len(row["course"]["waypoints"]) == len(pts) and all(tuple(w) == track.COURSE_POINT_KEYS for w in row["course"]["waypoints"])
        assert 0.0 <= row["course"]["completed_fraction"] <= 1.0 and row["course"]["cross_track_rms_m"] is not None
    assert tuple(tr.course.shape) == (2, G.PATH_COURSE_FLOATS) and tuple(tr.path_acc.shape) == (16, G.PATH_NACC)
    np.testing.assert_array_equal(tr.course_map.cpu().numpy(), np.repeat(np.arange(2), 8))
    np.testing.assert_array_equal(tr.course.cpu().numpy(), track.course_table([track.parse_waypoints(c) for c in courses]))
    # a speed beyond the env's command range is refused once the env exists, naming the range
    with pytest.raises(SystemExit, match="--waypoint_speed 0.5 is beyond the env's command range for vx"):
        track.run(track.build_parser().parse_args(argv + ["--waypoint_speed", "0.5"]))


def test_no_flag_means_no_launch_and_the_old_report(tmp_path, monkeypatch):
    """A run with neither flag calls none of the three Batch methods, has exactly the old keys, and its accumulator has the bits of the same
    run with the Tracker built by hand without the reports."""
    import torch
    from open_duck_playground_amd import engine, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    E, T, seed = 8, 40, 5
    calls = []
    for name in ("path_begin", "path_accumulate", "waypoint_command_apply"):
        real = getattr(engine.Batch, name)
        monkeypatch.setattr(engine.Batch, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    argv = ["--checkpoint", ckpt, "--command", "0.1", "0", "0", "--envs_per_command", str(E), "--episode_length", str(T), "--seed", str(seed),
            "--output", str(tmp_path / "r.json")]
    rep, tr, _ = _run(track, monkeypatch, argv)
    assert calls == [] and tr.path_acc is None and tr.course is None and tr.course_map is None and tr.reports == []
    assert tuple(rep) == track.REPORT_KEYS and all(tuple(r) == track.ROW_KEYS for r in rep["commands"])
    assert not [k for k in rep["settings"] if k == "path" or k == "courses" or k.startswith("waypoint")]
    args = track.build_parser().parse_args(argv)
    env = track.make_env(args, E, 0)
    net = track.load_networks(ckpt, env, torch.device("cuda", 0))
    env.set_commands(torch.from_numpy(track.command_blocks([track.command_row([0.1, 0, 0])], E)).cuda())
    hand = track.Tracker(env, net)
    with torch.no_grad():
        hand.reset(seed)
        for _ in range(T):
            hand.step()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hand.acc.cpu().numpy().view(np.int32), tr.acc.cpu().numpy().view(np.int32))
    assert rep["commands"] == track.reduce_tracking(hand.acc.cpu().numpy(), [track.command_row([0.1, 0, 0])], E)
    # with --path the step gains one launch and the reset one: the first step runs eagerly, the second is captured, the rest are replays
    _run(track, monkeypatch, argv + ["--path"])
    assert calls == ["path_begin", "path_accumulate", "path_accumulate"]
    env.set_commands(None)
    env.batch.close()


def test_refusals_launch_nothing():
    """Each refusal of the three C entries by its message, and the `Batch` methods' own: the accumulator and the command buffer keep their bits."""
    import torch
    from open_duck_playground_amd import engine
    n = 16
    L = engine.load_library()
    env = _duck(n)
    b = env.batch
    env.reset(1)
    b.step(torch.zeros(n, 14, device="cuda"))
    acc = torch.full((n, G.PATH_NACC), 3.0, device="cuda")
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    tab = torch.zeros(2, G.PATH_COURSE_FLOATS, device="cuda")
    tab[:, 0], tab[:, 1] = 1.0, 0.5
    cmap = torch.zeros(n, dtype=torch.int32, device="cuda")
    cmd = torch.full((n, 7), 9.0, device="cuda")
    good = dict(done_dev=b.done.data_ptr(), truncation_dev=b.truncation.data_ptr(), track_acc_dev=tacc.data_ptr(), course_dev=tab.data_ptr(),
                course_of_env_dev=cmap.data_ptr(), acc_dev=acc.data_ptr(), path_acc_dev=acc.data_ptr())

    def ptrs(null):
        return {k: (None if k == null else C.c_void_p(v)) for k, v in good.items()}

    def begin(batch, null=None):
        rc = L.odk_path_begin(batch, ptrs(null)["acc_dev"], b._stream())
        return rc, L.odk_last_error().decode()

    def accumulate(batch, null=None, ncourse=2, radius=0.05, course=True):
        a = ptrs(null)
        rc = L.odk_path_accumulate(batch, a["done_dev"], a["truncation_dev"], a["track_acc_dev"], a["course_dev"] if course else None, ncourse,
                                   a["course_of_env_dev"] if course else None, C.c_float(radius), a["acc_dev"], b._stream())
        return rc, L.odk_last_error().decode()

    def apply(batch, null=None, ncourse=2, v=0.1, rate=0.6, gain=2.0, slow=0.1):
        a = ptrs(null)
        rc = L.odk_waypoint_command_apply(batch, a["course_dev"], ncourse, a["course_of_env_dev"], a["track_acc_dev"], a["path_acc_dev"], C.c_float(v),
                                          C.c_float(rate), C.c_float(gain), C.c_float(slow), b._stream())
        return rc, L.odk_last_error().decode()

    # no commands bound: the follower needs them, the accumulator does not
    assert b.commands is None
    rc, msg = apply(b._b)
    assert rc == G.ERR_INVALID and "odk_waypoint_command_apply: no commands bound (odk_batch_bind_commands)" in msg, msg
    with pytest.raises(engine.OdkError, match="waypoint_command_apply: no commands bound"):
        b.waypoint_command_apply(tab, cmap, tacc, acc, 0.1, 0.6, 2.0, 0.1)
    b.bind_commands(cmd)
    # each null pointer, by name
    for fn, call, names in (("odk_path_begin", begin, ("acc_dev",)),
                            ("odk_path_accumulate", accumulate, ("done_dev", "truncation_dev", "track_acc_dev", "course_of_env_dev", "acc_dev")),
                            ("odk_waypoint_command_apply", apply, ("course_dev", "course_of_env_dev", "track_acc_dev", "path_acc_dev"))):
        for null in names:
            rc, msg = call(b._b, null=null)
            assert rc == G.ERR_INVALID and f"{fn}: null {null}" in msg, (fn, null, msg)
        rc, msg = call(None)
        assert rc == G.ERR_INVALID and f"{fn}: null batch" in msg, msg
    # ncourse outside its range: with a course at least one, without one exactly 0
    for bad in (0, -2):
        rc, msg = accumulate(b._b, ncourse=bad)
        assert rc == G.ERR_INVALID and "odk_path_accumulate: ncourse" in msg, (bad, msg)
        rc, msg = apply(b._b, ncourse=bad)
        assert rc == G.ERR_INVALID and "odk_waypoint_command_apply: ncourse" in msg, (bad, msg)
    rc, msg = accumulate(b._b, ncourse=2, course=False)
    assert rc == G.ERR_INVALID and "null course_dev with ncourse = 2" in msg, msg
    # a parameter that is negative or not finite; a gain or a slow-down distance of 0
    for bad in (-0.1, float("nan"), float("inf")):
        rc, msg = accumulate(b._b, radius=bad)
        assert rc == G.ERR_INVALID and "odk_path_accumulate: radius" in msg, (bad, msg)
        with pytest.raises(engine.OdkError, match="path_accumulate: radius"):
            b.path_accumulate(acc, tacc, tab, cmap, bad)
        for key, name in (("v", "v_cruise"), ("rate", "turn_rate"), ("gain", "heading_gain"), ("slow", "slow_dist")):
            rc, msg = apply(b._b, **{key: bad})
            assert rc == G.ERR_INVALID and f"odk_waypoint_command_apply: {name}" in msg, (name, bad, msg)
        with pytest.raises(engine.OdkError, match="waypoint_command_apply: turn_rate"):
            b.waypoint_command_apply(tab, cmap, tacc, acc, 0.1, bad, 2.0, 0.1)
    for key, name in (("gain", "heading_gain"), ("slow", "slow_dist")):
        rc, msg = apply(b._b, **{key: 0.0})
        assert rc == G.ERR_INVALID and name in msg, (name, msg)
    with pytest.raises(engine.OdkError, match="waypoint_command_apply: slow_dist"):
        b.waypoint_command_apply(tab, cmap, tacc, acc, 0.1, 0.6, 2.0, 0.0)
    # a course count outside its range never reaches the device: the builder refuses it
    from open_duck_playground_amd import track
    for pts in ([], [[0.1 * k, 0.0] for k in range(9)]):
        with pytest.raises(ValueError, match="a course has 1 to 8 points"):
            track.course_table([pts])
    # wrong-shaped and CPU tensors are OdkErrors before anything is launched
    for bad in (acc[:, :-1].contiguous(), acc.cpu(), acc.double(), acc[:-1]):
        with pytest.raises(engine.OdkError, match="path_begin: acc"):
            b.path_begin(bad)
        with pytest.raises(engine.OdkError, match="path_accumulate: acc"):
            b.path_accumulate(bad, tacc)
        with pytest.raises(engine.OdkError, match="waypoint_command_apply: path_acc"):
            b.waypoint_command_apply(tab, cmap, tacc, bad, 0.1, 0.6, 2.0, 0.1)
    for args in ((tab[:, :-1].contiguous(), cmap), (tab.cpu(), cmap), (tab, cmap.long()), (tab, cmap[:-1]), (tab, cmap.cpu()), (tab, None)):
        with pytest.raises(engine.OdkError, match="path_accumulate: course"):
            b.path_accumulate(acc, tacc, *args, 0.05)
        with pytest.raises(engine.OdkError, match="waypoint_command_apply: course"):
            b.waypoint_command_apply(*args, tacc, acc, 0.1, 0.6, 2.0, 0.1)
    with pytest.raises(engine.OdkError, match="path_accumulate: course_of_env without a course"):
        b.path_accumulate(acc, tacc, None, cmap)
    with pytest.raises(engine.OdkError, match="track_acc"):
        b.path_accumulate(acc, tacc.cpu())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.cpu().numpy(), 3.0)
    np.testing.assert_array_equal(cmd.cpu().numpy(), 9.0)
    # ... and the good calls count
    b.path_begin(acc)
    b.path_accumulate(acc, tacc, tab, cmap, 0.05)
    b.waypoint_command_apply(tab, cmap, tacc, acc, 0.1, 0.6, 2.0, 0.1)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert np.all(got[:, G.PATH_SAMPLES] == 1.0) and np.all(got[:, G.PATH_XTRACK_SAMPLES] == 1.0) and np.all(got[:, G.PATH_REACHED + 1:] == 0.0)
    np.testing.assert_array_equal(cmd.cpu().numpy()[:, 3:], 9.0)
    np.testing.assert_array_equal(cmd.cpu().numpy()[:, :3], np.tile(f32([0.1, 0, 0]), (n, 1)))      # clock 0: the point (0.5, 0) is dead ahead
    b.bind_commands(None)
    b.close()
