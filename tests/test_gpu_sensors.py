"""GPU checks of the sensor-fault stage (`odk_sensor_apply`, `Batch.sensor_apply`, `Tracker(sensors=...)`, `track --sensor` / `--sensor_grid`).
The kernel is driven with synthetic observation tensors -- no physics -- and held bit for bit against the numpy restatement
(`sensors.sensor_apply_reference`, itself checked in tests/test_sensors_host.py): there is no tolerance on a device result in this file."""
import functools
import json
import os

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

# robot, nu, Standing?, nobs
CASES = {"duck": ("flat_terrain", 14, False, 101), "duck_standing": ("flat_terrain", 14, True, 85),
         "biped_arms": ("biped_arms.xml", 16, False, 113), "tail_biped": ("tail_biped.xml", 15, False, 107)}
NENVS = (5, 67)      # 5: a quarter of a wave and a bit; 67: four full 256-thread blocks of 16 envs and one with 3, its wave three rows full
T_CALLS = 12
FAULTS = ("nominal", "rotation", "gyro", "acc", "imu_delay", "joint_delay", "both_delays", "enc_offset", "enc_quant", "contacts", "all")
DELAYS = (0.0, 1.0, 7.0, 9.0, 3.0)      # 9 is above the ring and clamped to 7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _batch(case, n):
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    robot, nu, standing, nobs = CASES[case]
    cfg = engine.default_config(standing)
    if robot.endswith(".xml"):
        model = Model.from_xml(os.path.join(RC.ASSETS, robot))
        cfg.use_imitation = 0
    else:
        model = load_task_model(robot)
    b = engine.Batch(model, n, cfg)
    assert (b.model.nu, b.nobs) == (nu, nobs)
    return b


def touched_columns(nu, standing):
    c = 13 + (5 if standing else 6) * nu
    return np.r_[0:6, 13:13 + 2 * nu, c:c + 2]


@functools.lru_cache(maxsize=None)
def inputs(case, n):
    """[T, n, nobs] observations and [T, n] done flags, seeded.  Every touched column holds ordinary numbers with exact zeros and -0.0
    sprinkled in; the untouched columns also hold NaN (one with a payload) and +-inf.  done: sprinkled, and for env 1 at call 0 and on the
    consecutive calls 4 and 5."""
    _, nu, standing, nobs = CASES[case]
    rng = np.random.default_rng(1000 * nu + n + standing)
    X = rng.standard_normal((T_CALLS, n, nobs)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.float32(0.0)
    X[rng.random(X.shape) < 0.05] = np.float32(-0.0)
    rest = np.setdiff1d(np.arange(nobs), touched_columns(nu, standing))
    odd = np.concatenate([np.float32([np.nan, np.inf, -np.inf]), np.frombuffer(np.uint32(0xFFC12345).tobytes(), np.float32)])
    plant = rng.random((T_CALLS, n, rest.size)) < 0.1
    sub = X[:, :, rest]
    sub[plant] = odd[rng.integers(0, 4, int(plant.sum()))]
    X[:, :, rest] = sub
    done = (rng.random((T_CALLS, n)) < 0.15).astype(np.float32)
    done[:, 1] = 0.0
    done[[0, 4, 5], 1] = 1.0
    return X, done


def fault_rows(kind, case, n):
    from open_duck_playground_amd import engine
    rng = np.random.default_rng(len(kind) + n)
    f = engine.sensor_fault_rows(n)
    every = kind == "all"
    if kind == "rotation" or every:
        for e in range(n):
            f[e, :9] = engine.sensor_rotation(*rng.uniform(-20, 20, 3)).reshape(9)
        if n > 2:
            f[2, :9] = np.eye(3, dtype=np.float32).reshape(9)      # per-env selects: one row keeps the identity
    if kind == "gyro" or every:
        f[:, engine.SENSOR_GYRO_SCALE] = rng.uniform(0.8, 1.2, n)
        f[:, engine.SENSOR_GYRO_BIAS:engine.SENSOR_GYRO_BIAS + 3] = rng.uniform(-0.3, 0.3, (n, 3))
        f[0, engine.SENSOR_GYRO_BIAS + 1] = 0.0                    # one nominal stage among the others
        f[n - 1, engine.SENSOR_GYRO_SCALE] = 1.0
    if kind == "acc" or every:
        f[:, engine.SENSOR_ACC_SCALE] = rng.uniform(0.8, 1.2, n)
        f[:, engine.SENSOR_ACC_BIAS:engine.SENSOR_ACC_BIAS + 3] = rng.uniform(-1.5, 1.5, (n, 3))
        f[0, engine.SENSOR_ACC_BIAS] = 1.3                         # the reference's deployment bias
    if kind in ("imu_delay", "both_delays") or every:
        f[:, engine.SENSOR_IMU_DELAY] = [DELAYS[e % 5] for e in range(n)]
    if kind in ("joint_delay", "both_delays") or every:
        f[:, engine.SENSOR_JOINT_DELAY] = [DELAYS[(e + 2) % 5] for e in range(n)]
    if kind == "enc_offset" or every:
        off = rng.uniform(-0.05, 0.05, (n, 16)).astype(np.float32)
        off[rng.random((n, 16)) < 0.2] *= 0                        # some actuators exact (-0.0 among them: nominal too)
        f[:, engine.SENSOR_ENC_OFFSET:] = off
    if kind == "enc_quant" or every:
        f[:, engine.SENSOR_ENC_QUANT] = [(0.01, 2 * np.pi / 4096, 0.0, 0.125)[e % 4] for e in range(n)]
    if kind == "contacts" or every:
        f[:, engine.SENSOR_CONTACT_MODE] = [e % 3 for e in range(n)]
        f[:, engine.SENSOR_CONTACT_MODE + 1] = [(e // 3) % 3 for e in range(n)]
    return f


@functools.lru_cache(maxsize=None)
def device_run(case, n, kind):
    """T_CALLS launches over `inputs` under `fault_rows`: (outputs [T, n, nobs], final state [n, NSTATE], the restatement's two)."""
    import torch
    from open_duck_playground_amd import engine, sensors
    _, nu, standing, nobs = CASES[case]
    b = _batch(case, n)
    X, done = inputs(case, n)
    f = fault_rows(kind, case, n)
    fault = torch.from_numpy(f).cuda()
    out_guard = torch.full((n + 3, nobs), 7.0, device="cuda")          # rows past the batch: the last wave's idle rows must not touch them
    state_guard = torch.full((n + 3, engine.SENSOR_NSTATE), 7.0, device="cuda")
    out, state = out_guard[:n], state_guard[:n]
    state.zero_()
    want_state = np.zeros((n, engine.SENSOR_NSTATE), np.float32)
    got, want = [], []
    for t in range(T_CALLS):
        obs = torch.from_numpy(X[t]).cuda()
        b.sensor_apply(obs, torch.from_numpy(done[t]).cuda(), fault, state, out)
        got.append(out.cpu().numpy())
        assert np.array_equal(bits(obs.cpu().numpy()), bits(X[t])), "the input row is only read"
        want.append(sensors.sensor_apply_reference(X[t], done[t], f, want_state, nu, joystick=not standing))
    assert (out_guard[n:] == 7.0).all() and (state_guard[n:] == 7.0).all()
    assert np.array_equal(bits(fault.cpu().numpy()), bits(f))
    return np.stack(got), state.cpu().numpy(), np.stack(want), want_state


@pytest.mark.parametrize("kind", FAULTS)
@pytest.mark.parametrize("n", NENVS)
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_has_the_restatements_bits(case, n, kind):
    _, nu, standing, nobs = CASES[case]
    got, state, want, want_state = device_run(case, n, kind)
    X, done = inputs(case, n)
    rest = np.setdiff1d(np.arange(nobs), touched_columns(nu, standing))
    for t in range(T_CALLS):
        assert np.array_equal(bits(got[t][:, rest]), bits(X[t][:, rest])), f"call {t}: an untouched column changed"
        bad = np.argwhere(bits(got[t]) != bits(want[t]))
        assert bad.size == 0, f"call {t}: (env, column) {bad[:5].tolist()} got {got[t][tuple(bad[0])]!r} want {want[t][tuple(bad[0])]!r}"
    assert np.array_equal(bits(state), bits(want_state)), "the state row after the run"
    if kind != "nominal":      # the fault is one: the run differs from its input somewhere in the touched columns
        assert not np.array_equal(bits(got), bits(X))


@pytest.mark.parametrize("n", NENVS)
@pytest.mark.parametrize("case", list(CASES))
def test_all_nominal_hands_back_every_bit(case, n):
    """-0.0, NaN (with a payload) and +-inf planted in touched and untouched columns alike; done sprinkled; done = None too"""
    import torch
    from open_duck_playground_amd import engine
    _, nu, standing, nobs = CASES[case]
    b = _batch(case, n)
    X, done = inputs(case, n)
    X = X.copy()
    rng = np.random.default_rng(n)
    odd = np.concatenate([np.float32([np.nan, np.inf, -np.inf, -0.0]), np.frombuffer(np.uint32(0xFFC12345).tobytes(), np.float32)])
    plant = rng.random(X.shape) < 0.2
    X[plant] = odd[rng.integers(0, 5, int(plant.sum()))]
    fault = torch.from_numpy(engine.sensor_fault_rows(n)).cuda()
    for with_done in (True, False):
        state = torch.zeros(n, engine.SENSOR_NSTATE, device="cuda")
        out = torch.full((n, nobs), 7.0, device="cuda")
        for t in range(T_CALLS):
            b.sensor_apply(torch.from_numpy(X[t]).cuda(), torch.from_numpy(done[t]).cuda() if with_done else None, fault, state, out)
            assert np.array_equal(bits(out.cpu().numpy()), bits(X[t])), (with_done, t)


def test_the_binding_refuses_by_name():
    import torch
    from open_duck_playground_amd import engine
    b = _batch("duck", 5)
    obs, out = torch.zeros(5, 101, device="cuda"), torch.full((5, 101), 3.0, device="cuda")
    fault, state = torch.from_numpy(engine.sensor_fault_rows(5)).cuda(), torch.zeros(5, engine.SENSOR_NSTATE, device="cuda")
    for args, message in (((obs, None, fault, state, obs), "out shares memory with obs"),
                          ((obs, None, fault, state, obs[:]), "out shares memory with obs"),
                          ((obs, None, fault, state, out[:, :100]), "sensor_apply: out: shape"),
                          ((obs, None, fault[:, :40], state, out), "sensor_apply: fault: shape"),
                          ((obs, None, fault, state[:4], out), "sensor_apply: state: shape"),
                          ((obs.double(), None, fault, state, out), "sensor_apply: obs: dtype"),
                          ((obs.cpu(), None, fault, state, out), "sensor_apply: obs: the tensor must live on cuda"),
                          ((obs, torch.zeros(4, device="cuda"), fault, state, out), "sensor_apply: done"),
                          ((obs, None, fault.t().contiguous().t(), state, out), "sensor_apply: fault: the tensor must be contiguous")):
        with pytest.raises(engine.OdkError, match=message):
            b.sensor_apply(*args)
    # the C entry point's own refusals: an overlapping output and a null pointer, nothing launched
    import ctypes as C
    L = engine.load_library()
    P = lambda t: C.c_void_p(t.data_ptr())
    both = torch.zeros(2 * 5 * 101 - 1, device="cuda")
    rc = L.odk_sensor_apply(b._b, P(both), None, P(fault), P(state), C.c_void_p(both.data_ptr() + 4 * (5 * 101 - 1)), None)
    assert rc != 0 and "odk_sensor_apply: obs_out_dev overlaps obs_dev" in L.odk_last_error().decode()
    rc = L.odk_sensor_apply(b._b, P(obs), None, None, P(state), P(out), None)
    assert rc != 0 and "odk_sensor_apply: null fault_dev" in L.odk_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 3.0).all() and not state.any()


# ---- the Tracker and `track`
E_T, T_T = 16, 20


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """One duck env of 2 * E_T envs under two commands and a randomly initialised policy, shared by the Tracker tests; each builds its
    Trackers one after the other and never steps an older one again."""
    import torch
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path_factory.mktemp("sensors"))
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--command", "0", "0", "0", "--seed", "1"])
    env = track.make_env(args, 2 * E_T, 0)
    net = track.load_networks(ckpt, env, torch.device("cuda", 0))
    cmds = [track.command_row([0, 0, 0]), track.command_row([0.15, 0, 0])]
    env.set_commands(torch.from_numpy(track.command_blocks(cmds, E_T)).cuda())
    yield track, env, net
    env.set_commands(None)
    env.batch.close()


def _accumulate(track, env, net, steps, use_graph=True, fault=None, between=None):
    """The tracking accumulator after `steps` steps of a fresh Tracker; `between(tr, t)` runs before step t."""
    import torch
    tr = track.Tracker(env, net, use_graph=use_graph, **({} if fault is None else dict(sensors=dict(fault=fault))))
    with torch.no_grad():
        tr.reset(1)
        for t in range(steps):
            if between:
                between(tr, t)
            tr.step()
        acc = tr.acc.cpu().numpy()
    assert (tr.graph is not None) == use_graph
    return acc, tr


def _biased(n):
    from open_duck_playground_amd import engine
    f = engine.sensor_fault_rows(n)
    f[:, engine.SENSOR_GYRO_BIAS + 1] = 0.2
    return f


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
def test_tracker_with_nominal_sensors_is_the_tracker_without(rig, use_graph):
    import torch
    from open_duck_playground_amd import engine
    track, env, net = rig
    n = env.num_envs
    plain, tr0 = _accumulate(track, env, net, T_T, use_graph)
    assert tr0.sensor_fault is None and tr0.sensor_state is None and tr0.sensor_obs is None
    nominal, tr1 = _accumulate(track, env, net, T_T, use_graph, torch.from_numpy(engine.sensor_fault_rows(n)).cuda())
    assert np.array_equal(bits(nominal), bits(plain)) and plain[:, track.STEPS].min() >= 1
    head =tr1.sensor_state[:, engine.SENSOR_HEAD].cpu().numpy()
    assert head.min() >= 1 and head.max() <= T_T      # the ring ran: a count since the last refill
    biased, _ = _accumulate(track, env, net, T_T, use_graph, torch.from_numpy(_biased(n)).cuda())
    assert not np.array_equal(bits(biased), bits(plain)), "a gyro bias of 0.2 rad/s changes what the policy does"


def test_the_captured_graph_follows_the_fault_tensor(rig):
    import torch
    from open_duck_playground_amd import engine
    track, env, net = rig
    n = env.num_envs
    nominal, biased = engine.sensor_fault_rows(n), _biased(n)
    fault = torch.from_numpy(nominal).cuda()

    def rewrite(tr, t):
        if t == 8:
            assert tr.graph is not None and tr.sensor_fault.data_ptr() == fault.data_ptr()      # the caller's own memory, read by the replays
            fault.copy_(torch.from_numpy(biased))
    mid, tr = _accumulate(track, env, net, T_T, True, fault, rewrite)
    # the same Tracker, its graph as captured, from a new reset with the rewritten tensor: a fresh Tracker built with that tensor
    with torch.no_grad():
        tr.reset(1)
        for _ in range(T_T):
            tr.step()
        again = tr.acc.cpu().numpy()
    fresh, _ = _accumulate(track, env, net, T_T, True, torch.from_numpy(biased).cuda())
    assert np.array_equal(bits(again), bits(fresh))
    # rewritten mid-run: what an eager Tracker, which reads the tensor at every launch, does with the same rewrite
    fault2 = torch.from_numpy(nominal).cuda()
    eager, _ = _accumulate(track, env, net, T_T, False, fault2, lambda tr, t: fault2.copy_(torch.from_numpy(biased)) if t == 8 else None)
    assert np.array_equal(bits(mid), bits(eager))
    plain, _ = _accumulate(track, env, net, T_T, True, torch.from_numpy(nominal).cuda())
    assert not np.array_equal(bits(mid), bits(plain)) and not np.array_equal(bits(mid), bits(fresh))


def test_track_sensor_sweep_end_to_end(tmp_path):
    from open_duck_playground_amd import sensors, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    base = ["--checkpoint", ckpt, "--envs_per_command", "2", "--episode_length", "8", "--seed", "1", "--falls"]
    out = tmp_path / "report.json"
    args = track.build_parser().parse_args(base + ["--command", "0.1", "0", "0", "--sensor_grid", "imu_delay=0:2:3", "--sensor", "gyro_bias_y=0.2",
                                                   "--output", str(out)])
    rep = track.run(args)
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep))
    s = back["settings"]
    assert s["graph"] and s["num_envs"] == 8 and s["sensors_per_command"] == 4 and s["sensor"] == ["gyro_bias_y=0.2"]
    assert s["sensor_grid"] == "imu_delay=0:2:3" and s["robust_fall_rate"] == 0.05 and "privileged row" in s["sensor_semantics"]
    assert tuple(back) == track.REPORT_KEYS and len(back["commands"]) == 1
    row = back["commands"][0]
    assert tuple(row) == track.ROW_KEYS + ("sensors", "falls", "sensor_robustness") and row["envs"] == 8
    cells = row["sensors"]
    assert [(c["sensor"]["gyro_bias_y"], c["sensor"]["imu_delay"]) for c in cells] == [(0.2, 0), (0.0, 0), (0.0, 1), (0.0, 2)]      # --sensor first, then the grid
    for c in cells:
        assert tuple(c) == track.ROW_KEYS + ("sensor", "falls") and c["envs"] == 2 and c["command"] == row["command"]
        assert tuple(c["sensor"]) == sensors.SENSOR_KEYS and isinstance(c["falls"], dict) and c["falls"]
    assert cells[1]["sensor"] == sensors.nominal_sensor()
    rb = row["sensor_robustness"]
    assert set(rb) == {"robust_fall_rate", "gyro_bias_y", "imu_delay", "survived_range"} and set(rb["survived_range"]) == {"gyro_bias_y", "imu_delay"}
    assert [p["value"] for p in rb["imu_delay"]] == [0, 1, 2] and [p["value"] for p in rb["gyro_bias_y"]] == [0.0, 0.2]
    assert all(tuple(p) == track.ROBUSTNESS_POINT_KEYS for p in rb["imu_delay"] + rb["gyro_bias_y"])
    for p, c in zip(rb["imu_delay"], cells[1:]):
        assert all(p[k] == c[k] for k in track.ROBUSTNESS_POINT_KEYS[1:])
    # no sensor flags, the same eight envs as four rows of two: row 1 holds the envs of the nominal cell, and is that cell figure for figure
    args = track.build_parser().parse_args(base + ["--command", "0.1", "0", "0"] * 4 + ["--output", str(tmp_path / "plain.json")])
    plain = track.run(args)
    assert not any(k.startswith("sensor") for k in plain["settings"]) and all(tuple(r) == track.ROW_KEYS + ("falls",) for r in plain["commands"])
    assert {k: v for k, v in cells[1].items() if k != "sensor"} == plain["commands"][1]
    figures = lambda r: [r[k] for k in track.ROW_KEYS[1:]]
    assert figures(cells[0]) != figures(plain["commands"][0]), "the biased cell is not the plain run"
    assert {k: v for k, v in s.items() if not k.startswith("sensor") and k not in ("robust_fall_rate", "num_envs")} == \
        {k: v for k, v in plain["settings"].items() if k != "num_envs"}
