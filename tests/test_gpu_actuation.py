"""GPU checks of the actuation-fault stage (`odk_action_apply`, `Batch.action_apply`, `Tracker(actuation=...)`, `track --actuation` /
`--actuation_grid`).  The kernel is driven with synthetic action tensors -- no physics -- and held bit for bit against the numpy restatement
(`actuation.action_apply_reference`, itself checked in tests/test_actuation_host.py): there is no tolerance on a device result in this file."""
import functools
import json
import os

import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

# robot, nu, Standing?
CASES = {"duck": ("flat_terrain", 14, False), "duck_standing": ("flat_terrain", 14, True), "biped12": ("biped12.xml", 12, False),
         "tail_biped": ("tail_biped.xml", 15, False), "biped_arms": ("biped_arms.xml", 16, False)}
NENVS = (5, 67)      # 5: a quarter of a wave and a bit; 67: four full 256-thread blocks of 16 envs and one with 3, its wave three rows full
T_CALLS = 24
FAULTS = ("nominal", "gain", "offset", "noise", "limit", "filter", "quant", "drop1", "drop3", "freeze", "all", "out_of_range")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _batch(case, n):
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    robot, nu, standing = CASES[case]
    cfg = engine.default_config(standing)
    if robot.endswith(".xml"):
        model = Model.from_xml(os.path.join(RC.ASSETS, robot))
        cfg.use_imitation = 0
    else:
        model = load_task_model(robot)
    b = engine.Batch(model, n, cfg)
    assert b.model.nu == nu
    return b


ODD = np.concatenate([np.float32([np.nan, np.inf, -np.inf]), np.frombuffer(np.uint32(0xFFC12345).tobytes(), np.float32)])


@functools.lru_cache(maxsize=None)
def inputs(case, n):
    """[T, n, nu] actions and [T, n] done flags, seeded: ordinary numbers with exact zeros and -0.0 sprinkled in.  done: sprinkled, and for
    env 1 at call 0 and on the consecutive calls 4 and 5."""
    _, nu, standing = CASES[case]
    rng = np.random.default_rng(1000 * nu + n + standing)
    X = np.tanh(rng.standard_normal((T_CALLS, n, nu))).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.float32(0.0)
    X[rng.random(X.shape) < 0.05] = np.float32(-0.0)
    done = (rng.random((T_CALLS, n)) < 0.15).astype(np.float32)
    done[:, 1] = 0.0
    done[[0, 4, 5], 1] = 1.0
    return X, done


def fault_rows(kind, n):
    from open_duck_playground_amd import actuation, engine
    E = engine
    rng = np.random.default_rng(len(kind) + n)
    f = engine.action_fault_rows(n)
    f[:, E.ACT_SEED] = actuation.env_seeds(n, n)
    every = kind in ("all", "out_of_range")
    if kind == "gain" or every:
        f[:, E.ACT_GAIN] = rng.uniform(0.7, 1.3, n)
        f[0, E.ACT_GAIN] = 1.0                                     # one nominal stage among the others
    if kind == "offset" or every:
        off = rng.uniform(-0.2, 0.2, (n, 16)).astype(np.float32)
        off[rng.random((n, 16)) < 0.2] *= 0                        # some actuators exact (-0.0 among them: nominal too)
        f[:, E.ACT_OFFSET:E.ACT_OFFSET + 16] = off
    if kind == "noise" or every:
        f[:, E.ACT_NOISE] = [(0.02, 0.0, 0.1, 1.0)[e % 4] for e in range(n)]
    if kind == "limit" or every:
        f[:, E.ACT_LIMIT] = [(0.5, 0.9, 0.0, 0.05)[(e + 1) % 4] for e in range(n)]
    if kind == "filter" or every:
        f[:, E.ACT_ALPHA] = [(actuation.filter_alpha(37.5, 0.02), actuation.filter_alpha(5.0, 0.02), 0.0, 0.5, 0.999)[(e + 2) % 5] for e in range(n)]
    if kind == "quant" or every:
        f[:, E.ACT_QUANT] = [(2 * np.pi / 4096 / 0.25, 0.01, 0.125, 0.0)[e % 4] for e in range(n)]
    if kind in ("drop1", "drop3") or every:
        f[:, E.ACT_DROP_P] = [(0.3, 0.05, 1.0, 0.0, 0.6)[e % 5] for e in range(n)]
        f[:, E.ACT_DROP_LEN] = 1.0 if kind == "drop1" else ([(3.0, 1.0, 2.0)[e % 3] for e in range(n)] if every else 3.0)
    if kind == "freeze" or every:
        for e in range(n):
            f[e, E.ACT_FREEZE_AT + (e % 12)] = 0.0                 # two actuators per env: one off the bus from the start, one from step 6
            f[e, E.ACT_FREEZE_AT + ((e + 5) % 12)] = 6.0
    if kind == "all" and n > 2:
        f[2] = engine.action_fault_rows(1)[0]                      # per-env selects: one row wholly nominal
    if kind == "out_of_range":
        for s in range(E.ACT_NPRM):                                # NaN in each slot: slot s in env s mod n, on rows with every stage on
            f[s % n, s] = np.nan
        for e in range(n):
            if e % 4 == 0 and not np.isnan(f[e, E.ACT_QUANT]):
                f[e, E.ACT_QUANT] = -0.01
            if e % 4 == 1 and not np.isnan(f[e, E.ACT_LIMIT]):
                f[e, E.ACT_LIMIT] = -0.5
            if e % 4 == 2 and not np.isnan(f[e, E.ACT_DROP_LEN]):
                f[e, E.ACT_DROP_LEN] = 0.0
            if e % 4 == 3 and not np.isnan(f[e, E.ACT_SEED]):
                f[e, E.ACT_SEED] = (2.0 ** 24 + 1000.0, -5.0, 3.5e9, 7.75)[(e // 4) % 4]
    return f


def all_nominal(f):
    from open_duck_playground_amd import engine
    g = f.copy()
    g[:, engine.ACT_SEED] = 0.0      # (a seed is no stage)
    return (bits(g) == bits(engine.action_fault_rows(1))).all(axis=1)


@functools.lru_cache(maxsize=None)
def device_run(case, n, kind):
    """T_CALLS launches over `inputs` under `fault_rows`: (inputs as run [T, n, nu], outputs [T, n, nu], final state [n, NSTATE], the
    restatement's two).  The envs whose row is all-nominal get NaN (one with a payload) and +-inf planted in their actions; no other env
    does, so no NaN arithmetic is compared by bits."""
    import torch
    from open_duck_playground_amd import actuation, engine
    _, nu, standing = CASES[case]
    b = _batch(case, n)
    X, done = inputs(case, n)
    f = fault_rows(kind, n)
    X = X.copy()
    rng = np.random.default_rng(n + nu)
    for e in np.flatnonzero(all_nominal(f)):
        plant = rng.random((T_CALLS, nu)) < 0.2
        X[:, e][plant] = ODD[rng.integers(0, 4, int(plant.sum()))]
    fault = torch.from_numpy(f).cuda()
    out_guard = torch.full((n + 3, nu), 7.0, device="cuda")          # rows past the batch: the last wave's idle rows must not touch them
    state_guard = torch.full((n + 3, engine.ACT_NSTATE), 7.0, device="cuda")
    out, state = out_guard[:n], state_guard[:n]
    state.zero_()
    want_state = np.zeros((n, engine.ACT_NSTATE), np.float32)
    got, want = [], []
    for t in range(T_CALLS):
        act = torch.from_numpy(X[t]).cuda()
        b.action_apply(act, torch.from_numpy(done[t]).cuda(), fault, state, out)
        got.append(out.cpu().numpy())
        assert np.array_equal(bits(act.cpu().numpy()), bits(X[t])), "the input row is only read"
        want.append(actuation.action_apply_reference(X[t], done[t], f, want_state, nu))
    assert (out_guard[n:] == 7.0).all() and (state_guard[n:] == 7.0).all()
    assert np.array_equal(bits(fault.cpu().numpy()), bits(f))
    return X, np.stack(got), state.cpu().numpy(), np.stack(want), want_state


@pytest.mark.parametrize("kind", FAULTS)
@pytest.mark.parametrize("n", NENVS)
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_has_the_restatements_bits(case, n, kind):
    X, got, state, want, want_state = device_run(case, n, kind)
    for t in range(T_CALLS):
        bad = np.argwhere(bits(got[t]) != bits(want[t]))
        assert bad.size == 0, f"call {t}: (env, actuator) {bad[:5].tolist()} got {got[t][tuple(bad[0])]!r} want {want[t][tuple(bad[0])]!r}"
    bad = np.argwhere(bits(state) != bits(want_state))
    assert bad.size == 0, f"the state row after the run: (env, slot) {bad[:5].tolist()}"
    nominal = all_nominal(fault_rows(kind, n))
    assert np.array_equal(bits(got[:, nominal]), bits(X[:, nominal])), "an all-nominal row hands back every bit"
    if kind != "nominal":      # the fault is one: the run differs from its input
        assert not np.array_equal(bits(got), bits(X))
    else:
        assert nominal.all()


@pytest.mark.parametrize("case", ["duck", "biped_arms"])
def test_all_nominal_hands_back_every_bit_without_done(case):
    """-0.0, NaN (with a payload) and +-inf planted everywhere; done = NULL"""
    import torch
    from open_duck_playground_amd import engine
    n = 67
    _, nu, _ = CASES[case]
    b = _batch(case, n)
    X = inputs(case, n)[0].copy()
    rng = np.random.default_rng(n)
    plant = rng.random(X.shape) < 0.2
    X[plant] = np.concatenate([ODD, np.float32([-0.0])])[rng.integers(0, 5, int(plant.sum()))]
    fault = torch.from_numpy(engine.action_fault_rows(n)).cuda()
    state = torch.zeros(n, engine.ACT_NSTATE, device="cuda")
    out = torch.full((n, nu), 7.0, device="cuda")
    for t in range(T_CALLS):
        b.action_apply(torch.from_numpy(X[t]).cuda(), None, fault, state, out)
        assert np.array_equal(bits(out.cpu().numpy()), bits(X[t])), t
    s = state.cpu().numpy()
    assert (s[:, engine.ACT_HEAD] == T_CALLS).all() and (s[:, engine.ACT_EPISODE] == 1).all() and (s[:, engine.ACT_CALLS] == T_CALLS).all()


def test_the_binding_and_the_entry_refuse_by_name():
    import torch
    from open_duck_playground_amd import engine
    b = _batch("duck", 5)
    act, out = torch.zeros(5, 14, device="cuda"), torch.full((5, 14), 3.0, device="cuda")
    fault, state = torch.from_numpy(engine.action_fault_rows(5)).cuda(), torch.zeros(5, engine.ACT_NSTATE, device="cuda")
    for args, message in (((act, None, fault, state, act), "action_apply: out shares memory with act"),
                          ((act, None, fault, state, act[:]), "action_apply: out shares memory with act"),
                          ((act, None, fault, state, out[:, :13]), "action_apply: out: shape"),
                          ((act[:4], None, fault, state, out), "action_apply: act: shape"),
                          ((act, None, fault[:, :40], state, out), "action_apply: fault: shape"),
                          ((act, None, fault, state[:4], out), "action_apply: state: shape"),
                          ((act.double(), None, fault, state, out), "action_apply: act: dtype"),
                          ((act.cpu(), None, fault, state, out), "action_apply: act: the tensor must live on cuda"),
                          ((act, None, fault.cpu().numpy(), state, out), "action_apply: fault: expected a torch tensor"),
                          ((act, torch.zeros(4, device="cuda"), fault, state, out), "action_apply: done"),
                          ((act, None, fault.t().contiguous().t(), state, out), "action_apply: fault: the tensor must be contiguous")):
        with pytest.raises(engine.OdkError, match=message):
            b.action_apply(*args)
    # the C entry point's own refusals: an overlapping output and every null pointer, nothing launched
    import ctypes as C
    L = engine.load_library()
    P = lambda t: C.c_void_p(t.data_ptr())
    both = torch.zeros(2 * 5 * 14 - 1, device="cuda")
    rc = L.odk_action_apply(b._b, P(both), None, P(fault), P(state), C.c_void_p(both.data_ptr() + 4 * (5 * 14 - 1)), None)
    assert rc != 0 and "odk_action_apply: act_out_dev overlaps act_dev" in L.odk_last_error().decode()
    for k, name in ((0, "batch"), (1, "act_dev"), (3, "fault_dev"), (4, "state_dev"), (5, "act_out_dev")):
        args = [b._b, P(act), None, P(fault), P(state), P(out), None]
        args[k] = None
        assert L.odk_action_apply(*args) != 0 and f"odk_action_apply: null {name}" in L.odk_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 3.0).all() and not state.any()


# ---- the Tracker and `track`
E_T, T_T = 16, 20


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    """One duck env of 2 * E_T = 32 envs under two commands and a randomly initialised policy, shared by the Tracker tests; each builds its
    Trackers one after the other and never steps an older one again."""
    import torch
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path_factory.mktemp("actuation"))
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--command", "0", "0", "0", "--seed", "1"])
    env = track.make_env(args, 2 * E_T, 0)
    net = track.load_networks(ckpt, env, torch.device("cuda", 0))
    cmds = [track.command_row([0, 0, 0]), track.command_row([0.15, 0, 0])]
    env.set_commands(torch.from_numpy(track.command_blocks(cmds, E_T)).cuda())
    yield track, env, net
    env.set_commands(None)
    env.batch.close()


def _run_tracker(track, env, net, steps, use_graph=True, fault=None, each=None):
    """(acc, obs, reward) after `steps` steps of a fresh Tracker, and the Tracker; `each(tr, t)` runs after step t."""
    import torch
    tr = track.Tracker(env, net, use_graph=use_graph, **({} if fault is None else dict(actuation=dict(fault=fault))))
    with torch.no_grad():
        tr.reset(1)
        for t in range(steps):
            tr.step()
            if each:
                each(tr, t)
        res = tuple(x.cpu().numpy().copy() for x in (tr.acc, env.batch.obs, env.batch.reward))
    assert (tr.graph is not None) == use_graph
    return res, tr


def _blocks(env, spec):
    from open_duck_playground_amd import actuation
    names = [str(s) for s in env.batch.model.a["names_actuator"]]
    return actuation.actuation_blocks(2, [actuation.parse_actuation(spec)], E_T, 1, float(env.batch.cfg.action_scale), float(env.dt), names)


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
def test_tracker_with_nominal_actuation_is_the_tracker_without(rig, use_graph):
    import torch
    from open_duck_playground_amd import engine
    track, env, net = rig
    n = env.num_envs
    plain, tr0 = _run_tracker(track, env, net, T_T, use_graph)
    assert tr0.actuation_fault is None and tr0.actuation_state is None and tr0.actuation_act is None
    nominal, tr1 = _run_tracker(track, env, net, T_T, use_graph, torch.from_numpy(engine.action_fault_rows(n)).cuda())
    for name, a, b in zip(("acc", "obs", "reward"), nominal, plain):
        assert np.array_equal(bits(a), bits(b)), name
    assert plain[0][:, track.STEPS].min() >= 1
    s = tr1.actuation_state.cpu().numpy()
    assert (s[:, engine.ACT_CALLS] == T_T).all() and not s[:, engine.ACT_DROPS].any() and s[:, engine.ACT_HEAD].min() >= 1
    filtered, _ = _run_tracker(track, env, net, T_T, use_graph, torch.from_numpy(_blocks(env, "cutoff=5")).cuda())
    assert not np.array_equal(bits(filtered[1]), bits(plain[1])), "a 5 Hz filter on the actions changes what the robot does"


def test_a_captured_tracker_is_the_eager_one(rig):
    import torch
    track, env, net = rig
    f = _blocks(env, "drop=0.3,cutoff=10,quant=0.0015")
    eager, tr_e = _run_tracker(track, env, net, T_T, False, torch.from_numpy(f).cuda())
    state_e, act_e = tr_e.actuation_state.cpu().numpy(), tr_e.actuation_act.cpu().numpy()
    captured, tr_c = _run_tracker(track, env, net, T_T, True, torch.from_numpy(f).cuda())
    for name, a, b in zip(("acc", "obs", "reward"), captured, eager):
        assert np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(bits(tr_c.actuation_state.cpu().numpy()), bits(state_e)) and np.array_equal(bits(tr_c.actuation_act.cpu().numpy()), bits(act_e))
    from open_duck_playground_amd import engine
    assert 0 < state_e[:, engine.ACT_DROPS].sum() < state_e[:, engine.ACT_CALLS].sum() == T_T * env.num_envs


def test_drop_one_hands_the_step_zeros(rig, monkeypatch):
    import torch
    track, env, net = rig
    seen = []
    step = env.batch.step
    monkeypatch.setattr(env.batch, "step", lambda act: (seen.append((act.data_ptr(), bool(act.any().item()))), step(act))[1])
    _, tr = _run_tracker(track, env, net, T_T, False, torch.from_numpy(_blocks(env, "drop=1")).cuda())
    assert len(seen) == T_T and all(ptr == tr.actuation_act.data_ptr() and not nonzero for ptr, nonzero in seen)


def test_track_actuation_sweep_end_to_end(tmp_path):
    from open_duck_playground_amd import actuation, track
    ckpt = RC.fresh_checkpoint(tmp_path)
    out = tmp_path / "report.json"
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--envs_per_command", "16", "--episode_length", "12", "--seed", "1", "--falls",
                                            "--command", "0.1", "0", "0", "--actuation_grid", "cutoff=5:40:3,drop=0:0.2:2", "--output", str(out)])
    rep = track.run(args)
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep))
    s = back["settings"]
    assert s["graph"] and s["num_envs"] == 96 and s["actuations_per_command"] == 6 and s["actuation"] is None
    assert s["actuation_grid"] == "cutoff=5:40:3,drop=0:0.2:2" and s["robust_fall_rate"] == 0.05 and "what the servos receive" in s["actuation_semantics"]
    assert tuple(back) == track.REPORT_KEYS and len(back["commands"]) == 1
    row = back["commands"][0]
    assert tuple(row) == track.ROW_KEYS + ("actuations", "falls", "actuation_robustness") and row["envs"] == 96
    cells = row["actuations"]
    assert [(c["actuation"]["cutoff"], c["actuation"]["drop"]) for c in cells] == [(5.0, 0.0), (5.0, 0.2), (22.5, 0.0), (22.5, 0.2), (40.0, 0.0), (40.0, 0.2)]
    for c in cells:
        assert tuple(c) == track.ROW_KEYS + ("actuation", "falls", "link") and c["envs"] == 16 and c["command"] == row["command"]
        assert tuple(c["actuation"]) == actuation.ACTUATION_KEYS and isinstance(c["falls"], dict) and tuple(c["link"]) == ("dropped_share",)
        if c["actuation"]["drop"] == 0:
            assert c["link"]["dropped_share"] == 0
        else:
            assert 0 < c["link"]["dropped_share"] < 1
    rb = row["actuation_robustness"]
    assert set(rb) == {"robust_fall_rate", "cutoff", "drop", "survived_range"} and set(rb["survived_range"]) == {"cutoff", "drop"}
    assert [p["value"] for p in rb["drop"]] == [0.0, 0.2] and [p["value"] for p in rb["cutoff"]] == [5.0, 22.5, 40.0]
    assert all(tuple(p) == track.ROBUSTNESS_POINT_KEYS for p in rb["cutoff"] + rb["drop"])


@pytest.mark.parametrize("flags,keys", [
    (["--sequence", "0: 0 0 0 | 4: 0.1 0 0", "--gait", "--path", "--randomize", "--noise_level", "0.5"], ("segments", "gait", "path")),
    (["--waypoints", "0.5,0 | 0.5,0.5", "--falls", "--imitation_report"], ("course", "path", "falls", "imitation")),
    (["--env", "standing", "--command", "0", "0", "0", "0.2", "--posture"], ("posture",))], ids=["schedule", "waypoints", "standing"])
def test_track_actuation_combines_with_the_other_flags(tmp_path, flags, keys):
    """every cell carries the other flags' objects next to its own `actuation` and `link`"""
    import torch
    from open_duck_playground_amd import track
    from open_duck_playground_amd.ppo.networks import PPONetworks
    from open_duck_playground_amd.ppo.train import save_checkpoint
    standing = "standing" in flags
    ckpt = RC.fresh_checkpoint(tmp_path)
    if standing:
        torch.manual_seed(0)
        save_checkpoint(ckpt, PPONetworks(85, 153, 14))
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--envs_per_command", "4", "--episode_length", "10", "--seed", "1",
                                            "--actuation", "drop=0.5,cutoff=20", "--actuation", "quant=0.0015,freeze=left_knee,freeze_at=3",
                                            "--output", str(tmp_path / "report.json")] + flags)
    rep = track.run(args)
    assert rep["settings"]["actuations_per_command"] == 2 and rep["settings"]["num_envs"] == 8 and len(rep["commands"]) == 1
    row = rep["commands"][0]
    cells = row["actuations"]
    assert [c["actuation"]["freeze"] for c in cells] == ["none", "left_knee"] and all(k in row for k in keys)
    for c in cells:
        assert all(k in c for k in keys) and c["envs"] == 4
    assert 0 < cells[0]["link"]["dropped_share"] < 1 and cells[1]["link"]["dropped_share"] == 0
