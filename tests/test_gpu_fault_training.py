"""GPU checks of training under faults redrawn per episode: `odk_fault_resample` / `Batch.fault_resample` held bit for bit against the numpy
restatement (`fault_training.fault_resample_reference`, itself checked in tests/test_fault_training_host.py), and `FaultStage` inside
`ppo.train.rollout` / `train` on the duck on flat terrain.  There is no tolerance on a device result in this file but where two different
policy kernels are compared (the generic rollout loop against the engine path), and that bound is tests/test_gpu_api.py's for those two."""
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALLS = 12
SENTINEL = 7.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def tbits(t):
    return bits(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _batch(n):
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    return engine.Batch(load_task_model("flat_terrain"), n)


def kernel_spec():
    """All three kinds over both rows, NaN and -0.0 in FIXED slots, a kind of 7 (FIXED) and a NaN kind (FIXED)."""
    from open_duck_playground_amd import engine as E, fault_training as FT
    spec = FT.fault_spec(FT.parse_train_sensor(["gyro_bias_y=-0.2:0.2,acc_scale=0.9:1.2,imu_delay=0:3,joint_delay=2:7,encoder_offset=0.03,acc_bias_x=1.3"]),
                         FT.parse_train_actuation(["cutoff=10:40,drop=0:0.3,drop_len=1:3,offset=0.02,quant=0.0015,noise=0.05"]))
    t = FT.spec_table(spec, 0.25, 0.02, None)
    t[0, 22], t[0, 23] = np.nan, -0.0                          # FIXED: lo's bits
    t[:, 24] = 0.5, 2.5, 7.0                                   # a kind that is none of the three: FIXED
    t[:, 25] = 0.25, 2.5, np.nan
    t[:, E.SENSOR_NPRM + 8] = -3.0, 4.0, E.FAULT_WHOLE         # a WHOLE slot from a negative lo
    t[:, E.SENSOR_NPRM + 9] = 5.0, 5.0, E.FAULT_WHOLE          # an empty span
    assert {float(k) for k in t[2] if k == k} == {0.0, 1.0, 2.0, 7.0}
    return t


def done_pattern(n):
    """[CALLS, n]: env 0 never ends, env 1 ends on every call, the others now and then (env 2 on two calls running)."""
    done = (np.random.default_rng(n).random((CALLS, n)) < 0.25).astype(np.float32)
    done[:, 0], done[:, 1] = 0.0, 1.0
    done[4, 2] = done[5, 2] = 1.0
    return done


def _compare(got, want, what, call):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what} after call {call}: (env, slot) {bad[:5].tolist()} got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_kernel_has_the_restatements_bits(captured):
    """nenv = 5: four envs per wave, so one row in a second, partly empty wave; rows past the batch keep their sentinel"""
    import torch
    from open_duck_playground_amd import engine as E, fault_training as FT
    n, seed, offset = 5, 0x9E3779B1, 1000
    b, t, done = _batch(n), kernel_spec(), done_pattern(n)
    spec = torch.from_numpy(t).cuda()
    guard = [torch.full((n + 3, k), SENTINEL, device="cuda") for k in (E.FAULT_NSTATE, E.SENSOR_NPRM, E.ACT_NPRM)]
    state, sf, af = (g[:n] for g in guard)
    state[:, :2] = 0.0                                          # HEAD and EPISODE zeroed; slots 2 and 3 keep the sentinel
    done_d = torch.zeros(n, device="cuda")
    w_state = np.full((n, E.FAULT_NSTATE), SENTINEL, np.float32)
    w_state[:, :2] = 0.0
    w_sf, w_af = np.full((n, E.SENSOR_NPRM), SENTINEL, np.float32), np.full((n, E.ACT_NPRM), SENTINEL, np.float32)
    launch = lambda: b.fault_resample(done_d, spec, seed, offset, state, sf, af)
    if captured:
        keep = [x.clone() for x in (state, sf, af)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()                                            # warm-up
        torch.cuda.current_stream().wait_stream(side)
        for x, k in zip((state, sf, af), keep):
            x.copy_(k)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch()
        launch = graph.replay
    redrawn = np.zeros(n)
    for c in range(CALLS):
        done_d.copy_(torch.from_numpy(done[c]))
        launch()
        redrawn += FT.fault_resample_reference(done[c], t, seed, offset, w_state, w_sf, w_af)
        for got, want, what in ((state, w_state, "state"), (sf, w_sf, "sensor table"), (af, w_af, "actuation table")):
            _compare(got.cpu().numpy(), want, what, c)
    assert redrawn.tolist()[:2] == [1.0, float(CALLS)] and (w_state[:, E.FAULT_HEAD] == CALLS).all() and (w_state[:, 2:] == SENTINEL).all()
    assert not (w_sf == SENTINEL).any() and np.isnan(w_sf[:, 22]).all() and (bits(w_sf[:, 23]) == bits(np.float32(-0.0))).all()
    assert (w_sf[:, 24] == 0.5).all() and (w_sf[:, 25] == 0.25).all() and (w_af[:, 9] == 5.0).all()
    for g in guard:
        assert (g[n:] == SENTINEL).all()
    assert np.array_equal(bits(spec.cpu().numpy()), bits(t)), "the spec is only read"
    # done = NULL: only the first call redraws
    state.zero_()
    b.fault_resample(None, spec, seed, offset, state, sf, af)
    first = sf.clone(), af.clone()
    b.fault_resample(None, spec, seed, offset, state, sf, af)
    assert torch.equal(tbits_t(sf), tbits_t(first[0])) and torch.equal(tbits_t(af), tbits_t(first[1]))
    assert (state[:, E.FAULT_HEAD] == 2).all() and (state[:, E.FAULT_EPISODE] == 1).all()


def tbits_t(t):
    import torch
    return t.contiguous().view(torch.int32)


def test_the_binding_and_the_entry_refuse_by_name():
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine as E
    n = 5
    b = _batch(n)
    spec = torch.from_numpy(kernel_spec()).cuda()
    state = torch.zeros(n, E.FAULT_NSTATE, device="cuda")
    sf, af = torch.full((n, E.SENSOR_NPRM), SENTINEL, device="cuda"), torch.full((n, E.ACT_NPRM), SENTINEL, device="cuda")
    for args, message in (((None, spec[:2], 0, 0, state, sf, af), "fault_resample: spec: shape"),
                          ((None, spec.cpu(), 0, 0, state, sf, af), "fault_resample: spec: the tensor must live on cuda"),
                          ((None, spec, 0, 0, state[:4], sf, af), "fault_resample: state: shape"),
                          ((None, spec, 0, 0, state, sf[:, :40], af), "fault_resample: sensor_fault: shape"),
                          ((None, spec, 0, 0, state, sf, af.double()), "fault_resample: act_fault: dtype"),
                          ((torch.zeros(4, device="cuda"), spec, 0, 0, state, sf, af), "fault_resample: done"),
                          ((None, spec, -1, 0, state, sf, af), "fault_resample: seed"),
                          ((None, spec, 0, 1 << 32, state, sf, af), "fault_resample: env_id_offset")):
        with pytest.raises(E.OdkError, match=message):
            b.fault_resample(*args)
    # the C entry point's own refusals: every null pointer and every overlap, nothing launched
    L = E.load_library()
    P = lambda t: C.c_void_p(t.data_ptr())
    for k, name in ((0, "batch"), (2, "spec_dev"), (5, "state_dev"), (6, "sensor_fault_dev"), (7, "act_fault_dev")):
        args = [b._b, None, P(spec), 1, 2, P(state), P(sf), P(af), None]
        args[k] = None
        assert L.odk_fault_resample(*args) == E.ERR_INVALID and f"odk_fault_resample: null {name}" in L.odk_last_error().decode()
    rows = n * 48
    both = torch.full((2 * rows + 3 * E.FAULT_NSLOT - 2,), SENTINEL, device="cuda")      # one allocation: what overlaps what is ours to say
    at = lambda k: C.c_void_p(both.data_ptr() + 4 * k)
    # a table that begins on the other's last float; a table whose last float is the spec's first; one that begins on the spec's last
    for spec_p, tables, message in ((P(spec), [at(0), at(rows - 1)], "sensor_fault_dev overlaps act_fault_dev"),
                                    (P(spec), [at(rows - 1), at(0)], "sensor_fault_dev overlaps act_fault_dev"),
                                    (at(rows - 1), [at(0), P(af)], "sensor_fault_dev overlaps spec_dev"),
                                    (at(0), [at(3 * E.FAULT_NSLOT - 1), P(af)], "sensor_fault_dev overlaps spec_dev"),
                                    (at(rows - 1), [P(sf), at(0)], "act_fault_dev overlaps spec_dev")):
        rc = L.odk_fault_resample(b._b, None, spec_p, 1, 2, P(state), *tables, None)
        assert rc == E.ERR_INVALID and f"odk_fault_resample: {message}" in L.odk_last_error().decode(), message
    torch.cuda.synchronize()
    assert (sf == SENTINEL).all() and (af == SENTINEL).all() and (both == SENTINEL).all() and not state.any()
    assert np.array_equal(bits(spec.cpu().numpy()), bits(kernel_spec()))


# ---- the stage in a rollout
N_R = 16
CHAIN = dict(sensor=["gyro_bias_y=-0.2:0.2,imu_delay=0:3,encoder_offset=0.03"], actuation=["cutoff=10:40,noise=0.05,drop=0:0.3,quant=0.0015"])


def _env(n=N_R, **overrides):
    from open_duck_playground_amd import joystick
    return joystick.Joystick(task="flat_terrain", num_envs=n, config_overrides=overrides or None)


def _net():
    import torch
    from open_duck_playground_amd.ppo.networks import PPONetworks
    torch.manual_seed(0)
    return PPONetworks(101, 212, 14).cuda()


def _stage(env, sensor=None, act=None, seed=5):
    from open_duck_playground_amd import fault_training as FT
    spec = FT.fault_spec(FT.parse_train_sensor(sensor) if sensor else None, FT.parse_train_actuation(act) if act else None)
    return FT.FaultStage(env, spec, seed=seed)


def _rollout(env, net, T_, faults=None, seed=5, **kw):
    import torch
    from open_duck_playground_amd.ppo import train as T
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    state = env.reset(seed)
    if faults is not None:
        faults.reset()
    data, _ = T.rollout(env, net, state, T_, gen, faults=faults, **kw)
    return {k: v.clone() for k, v in data.items()}


KEYS = ("obs", "priv", "raw_action", "log_prob", "reward", "done", "truncation")


def test_a_nominal_stage_is_the_rollout_without_one():
    import torch
    from open_duck_playground_amd import engine as E
    net = _net()
    plain = _rollout(_env(), net, 6)
    env = _env()
    stage = _stage(env)
    staged = _rollout(env, net, 6, stage)
    for k in KEYS + ("last_priv",):
        assert torch.equal(tbits_t(staged[k]), tbits_t(plain[k])), k
    assert float(plain["raw_action"].abs().sum()) > 0 and torch.isfinite(plain["reward"]).all()
    # the stage ran: six calls of each launch, the SEED slots drawn, every other slot nominal
    assert (stage.fault_state[:, E.FAULT_HEAD] == 6).all() and (stage.act_state[:, E.ACT_CALLS] == 6).all()
    af = stage.act_fault.cpu().numpy()
    assert len(set(af[:, E.ACT_SEED].tolist())) == N_R
    af[:, E.ACT_SEED] = 0.0
    assert np.array_equal(bits(af), bits(E.action_fault_rows(N_R))) and np.array_equal(tbits(stage.sensor_fault), bits(E.sensor_fault_rows(N_R)))


def test_the_whole_chain_has_the_restatements_bits():
    """episode_length = 3: every env redraws at least twice inside one unroll of 8.  The engine-path rollout against a loop around env.step
    that runs the same policy launches and the three numpy restatements."""
    import torch
    from open_duck_playground_amd import actuation, engine as E, fault_training as FT, sensors
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.learner import fused_policy
    T_, seed = 8, 5
    net = _net()
    env = _env(episode_length=3)
    stage = _stage(env, CHAIN["sensor"], CHAIN["actuation"], seed=seed)
    delivered, deliver = [], stage.deliver
    stage.deliver = lambda action, done: (lambda out: (delivered.append(out.clone()), out)[1])(deliver(action, done))
    data = _rollout(env, net, T_, stage, seed=seed)
    assert len(delivered) == T_ and (stage.fault_state[:, E.FAULT_EPISODE] >= 3).all()
    assert float(stage.act_state[:, E.ACT_DROPS].sum()) > 0 and len(set(stage.sensor_fault[:, E.SENSOR_IMU_DELAY].tolist())) > 1
    # the loop: a second env, the same seed, noise as the engine path draws it
    env2 = _env(episode_length=3)
    nu, table = 14, FT.spec_table(stage.spec, stage.action_scale, stage.ctrl_dt, [str(s) for s in env2.batch.model.a["names_actuator"]])
    assert np.array_equal(tbits(stage.table), bits(table))
    fstate, sstate, astate = (np.zeros((N_R, k), np.float32) for k in (E.FAULT_NSTATE, E.SENSOR_NSTATE, E.ACT_NSTATE))
    sf, af = E.sensor_fault_rows(N_R), E.action_fault_rows(N_R)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    state = env2.reset(seed)
    noise = torch.randn(T_, N_R, nu, generator=gen, device="cuda")
    fp = fused_policy(net, N_R)
    x, raw, act, logp = (torch.zeros(N_R, k, device="cuda") for k in (101, nu, nu, 1))
    logp = logp.reshape(N_R)
    for t in range(T_):
        done = state.done.cpu().numpy()
        FT.fault_resample_reference(done, table, seed, 0, fstate, sf, af)
        seen = sensors.sensor_apply_reference(state.obs["state"].cpu().numpy(), done, sf, sstate, nu)
        x.copy_(torch.from_numpy(seen))
        logits = fp(x) if fp is not None else net.policy(net.norm_obs(x))
        E.policy_sample(logits, noise[t], out=(raw, act, logp))
        want = actuation.action_apply_reference(act.cpu().numpy(), done, af, astate, nu)
        assert np.array_equal(tbits(data["obs"][:, t]), bits(seen)), f"step {t}: obs is not the row the policy read"
        assert np.array_equal(tbits(data["raw_action"][:, t]), tbits(raw)) and np.array_equal(tbits(data["log_prob"][:, t]), tbits(logp)), t
        assert np.array_equal(tbits(delivered[t]), bits(want)), f"step {t}: the delivered action"
        assert np.array_equal(tbits(data["priv"][:, t]), tbits(state.obs["privileged_state"])), t
        state = env2.step(state, torch.from_numpy(want).cuda())
        assert np.array_equal(tbits(data["reward"][:, t]), tbits(state.reward)) and np.array_equal(tbits(data["done"][:, t]), tbits(state.done)), t
    for got, want in ((stage.fault_state, fstate), (stage.sensor_state, sstate), (stage.act_state, astate), (stage.sensor_fault, sf), (stage.act_fault, af)):
        assert np.array_equal(tbits(got), bits(want))
    assert not torch.equal(data["obs"], _rollout(_env(episode_length=3), net, T_, None, seed=seed)["obs"]), "the faults are some"


def test_the_generic_loop_runs_the_same_stage():
    """engine_path=False against the engine path, deterministic (the two draw their noise differently).  What does not pass through a policy
    kernel is equal bit for bit: step 0's observation, every done and truncation, the fault tables.  What does is compared as
    tests/test_gpu_api.py compares the two paths (their policy GEMMs round differently): step 0 within 1e-4, everything else within 2e-3 in
    all but 1 % of the entries."""
    import torch
    net, out = _net(), []
    for fast in (True, False):
        env = _env(episode_length=3)
        stage = _stage(env, CHAIN["sensor"], CHAIN["actuation"])
        out.append((_rollout(env, net, 8, stage, deterministic=True, engine_path=fast), stage))
    (a, sa), (b, sb) = out
    assert torch.equal(tbits_t(a["obs"][:, 0]), tbits_t(b["obs"][:, 0])) and not torch.equal(a["obs"][:, 0], _env().reset(5).obs["state"])
    assert torch.equal(a["done"], b["done"]) and torch.equal(a["truncation"], b["truncation"]) and float(a["done"].sum()) >= 2 * N_R
    for x, y in ((sa.sensor_fault, sb.sensor_fault), (sa.act_fault, sb.act_fault), (sa.fault_state, sb.fault_state)):
        assert torch.equal(tbits_t(x), tbits_t(y))
    for k in ("raw_action", "log_prob"):
        torch.testing.assert_close(a[k][:, 0], b[k][:, 0], rtol=1e-4, atol=1e-4)
    for k in KEYS:
        bad = ((a[k] - b[k]).abs() > 2e-3 + 2e-3 * b[k].abs()).float().mean()
        print(f"generic loop against the engine path: {k}: share of entries beyond 2e-3: {float(bad):.4f}")
        assert float(bad) < 0.01, (k, float(bad))


def test_a_tiny_training_run_under_faults(tmp_path):
    import torch
    from open_duck_playground_amd import engine as E, track
    from open_duck_playground_amd.ppo import train as T
    kw = dict(num_timesteps=256 * 20 * 2, num_minibatches=4, num_updates_per_batch=2, num_evals=2, num_eval_envs=0, tune_gemms=False)
    runs = []
    for _ in range(2):
        env = _env(256, episode_length=10)
        stage = _stage(env, ["imu_delay=0:3,acc_bias_x=1.3"], ["cutoff=15:40,drop=0:0.05"], seed=0)
        net, metrics = T.train(env, seed=0, faults=stage, **kw)
        runs.append((net, metrics, stage))
    (net, metrics, stage), (net2, _, stage2) = runs
    assert np.isfinite(metrics["training/total_loss"]) and np.isfinite(metrics["training/unroll_reward"])
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.isfinite(p).all() and torch.equal(p, q)
    assert torch.equal(stage.sensor_fault, stage2.sensor_fault) and torch.equal(stage.act_fault, stage2.act_fault)
    assert not stage.fault_state.any(), "train zeroes the stage after the epoch's reset of the env"
    assert sorted(set(stage.sensor_fault[:, E.SENSOR_IMU_DELAY].tolist())) == [0.0, 1.0, 2.0, 3.0]      # (the tables keep the last draws)
    assert (stage.sensor_fault[:, E.SENSOR_ACC_BIAS] == np.float32(1.3)).all()
    # another seed: other robots
    env = _env(256, episode_length=10)
    other = _stage(env, ["imu_delay=0:3,acc_bias_x=1.3"], ["cutoff=15:40,drop=0:0.05"], seed=1)
    state = env.reset(0)
    other.reset()
    first = _stage(env, ["imu_delay=0:3,acc_bias_x=1.3"], ["cutoff=15:40,drop=0:0.05"], seed=0)
    first.observe(state.obs["state"], state.done); other.observe(state.obs["state"], state.done)
    assert not torch.equal(first.act_fault, other.act_fault) and not torch.equal(first.sensor_fault[:, E.SENSOR_IMU_DELAY], other.sensor_fault[:, E.SENSOR_IMU_DELAY])
    # the checkpoint carries the spec, and track reads both
    path = str(tmp_path / "faulty.pt")
    T.save_checkpoint(path, net, fault_spec=stage.describe())
    spec = track.trained_under(path)
    assert spec == json.loads(json.dumps(stage.describe())) and spec["sensor"]["imu_delay"] == [0, 3] and spec["actuation"]["cutoff"] == [15.0, 40.0]
    back = track.load_networks(path, env, torch.device("cuda", 0))
    for p, q in zip(net.parameters(), back.parameters()):
        assert torch.equal(p, q)
