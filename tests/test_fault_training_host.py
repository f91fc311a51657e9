"""Host checks of training under faults redrawn per episode (open_duck_playground_amd/fault_training.py, the `faults` argument of
ppo/train.py's `rollout` / `train`, `save_checkpoint`'s `fault_spec`): the flags' parser and the table of ranges it builds, the numpy
restatement of `odk_fault_resample`, and the rollout's contract on a CPU toy env.  No GPU, no libodk.so."""
import json
import sys

import numpy as np
import pytest
import torch

from open_duck_playground_amd import actuation, engine, fault_training as FT, sensors
from open_duck_playground_amd.ppo import train as T

E = engine
SCALE, DT = 0.25, 0.02
NAMES = ["left_hip_yaw", "left_knee", "right_knee"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def table(sensor=None, act=None, names=NAMES):
    spec = FT.fault_spec(FT.parse_train_sensor(sensor) if sensor else None, FT.parse_train_actuation(act) if act else None)
    return FT.spec_table(json.loads(json.dumps(spec)), SCALE, DT, names)      # (as a checkpoint hands it back: lists for ranges)


def slot(t, s):
    return tuple(float(x) for x in t[:, s])


# ---- parsing
def test_every_kind_of_slot_is_built():
    t = table(["gyro_bias_y=-0.2:0.2,imu_delay=0:3", "acc_bias_x=1.3,encoder_offset=0.03,contact_left=off,imu_yaw=90"],
              ["cutoff=10:40,noise=0.05", "drop=0:0.3,quant=0.0015,offset=0.02,drop_len=1:3,freeze=left_knee,freeze_at=7"])
    assert t.dtype == np.float32 and t.shape == (3, E.FAULT_NSLOT) and E.FAULT_NSLOT == 96
    f32 = lambda x: float(np.float32(x))
    S, A = t[:, :E.SENSOR_NPRM], t[:, E.SENSOR_NPRM:]
    assert slot(S, E.SENSOR_GYRO_BIAS + 1) == (f32(-0.2), f32(0.2), E.FAULT_UNIFORM)
    assert slot(S, E.SENSOR_IMU_DELAY) == (0.0, 3.0, E.FAULT_WHOLE)                        # whole steps, both ends included
    assert slot(S, E.SENSOR_ACC_BIAS) == (f32(1.3), f32(1.3), E.FAULT_FIXED)
    assert slot(S, E.SENSOR_CONTACT_MODE) == (1.0, 1.0, E.FAULT_FIXED) and slot(S, E.SENSOR_CONTACT_MODE + 1) == (0.0, 0.0, E.FAULT_FIXED)
    assert np.array_equal(bits(S[0, :9]), bits(engine.sensor_rotation(0, 0, 90).reshape(9))) and not S[2, :9].any()      # built on the host
    for u in range(16):
        assert slot(S, E.SENSOR_ENC_OFFSET + u) == (f32(-0.03), f32(0.03), E.FAULT_UNIFORM)
        assert slot(A, E.ACT_OFFSET + u) == (-f32(0.02 / SCALE), f32(0.02 / SCALE), E.FAULT_UNIFORM)      # action units
        assert slot(A, E.ACT_FREEZE_AT + u) == ((7.0, 7.0, 0.0) if u == 1 else (-1.0, -1.0, 0.0))
    # cutoff=a:b: uniform in the coefficient, from the higher cutoff's (the smaller) to the lower cutoff's
    assert slot(A, E.ACT_ALPHA) == (float(actuation.filter_alpha(40, DT)), float(actuation.filter_alpha(10, DT)), E.FAULT_UNIFORM)
    assert A[0, E.ACT_ALPHA] < A[1, E.ACT_ALPHA]
    assert slot(A, E.ACT_QUANT) == (f32(0.0015 / SCALE),) * 2 + (E.FAULT_FIXED,)            # radians / action_scale, as actuation.fault_row
    assert slot(A, E.ACT_NOISE) == (f32(0.05), f32(0.05), E.FAULT_FIXED) and slot(A, E.ACT_DROP_P) == (0.0, f32(0.3), E.FAULT_UNIFORM)
    assert slot(A, E.ACT_DROP_LEN) == (1.0, 3.0, E.FAULT_WHOLE) and slot(A, E.ACT_GAIN) == (1.0, 1.0, E.FAULT_FIXED)
    assert slot(A, E.ACT_SEED) == (0.0, float(2 ** 24 - 1), E.FAULT_WHOLE)
    tq = table(None, ["quant=0.001:0.002"])
    assert slot(tq[:, E.SENSOR_NPRM:], E.ACT_QUANT) == (f32(0.001 / SCALE), f32(0.002 / SCALE), E.FAULT_UNIFORM)


def test_the_fixed_part_is_tracks_own_rows_and_nominal_is_nominal():
    t = table()
    fixed = t[2] == E.FAULT_FIXED
    assert not t[2, :E.SENSOR_NPRM].any() and np.array_equal(bits(t[0])[fixed], bits(t[1])[fixed])
    assert np.array_equal(bits(t[0, :E.SENSOR_NPRM]), bits(engine.sensor_fault_rows(1)[0]))
    assert np.array_equal(bits(t[0, E.SENSOR_NPRM:]), bits(engine.action_fault_rows(1)[0]))      # (SEED's lo is the nominal 0)
    assert [int(s) for s in np.flatnonzero(t[2])] == [E.SENSOR_NPRM + E.ACT_SEED]          # the SEED slot is always drawn
    s, a = "gyro_scale=1.1,acc_bias_z=-0.4,imu_roll=3,joint_delay=2,encoder_quant=0.0015,contact_right=on", "gain=0.9,limit=0.8,cutoff=37.5,drop_len=2"
    t = table([s], [a])
    assert np.array_equal(bits(t[0, :E.SENSOR_NPRM]), bits(sensors.fault_row(sensors.parse_sensor(s))))
    want = actuation.fault_row(actuation.parse_actuation(a), SCALE, DT, NAMES)
    assert np.array_equal(bits(t[0, E.SENSOR_NPRM:]), bits(want))


@pytest.mark.parametrize("parse,flag,items,key,why", [
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_w=0.1"], "gyro_bias_w", "unknown key"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_w=0:1"], "gyro_bias_w", "unknown key"),
    (FT.parse_train_sensor, "--train_sensor", ["imu_delay=0:9"], "imu_delay", "outside the sample ring"),
    (FT.parse_train_sensor, "--train_sensor", ["imu_delay=0.5:3"], "imu_delay", "not a whole number"),
    (FT.parse_train_sensor, "--train_sensor", ["imu_pitch=-5:5"], "imu_pitch", "takes one value"),
    (FT.parse_train_sensor, "--train_sensor", ["contact_left=ok:on"], "contact_left", "takes one value"),
    (FT.parse_train_sensor, "--train_sensor", ["encoder_offset=0:0.03"], "encoder_offset", "already a bound"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_x=0.2:-0.2"], "gyro_bias_x", "LO above HI"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_x=0:1:3"], "gyro_bias_x", "LO:HI"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_x=0:"], "gyro_bias_x", "LO:HI"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_x=0:nan"], "gyro_bias_x", "not finite"),
    (FT.parse_train_sensor, "--train_sensor", ["gyro_bias_x=0.1", "acc_scale=1,gyro_bias_x=0:1"], "gyro_bias_x", "given twice"),
    (FT.parse_train_sensor, "--train_sensor", ["imu_delay"], "imu_delay", "KEY=VALUE"),
    (FT.parse_train_sensor, "--train_sensor", [" , "], "key", "no key given"),
    (FT.parse_train_actuation, "--train_actuation", ["cutoff=0:40"], "cutoff", "filter off"),
    (FT.parse_train_actuation, "--train_actuation", ["cutoff=-1:40"], "cutoff", "negative"),
    (FT.parse_train_actuation, "--train_actuation", ["offset=0:0.02"], "offset", "already a bound"),
    (FT.parse_train_actuation, "--train_actuation", ["freeze=left_knee:right_knee"], "freeze", "takes one value"),
    (FT.parse_train_actuation, "--train_actuation", ["freeze_at=0:10"], "freeze_at", "takes one value"),
    (FT.parse_train_actuation, "--train_actuation", ["drop=0:1.5"], "drop", "outside 0 .. 1"),
    (FT.parse_train_actuation, "--train_actuation", ["drop_len=0:2"], "drop_len", "below 1"),
    (FT.parse_train_actuation, "--train_actuation", ["torque=1"], "torque", "unknown key")])
def test_every_refusal_names_the_flag_and_the_key(parse, flag, items, key, why):
    with pytest.raises(ValueError) as err:
        parse(items)
    text = str(err.value)
    assert text.startswith(flag + ":") and key in text and why in text, text


def test_a_freeze_the_robot_lacks_is_refused_as_the_training_flags():
    with pytest.raises(ValueError, match="--train_actuation: freeze='tail'"):
        table(None, ["freeze=tail"])


def test_the_runner_takes_the_flags_and_refuses_at_parse_time(capsys):
    from open_duck_playground_amd import runner
    p = runner.build_parser()
    args = p.parse_args(["--train_sensor", "imu_delay=0:3,acc_bias_x=1.3", "--train_actuation", "cutoff=15:40", "--train_actuation", "drop=0:0.05"])
    runner.check_env_flags(p, args)
    spec = FT.spec_from_args(args)
    assert spec["sensor"]["imu_delay"] == [0, 3] and spec["sensor"]["acc_bias_x"] == 1.3 and spec["sensor"]["gyro_scale"] == 1.0
    assert spec["actuation"]["cutoff"] == [15.0, 40.0] and spec["actuation"]["drop"] == [0.0, 0.05] and spec["actuation"]["freeze"] == "none"
    assert json.loads(json.dumps(spec)) == spec
    assert FT.spec_from_args(p.parse_args([])) is None                                      # no flag: no stage, not a nominal one
    with pytest.raises(SystemExit):
        runner.check_env_flags(p, p.parse_args(["--train_actuation", "cutoff=0:40"]))
    assert "--train_actuation: cutoff=0:40" in capsys.readouterr().err


# ---- the restatement
N = 4096


def _run(t, n=N, seed=3, offset=0, calls=1, done=None, sentinel=7.0):
    state = np.zeros((n, E.FAULT_NSTATE), np.float32)
    sf, af = np.full((n, E.SENSOR_NPRM), sentinel, np.float32), np.full((n, E.ACT_NPRM), sentinel, np.float32)
    for c in range(calls):
        FT.fault_resample_reference(None if done is None else done[c], t, seed, offset, state, sf, af)
    return state, sf, af


def test_whole_slots_stay_inside_their_range_and_take_every_value():
    t = table(["imu_delay=0:3,joint_delay=2:7"], ["drop_len=1:3"])
    state, sf, af = _run(t)
    assert (state[:, E.FAULT_HEAD] == 1).all() and (state[:, E.FAULT_EPISODE] == 1).all()
    assert sorted(set(sf[:, E.SENSOR_IMU_DELAY].tolist())) == [0.0, 1.0, 2.0, 3.0]
    assert sorted(set(sf[:, E.SENSOR_JOINT_DELAY].tolist())) == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert sorted(set(af[:, E.ACT_DROP_LEN].tolist())) == [1.0, 2.0, 3.0]
    seeds = af[:, E.ACT_SEED]
    assert (seeds == np.floor(seeds)).all() and seeds.min() >= 0 and seeds.max() <= 2 ** 24 - 1 and len(set(seeds.tolist())) > N - 8


def test_uniform_slots_have_the_midpoints_mean():
    t = table(["gyro_bias_y=-0.2:0.2,acc_scale=0.9:1.2,encoder_offset=0.03"], ["cutoff=10:40,drop=0:0.3,offset=0.02"])
    checked = 0
    for seed, offset in ((3, 0), (4, 8192)):
        _, sf, af = _run(t, seed=seed, offset=offset)
        both = np.concatenate([sf, af], axis=1).astype(np.float64)
        for s in np.flatnonzero(t[2] == E.FAULT_UNIFORM):
            lo, hi = float(t[0, s]), float(t[1, s])
            sigma = (hi - lo) / np.sqrt(12 * N)
            assert lo <= both[:, s].min() and both[:, s].max() <= hi
            assert abs(both[:, s].mean() - 0.5 * (lo + hi)) <= 5 * sigma, (seed, s, both[:, s].mean(), lo, hi)
            checked += 1
    assert checked == 2 * (2 + 16 + 2 + 16)
    # the slots are drawn apart: two actuators' offsets of one env are not the same number
    assert not np.array_equal(sf[:, E.SENSOR_ENC_OFFSET], sf[:, E.SENSOR_ENC_OFFSET + 1])


def test_an_env_without_done_keeps_both_rows_bits_and_a_done_one_is_redrawn():
    n, calls = 6, 5
    t = table(["gyro_bias_y=-0.2:0.2,imu_delay=0:3"], ["drop=0:0.3"])
    t[0, 3], t[0, 5], t[2, 7] = np.nan, -0.0, 7.0                                             # FIXED keeps NaN and -0.0; a kind of 7 is FIXED
    done = np.zeros((calls, n), np.float32)
    done[:, 1] = 1.0                                                                        # env 1 ends on every call, env 0 never
    done[2, 2] = done[3, 2] = done[3, 3] = 1.0
    state = np.zeros((n, E.FAULT_NSTATE), np.float32)
    state[:, 2:] = 5.0
    sf, af = np.full((n, E.SENSOR_NPRM), 7.0, np.float32), np.full((n, E.ACT_NPRM), 7.0, np.float32)
    episodes = np.zeros(n)
    for c in range(calls):
        before = bits(sf).copy(), bits(af).copy()
        redraw = FT.fault_resample_reference(done[c], t, 11, 1000, state, sf, af)
        assert np.array_equal(redraw, (done[c] != 0) | (c == 0))
        episodes += redraw
        keep = ~redraw
        assert np.array_equal(bits(sf)[keep], before[0][keep]) and np.array_equal(bits(af)[keep], before[1][keep])
        if c:
            assert not np.array_equal(bits(sf)[1], before[0][1]) and not np.array_equal(bits(af)[1], before[1][1])
        assert (state[:, E.FAULT_HEAD] == c + 1).all() and np.array_equal(state[:, E.FAULT_EPISODE], episodes) and (state[:, 2:] == 5.0).all()
    assert not (sf == 7.0).any() and not (af == 7.0).any()                                  # a redraw writes all 96 slots
    assert np.isnan(sf[:, 3]).all() and (bits(sf[:, 5]) == bits(np.float32(-0.0))).all() and (bits(sf[:, 7]) == bits(t[0, 7])).all()
    # the draw is a function of (seed, env_id_offset + e, episode, slot) alone: env 1 of this run is env 0 of a run one env further on
    s2 = np.zeros((1, E.FAULT_NSTATE), np.float32)
    sf2, af2 = np.zeros((1, E.SENSOR_NPRM), np.float32), np.zeros((1, E.ACT_NPRM), np.float32)
    for c in range(calls):
        FT.fault_resample_reference(np.ones(1, np.float32), t, 11, 1001, s2, sf2, af2)
    assert np.array_equal(bits(sf2[0]), bits(sf[1])) and np.array_equal(bits(af2[0]), bits(af[1]))
    _, sf3, _ = _run(t, n=n, seed=12, offset=1000)
    assert not np.array_equal(sf3[:, E.SENSOR_GYRO_BIAS + 1], _run(t, n=n, seed=11, offset=1000)[1][:, E.SENSOR_GYRO_BIAS + 1])


# ---- the checkpoint
def test_checkpoint_round_trip_of_the_fault_spec(tmp_path):
    from open_duck_playground_amd import track
    from open_duck_playground_amd.ppo.networks import PPONetworks
    torch.manual_seed(0)
    net = PPONetworks(5, 7, 2, (8, 8), (8, 8))
    spec = dict(FT.fault_spec(FT.parse_train_sensor(["imu_delay=0:3"]), None), seed=4, redrawn="per episode")
    spec = json.loads(json.dumps(spec))
    T.save_checkpoint(str(tmp_path / "with.pt"), net, fault_spec=spec)
    T.save_checkpoint(str(tmp_path / "without.pt"), net)
    with_, without = torch.load(str(tmp_path / "with.pt")), torch.load(str(tmp_path / "without.pt"))
    assert tuple(with_) == ("networks", "fault_spec") and tuple(without) == ("networks",)      # an old reader finds what it always found
    assert with_["fault_spec"] == spec and track.trained_under(str(tmp_path / "with.pt")) == spec
    assert track.trained_under(str(tmp_path / "without.pt")) is None
    for k, v in net.state_dict().items():
        assert torch.equal(with_["networks"][k], v)


# ---- the rollout's contract, on a CPU toy env
class _Toy:
    def __init__(self, n=8):
        self.num_envs, self.device, self.action_size = n, torch.device("cpu"), 2
        self.observation_size = {"state": (5,), "privileged_state": (7,)}
        self.resets, self.stepped = 0, []

    def make_eval_env(self, n):
        return _Toy(n)

    def _state(self, reward, done):
        from open_duck_playground_amd.joystick import State
        obs = torch.full((self.num_envs, 5), float(self.t))
        return State(data=None, obs={"state": obs, "privileged_state": torch.full((self.num_envs, 7), float(self.t))}, reward=reward, done=done,
                     metrics={}, info={"truncation": torch.zeros(self.num_envs)})

    def reset(self, seed):
        self.resets += 1
        self.t = 0
        return self._state(torch.zeros(self.num_envs), torch.zeros(self.num_envs))

    def step(self, state, action):
        self.stepped.append(action.clone())
        self.t += 1
        return self._state(action[:, 0].clone(), torch.full((self.num_envs,), float(self.t % 3 == 0)))


class _Stage:
    """A stand-in with FaultStage's surface: the observation plus 100, the action halved; it records what it was handed."""

    def __init__(self):
        self.resets, self.log = 0, []

    def reset(self):
        self.resets += 1
        self.log.append("reset")

    def observe(self, obs, done):
        self.log.append(("observe", obs.clone(), done.clone()))
        return obs + 100.0

    def deliver(self, action, done):
        self.log.append(("deliver", action.clone(), done.clone()))
        return action * 0.5


def test_rollout_records_what_the_policy_read_and_steps_with_what_was_delivered():
    from open_duck_playground_amd.ppo.networks import PPONetworks
    torch.manual_seed(0)
    env, stage, net = _Toy(), _Stage(), PPONetworks(5, 7, 2, (8, 8), (8, 8))
    gen = torch.Generator().manual_seed(1)
    data, state = T.rollout(env, net, env.reset(0), 4, gen, faults=stage)
    for t in range(4):
        assert (data["obs"][:, t] == 100.0 + t).all() and (data["priv"][:, t] == float(t)).all()      # the stage's row; priv stays the env's
        kind, obs, done = stage.log[2 * t]
        assert kind == "observe" and (obs == float(t)).all() and (done == float(t > 0 and t % 3 == 0)).all()
        kind, action, done2 = stage.log[2 * t + 1]
        assert kind == "deliver" and torch.equal(done2, done)                                  # the same done, before the step replaces it
        assert torch.equal(action, torch.tanh(data["raw_action"][:, t])) and torch.equal(env.stepped[t], action * 0.5)
        loc, scale = net.dist_params(data["obs"][:, t])
        assert torch.allclose(data["log_prob"][:, t], T.tanh_normal_log_prob(loc, scale, data["raw_action"][:, t]))
    assert len(stage.log) == 8
    # without a stage: the env's own rows, the policy's own action
    env2 = _Toy()
    data2, _ = T.rollout(env2, net, env2.reset(0), 4, torch.Generator().manual_seed(1))
    assert (data2["obs"][:, 2] == 2.0).all() and torch.equal(env2.stepped[1], torch.tanh(data2["raw_action"][:, 1]))


KW = dict(num_evals=3, unroll_length=5, num_minibatches=4, num_updates_per_batch=1, episode_length=20, num_eval_envs=4,
          network_factory=dict(policy_hidden_layer_sizes=(8, 8), value_hidden_layer_sizes=(8, 8)))


def test_train_resets_the_stage_after_every_env_reset_and_evaluates_without_it():
    env, stage = _Toy(), _Stage()
    T.train(env, num_timesteps=8 * 5 * 4, seed=0, faults=stage, **KW)
    assert env.resets == 3 and stage.resets == 3 and stage.log[0] == "reset"
    observed = sum(1 for x in stage.log if x != "reset" and x[0] == "observe")
    assert observed == len(env.stepped) == 2 * 2 * 5                                        # the training env's steps only: the Evaluator has its own env
    assert all(x[1].shape[0] == 8 for x in stage.log if x != "reset")


def test_train_without_faults_never_touches_the_stage(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the fault stage was used without faults")
    for name in ("__init__", "reset", "observe", "deliver", "describe"):
        monkeypatch.setattr(FT.FaultStage, name, boom)
    monkeypatch.setitem(sys.modules, "open_duck_playground_amd.fault_training", None)      # an import of it raises ImportError
    env = _Toy()
    net, _ = T.train(env, num_timesteps=8 * 5 * 4, seed=0, faults=None, **KW)
    net2, _ = T.train(_Toy(), num_timesteps=8 * 5 * 4, seed=0, **KW)
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(a, b)
    assert env.resets == 3
