"""GPU checks of the velocity-tracking accumulator (odk_tracking_accumulate) and `python -m open_duck_playground_amd.track`."""
import json
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _env(n, episode_length=60, noise=True, task="flat_terrain", standing=False):
    from open_duck_playground_amd import joystick, standing as st
    ov = {"episode_length": episode_length}
    if not noise:
        ov["noise_config.level"] = 0.0
    cls = st.Standing if standing else joystick.Joystick
    return cls(task=task, num_envs=n, config_overrides=ov, lanes_per_env=64)


@pytest.mark.parametrize("standing", [False, True])
def test_accumulator_matches_a_torch_restatement(standing):
    import torch
    from open_duck_playground_amd import engine
    n = 64
    env = _env(n, standing=standing)
    b = env.batch
    rng = np.random.default_rng(0)
    cmd = torch.tensor(rng.uniform(-0.3, 0.3, (n, 7)).astype(np.float32), device="cuda")
    env.set_commands(cmd)
    env.reset(4)
    acc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    # the same sums, restated with torch ops on the same outputs
    nobs = b.nobs
    ended = torch.zeros(n, device="cuda"); steps = torch.zeros_like(ended); samples = torch.zeros_like(ended); falls = torch.zeros_like(ended)
    rew = torch.zeros_like(ended); s = torch.zeros(n, 3, device="cuda"); q = torch.zeros(n, 3, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    act = torch.empty(n, 14, device="cuda")
    for t in range(150):
        act.uniform_(-1, 1, generator=gen)
        b.step(act)
        b.tracking_accumulate(acc)
        active = ended == 0
        d = b.done != 0
        sample = active & ~d
        steps += active.float(); rew += torch.where(active, b.reward, torch.zeros_like(rew))
        falls += (active & d & (b.truncation == 0)).float()
        v = torch.stack([b.priv[:, nobs + 9], b.priv[:, nobs + 10], b.priv[:, nobs + 2]], 1)
        err = v - cmd[:, :3]
        s += torch.where(sample[:, None], v, torch.zeros_like(v)); q += torch.where(sample[:, None], err * err, torch.zeros_like(v))
        samples += sample.float()
        ended = torch.where(active & d, torch.ones_like(ended), ended)
    a = acc.cpu().numpy()
    for k, ref in ((engine.TRACK_ENDED, ended), (engine.TRACK_STEPS, steps), (engine.TRACK_SAMPLES, samples), (engine.TRACK_FALLS, falls)):
        np.testing.assert_array_equal(a[:, k], ref.cpu().numpy(), err_msg=str(k))
    np.testing.assert_allclose(a[:, engine.TRACK_REWARD], rew.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a[:, engine.TRACK_SUM:engine.TRACK_SUM + 3], s.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a[:, engine.TRACK_SQERR:engine.TRACK_SQERR + 3], q.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert ended.sum() > 0 and samples.min() > 0
    b.close()


def test_accumulator_offsets_are_the_gyro_and_the_local_linvel():
    """priv[nobs + 9 : nobs + 12] and priv[nobs : nobs + 3] are the local_linvel and gyro sensors of the last forward pass (noise off)"""
    import torch
    from open_duck_playground_amd import engine
    env = _env(32, noise=False)
    b = env.batch
    m = b.model
    adr = m.a["sensor_adr"]
    a_lin, a_gyro = int(adr[m.sensor_id("local_linvel")]), int(adr[m.sensor_id("gyro")])
    env.set_commands(torch.zeros(32, 7, device="cuda"))
    env.reset(2)
    L = engine.load_library()
    L.odk_set_debug_dump(1)
    try:
        for t in range(3):
            b.step(torch.zeros(32, 14, device="cuda"))
            sens = b.get_debug()["sensordata"]
            priv = b.priv.cpu().numpy()
            live = b.done.cpu().numpy() == 0
            np.testing.assert_array_equal(priv[live, b.nobs + 9:b.nobs + 12], sens[live, a_lin:a_lin + 3])
            np.testing.assert_array_equal(priv[live, b.nobs:b.nobs + 3], sens[live, a_gyro:a_gyro + 3])
    finally:
        L.odk_set_debug_dump(0)
    b.close()


def test_tracker_actions_equal_the_evaluators():
    import torch
    from open_duck_playground_amd import track
    from open_duck_playground_amd.ppo.learner import fused_policy
    from open_duck_playground_amd.ppo.networks import PPONetworks
    n = 64
    env = _env(n)
    torch.manual_seed(0)
    net = PPONetworks(101, 212, 14).cuda()
    env.set_commands(torch.zeros(n, 7, device="cuda"))
    tr = track.Tracker(env, net)
    tr.reset(1)
    obs = env.batch.obs.clone()
    fp = fused_policy(net, n)
    with torch.no_grad():
        logits = fp(obs) if fp is not None else net.policy(net.norm_obs(obs))     # Evaluator._one_step
        ev = torch.tanh(logits[..., :14]).contiguous()
        got = tr.actions(obs)
        torch.testing.assert_close(got, ev, rtol=0, atol=0)
        eager = torch.tanh(net.policy(net.norm_obs(obs))[..., :14])
        torch.testing.assert_close(got, eager, rtol=1e-3, atol=1e-3)
    env.batch.close()


def test_track_runs_end_to_end(tmp_path):
    import torch
    from open_duck_playground_amd import track
    from open_duck_playground_amd.ppo.networks import PPONetworks
    from open_duck_playground_amd.ppo.train import save_checkpoint
    torch.manual_seed(0)
    ckpt = str(tmp_path / "fresh.pt")
    save_checkpoint(ckpt, PPONetworks(101, 212, 14))
    out, pkl, npz = tmp_path / "report.json", tmp_path / "obs.pkl", tmp_path / "qpos.npz"
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--command", "0", "0", "0", "--command", "0.15", "0", "0", "--envs_per_command", "64",
                                            "--episode_length", "80", "--seed", "1", "--output", str(out), "--save_obs", str(pkl), "--save_qpos", str(npz)])
    rep = track.run(args)
    back = json.load(open(out))
    assert back == json.loads(json.dumps(rep))
    assert tuple(back) == track.REPORT_KEYS and len(back["commands"]) == 2
    assert back["settings"]["graph"] and back["settings"]["num_envs"] == 128 and back["settings"]["episode_length"] == 80
    for r, c in zip(back["commands"], ([0.0] * 7, [0.15] + [0.0] * 6)):
        assert tuple(r) == track.ROW_KEYS and r["command"] == pytest.approx(c) and r["envs"] == 64
        assert 0.0 <= r["fall_rate"] <= 1.0 and 0 < r["mean_episode_steps"] <= 80 and r["steps"] > 0
        assert all(np.isfinite(r[k]) for k in track.ROW_KEYS if k != "command")
    obs = pickle.load(open(pkl, "rb"))
    assert isinstance(obs, list) and len(obs) == 80 and all(isinstance(o, np.ndarray) and o.shape == (101,) for o in obs)
    np.testing.assert_array_equal(np.stack(obs)[:, 6:13], 0.0)       # env 0 runs the first command
    z = np.load(npz)
    assert z["qpos"].shape == (81, 21) and float(z["dt"]) == pytest.approx(0.02)
