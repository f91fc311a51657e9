"""Reward-library terms on the GPU (include/odk.h odk_batch_set_reward_terms): turning them on moves nothing but the reward and the new
metric columns; every column equals a numpy restatement of its reference function on inputs read back from the engine; a cleared set is
bit-identical to no set; a captured graph follows later changes; and the Evaluator reports the enabled terms."""
import numpy as np
import pytest

from test_reward_terms_host import TERMS

pytestmark = pytest.mark.gpu

# (task, standing, domain randomisation, lanes per env): the cases of the commands test plus both lane widths where they exist
CASES = [("flat_terrain", False, False, 32), ("flat_terrain", False, False, 64), ("flat_terrain_backlash", False, True, 32),
         ("flat_terrain_backlash", False, True, 64), ("rough_terrain_backlash", False, False, 32), ("flat_terrain", True, False, 32),
         ("flat_terrain", True, False, 64), ("biped12.xml", False, False, 32)]
IDS = [f"{t}-{'standing' if s else 'joystick'}{'-dr' if d else ''}-G{g}" for t, s, d, g in CASES]


def _model(task):
    from open_duck_playground_amd.model import load_task_model
    if task.endswith(".xml"):
        from test_gpu_env import _xml_model
        return _xml_model(task)
    return load_task_model(task)


def _batches(task, standing, dr, lanes, n, count, episode_length=1000):
    from open_duck_playground_amd import engine, randomize
    model = _model(task)
    out = []
    for _ in range(count):
        cfg = engine.default_config(standing)
        if task.endswith(".xml"):
            cfg.use_imitation = 0
        cfg.episode_length = episode_length
        cfg.lanes_per_env = lanes
        b = engine.Batch(model, n, cfg)
        if dr:
            fields, _ = randomize.domain_randomize(model, np.random.default_rng(17), n)
            randomize.apply(b, fields)
        out.append(b)
    return model, out


def _all_terms(model, scale=None):
    """Every one of the twelve terms on, with parameters read off the model (base height target: the home keyframe's)."""
    from open_duck_playground_amd import engine
    t = engine.RewardTerms()
    sc = scale or [-1.0, -0.5, -2.0, -10.0, -1e-3, -1.0, -5.0, -0.1, -0.2, -0.3, -0.4, 2.0]
    for i, s in enumerate(sc):
        t.scale[i] = s
    t.base_height_target = float(model.a["key_qpos"][2])
    t.max_foot_height = 0.03
    t.air_time_range[0], t.air_time_range[1] = 0.1, 0.5
    t.soft_joint_pos_limit_factor = 0.95
    for u in range(model.nu):
        t.pose_weight[u] = 0.5 + 0.1 * u
    return t


@pytest.mark.parametrize("task,standing,dr,lanes", CASES, ids=IDS)
def test_terms_move_nothing_but_the_reward(task, standing, dr, lanes):
    """Same seed and actions, all twelve terms on vs none, over 1100 steps (falls and auto-resets, the step-500 resample, the episode
    limit): state, obs, privileged obs, done, truncation and the eight native metric columns are bit-identical; where neither reward is
    clipped, reward_on - reward_off = dt * (sum of the scaled library terms)."""
    import torch
    model, (off, on) = _batches(task, standing, dr, lanes, 32, 2)
    terms = _all_terms(model)
    on.set_reward_terms(terms)
    n, nu = off.nenv, model.nu
    for b in (off, on):
        b.reset(seed=5)
    assert on.xmetrics is not None and torch.count_nonzero(on.xmetrics) == 0      # the reset writes zeros
    scales = torch.tensor([terms.scale[i] for i in range(12)], device="cuda")
    dt = np.float32(off.cfg.ctrl_dt)
    gen = torch.Generator(device="cuda").manual_seed(4)
    act = torch.empty(n, nu, device="cuda")
    n_done = n_cmp = 0
    worst = 0.0
    for t in range(1100):
        act.uniform_(-1, 1, generator=gen)
        off.step(act); on.step(act)
        for name in ("obs", "priv", "done", "truncation", "metrics"):
            assert torch.equal(getattr(off, name), getattr(on, name)), f"t={t} {name}"
        if t % 50 == 0 or t > 1090:
            so, sn = off.get_state(), on.get_state()
            for k in range(3):
                np.testing.assert_array_equal(so[k], sn[k], err_msg=f"t={t} state {k}")
        # metric = scale > 0 ? scaled : -scaled  ->  scaled = sign(scale) * metric
        scaled = (torch.sign(scales) * on.xmetrics).double().sum(1)
        ro, rn = off.reward.double(), on.reward.double()
        free = (ro > 0) & (ro < 10000) & (rn > 0) & (rn < 10000)
        if bool(free.any()):
            err = ((rn - ro) - float(dt) * scaled)[free].abs()
            bound = 2e-6 * (ro[free].abs() + rn[free].abs()) + 1e-6      # float32 rounding of the two totals
            worst = max(worst, float(err.max()))
            assert bool((err <= bound).all()), (t, float(err.max()))
            n_cmp += int(free.sum())
        n_done += int(off.done.sum())
    assert n_done > n and n_cmp > 0, (n_done, n_cmp)
    off.close(); on.close()
    print(f"{task} reward identity worst |error| {worst:.2e} over {n_cmp} unclipped env-steps")


def _sadr(model, name):
    return int(model.a["sensor_adr"][model.sensor_id(name)])


@pytest.mark.parametrize("task,standing,dr,lanes", CASES, ids=IDS)
def test_metric_columns_match_the_restatement(task, standing, dr, lanes):
    """Each column against the numpy restatement of its reference function (tests/test_reward_terms_host.py, itself checked against the
    reference's outputs), on inputs read back from the engine: the info fields before and after the step (odk_record_field), the debug
    sensordata and actuator forces of the step's last forward pass, the state after it and the privileged observation's contact flags."""
    import torch
    from open_duck_playground_amd import engine
    model, (b,) = _batches(task, standing, dr, lanes, 64, 1, episode_length=1000)
    terms = _all_terms(model)
    b.set_reward_terms(terms)
    n, nu = b.nenv, model.nu
    trn = np.asarray(model.a["actuator_trnid"]).reshape(nu, -1)[:, 0]
    qadr = np.asarray(model.a["jnt_qposadr"])[trn]; dadr = np.asarray(model.a["jnt_dofadr"])[trn]
    rng_ = np.asarray(model.a["jnt_range"], np.float64).reshape(-1, 2)[trn]
    c, r = 0.5 * (rng_[:, 0] + rng_[:, 1]), rng_[:, 1] - rng_[:, 0]
    soft_lo = (c - 0.5 * r * 0.95).astype(np.float32); soft_hi = (c + 0.5 * r * 0.95).astype(np.float32)
    key_ctrl = np.asarray(model.a["key_ctrl"], np.float32).reshape(-1)[:nu]
    w = np.array([terms.pose_weight[u] for u in range(nu)], np.float32)
    s = {nm: _sadr(model, nm) for nm in ("global_linvel", "global_angvel", "upvector", "left_foot_global_linvel", "right_foot_global_linvel",
                                         "left_foot_pos", "right_foot_pos")}
    dt = np.float32(b.cfg.ctrl_dt)
    scales = np.array([terms.scale[i] for i in range(12)], np.float32)
    L = engine.load_library()
    L.odk_set_debug_dump(1)
    worst = np.zeros(12)
    checked = 0
    try:
        b.reset(seed=11)
        gen = torch.Generator(device="cuda").manual_seed(6)
        act = torch.empty(n, nu, device="cuda")
        for t in range(80):
            I0 = b.info()
            air0, lc0, peak0, cmd = I0["feet_air_time"].copy(), b.last_contact_bool(I0).astype(np.float32), I0["swing_peak"].copy(), I0["command"].copy()
            act.uniform_(-1, 1, generator=gen)
            b.step(act)
            torch.cuda.synchronize()
            dbg = b.get_debug()
            sens, af = dbg["sensordata"], dbg["actuator_force"]
            qpos, qvel, _ = b.get_state()
            priv = b.priv.cpu().numpy(); done = b.done.cpu().numpy(); trunc = b.truncation.cpu().numpy()
            xm = b.xmetrics.cpu().numpy()
            contact = priv[:, b.nobs + 16 + 3 * nu: b.nobs + 18 + 3 * nu]
            for e in range(n):
                want = np.zeros(12, np.float32)
                want[6] = TERMS["termination"](done[e] - trunc[e])
                if done[e] == 0:      # an auto-reset replaces state and observation: the rest is checked on the envs that carry on
                    se = sens[e]
                    fv = np.stack([se[s["left_foot_global_linvel"]:][:3], se[s["right_foot_global_linvel"]:][:3]])
                    fp = np.stack([se[s["left_foot_pos"]:][:3], se[s["right_foot_pos"]:][:3]])
                    fc = ((air0[e] > 0) * np.maximum(contact[e], lc0[e])).astype(np.float32)
                    air = air0[e] + dt
                    peak = np.maximum(peak0[e], fp[:, 2])
                    jq, jv = qpos[e, qadr], qvel[e, dadr]
                    want[0] = TERMS["lin_vel_z"](se[s["global_linvel"]:][:3])
                    want[1] = TERMS["ang_vel_xy"](se[s["global_angvel"]:][:3])
                    want[2] = TERMS["orientation"](se[s["upvector"]:][:3])
                    want[3] = TERMS["base_height"](qpos[e, 2], np.float32(terms.base_height_target))
                    want[4] = TERMS["energy"](jv, af[e])
                    want[5] = TERMS["joint_pos_limits"](jq, soft_lo, soft_hi)
                    want[7] = TERMS["pose"](jq, key_ctrl, w)
                    want[8] = TERMS["feet_slip"](contact[e], fv)
                    want[9] = TERMS["feet_clearance"](fv, fp, np.float32(0.03))
                    want[10] = TERMS["feet_height"](peak, fc, np.float32(0.03))
                    want[11] = TERMS["feet_air_time"](air, fc, cmd[e], np.float32(0.1), np.float32(0.5))
                    cols = range(12)
                    checked += 1
                else:
                    cols = [6]
                exp = np.where(scales > 0, want * scales, -(want * scales))
                for k in cols:
                    err = abs(float(xm[e, k]) - float(exp[k]))
                    tol = 2e-5 * abs(float(exp[k])) + 2e-6 * abs(float(scales[k])) + (2e-4 * abs(float(scales[k])) if k == 9 else 0.0)
                    worst[k] = max(worst[k], err / max(abs(float(exp[k])), 1e-6))
                    assert err <= tol, (t, e, engine.XTERM_NAMES[k], float(xm[e, k]), float(exp[k]))
    finally:
        L.odk_set_debug_dump(0)
        b.close()
    assert checked > n
    print(f"{task}: worst relative error per term " + " ".join(f"{k}={v:.1e}" for k, v in zip(engine.XTERM_NAMES, worst)))


@pytest.mark.parametrize("lanes", [32, 64])
def test_cleared_terms_are_no_terms(lanes):
    """Set and then cleared (None, and all scales 0) vs never set: bit-identical outputs, reward included."""
    import torch
    from open_duck_playground_amd import engine
    model, (never, cleared, zeroed) = _batches("flat_terrain", False, False, lanes, 32, 3)
    for b in (cleared, zeroed):
        b.set_reward_terms(_all_terms(model))
        b.reset(seed=2); b.step(torch.zeros(32, model.nu, device="cuda"))
    cleared.set_reward_terms(None)
    zeroed.set_reward_terms(engine.RewardTerms())
    assert not cleared.reward_terms_on and not zeroed.reward_terms_on
    gen = torch.Generator(device="cuda").manual_seed(8)
    act = torch.empty(32, model.nu, device="cuda")
    for b in (never, cleared, zeroed):
        b.reset(seed=3)
    for t in range(300):
        act.uniform_(-1, 1, generator=gen)
        for b in (never, cleared, zeroed):
            b.step(act)
        for b in (cleared, zeroed):
            for name in ("obs", "priv", "reward", "done", "truncation", "metrics"):
                assert torch.equal(getattr(never, name), getattr(b, name)), f"t={t} {name}"
    for b in (never, cleared, zeroed):
        b.close()


def test_a_captured_step_follows_set_reward_terms():
    """The graph is captured with terms on; set_reward_terms after the capture changes what its replays compute."""
    import torch
    from open_duck_playground_amd import engine
    model, (b,) = _batches("flat_terrain", False, False, 32, 64, 1)
    b.set_reward_terms(_all_terms(model))
    b.reset(seed=1)
    act = torch.zeros(64, model.nu, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.step(act)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.step(act)
    g.replay(); torch.cuda.synchronize()
    base_col = engine.XTERM_NAMES.index("base_height")
    assert torch.count_nonzero(b.xmetrics[:, base_col]) > 0
    # only base_height on, at ten times its scale: the other columns go to zero, this one scales
    only = _all_terms(model, scale=[0.0] * 12)
    only.scale[base_col] = -10.0
    b.set_reward_terms(only)
    g.replay(); torch.cuda.synchronize()
    m = b.xmetrics.cpu().numpy()
    assert np.count_nonzero(np.delete(m, base_col, axis=1)) == 0
    qz = b.get_state()[0][:, 2]
    live = b.done.cpu().numpy() == 0
    want = 10.0 * np.square(qz - np.float32(only.base_height_target))
    np.testing.assert_allclose(m[live, base_col], want[live], rtol=2e-5, atol=1e-7)
    # all scales 0: the replays write zeros
    b.set_reward_terms(None)
    g.replay(); torch.cuda.synchronize()
    assert torch.count_nonzero(b.xmetrics) == 0
    del g
    b.close()


def test_train_reports_enabled_terms():
    from open_duck_playground_amd import joystick
    from open_duck_playground_amd.ppo import train as T
    ov = {"reward_config.scales.feet_air_time": 2.0, "reward_config.scales.base_height": -10.0, "reward_config.base_height_target": 0.15}
    env = joystick.Joystick(task="flat_terrain", num_envs=256, config_overrides=ov)
    assert env.reward_terms() == ["base_height", "feet_air_time"]
    st = env.reset(0)
    assert {"reward/feet_air_time", "cost/base_height"} <= set(st.metrics)
    seen = []
    net, metrics = T.train(env, num_timesteps=256 * 20 * 2, seed=0, num_minibatches=4, num_updates_per_batch=1, num_evals=2,
                           progress_fn=lambda s, m: seen.append((s, m)))
    for key in ("eval/episode_reward/feet_air_time", "eval/episode_cost/base_height", "eval/episode_reward/tracking_lin_vel"):
        assert key in metrics and np.isfinite(metrics[key]), key
    assert metrics["eval/episode_cost/base_height"] > 0
    env.batch.close()
