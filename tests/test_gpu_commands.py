"""GPU checks of caller-given commands (odk_batch_bind_commands / Joystick.set_commands): the bound row is the command across steps,
resets, auto-resets and the step-500 resample; nothing but the command and what follows from it changes (same random streams); the
env agrees with the CPU oracle env driven by the same command; a captured step graph follows the buffer's contents."""
import numpy as np
import pytest

from test_gpu_env import ENV_BOUNDS, RESET_BOUNDS, SET_ASIDE, _ids, _ill_resets, _lt, _mk, _new_W, _errs, _obs_err, _resync, _step_and_compare

pytestmark = pytest.mark.gpu

CMD = slice(6, 13)      # the command slots of `state` (both tasks; joystick.py:570-589, standing.py:524-540)


def _rows(n, seed, cfg):
    """one command per env inside the task's ranges, a few all-zero ones"""
    rng = np.random.default_rng(seed)
    lo = np.array([cfg.cmd_range[k][0] for k in range(7)], np.float32); hi = np.array([cfg.cmd_range[k][1] for k in range(7)], np.float32)
    r = (lo + rng.random((n, 7)) * (hi - lo)).astype(np.float32)
    r[::7] = 0.0
    return r


def _ref_slots(nobs, nu, standing):
    """privileged slots that are functions of the command: the reference motion (joystick.py:608-610; Standing has none)"""
    return [] if standing else list(range(nobs + 26 + 3 * nu, nobs + 66 + 3 * nu))


def test_bound_commands_hold_across_resets_and_the_step_500_resample():
    import torch
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    model = load_task_model("flat_terrain")
    n = 64
    cfg = engine.default_config()
    cfg.episode_length = 300          # truncations as well as falls: many auto-resets in 1 200 steps
    b = engine.Batch(model, n, cfg)
    assert cfg.noise_level > 0 and cfg.push_enable > 0
    rows = _rows(n, 0, cfg)
    cmd = torch.tensor(rows, device="cuda")
    b.bind_commands(cmd)
    off, cnt, kind = b.record_field("command")
    assert (cnt, kind) == (7, 0)
    b.reset(seed=5)
    np.testing.assert_array_equal(b.records()[:, off:off + 7], rows)
    np.testing.assert_array_equal(b.obs.cpu().numpy()[:, CMD], rows)
    I = b.info()
    I["step"][:] = 440 + np.arange(n)          # every env passes step 500 (the in-step resample) early in the run
    b.set_records(I["_records"])
    gen = torch.Generator(device="cuda").manual_seed(1)
    act = torch.empty(n, 14, device="cuda")
    n_done = n_resampled_steps = 0
    for t in range(1200):
        act.uniform_(-1, 1, generator=gen)
        b.step(act)
        rec = b.records()
        np.testing.assert_array_equal(rec[:, off:off + 7], rows, err_msg=f"step {t}")
        done = b.done.cpu().numpy()
        obs = b.obs.cpu().numpy()
        np.testing.assert_array_equal(obs[:, CMD], rows, err_msg=f"step {t} (obs)")   # auto-reset's first obs too
        n_done += int(done.sum())
        n_resampled_steps += int((b.info(rec)["step"] == 0).sum())
    assert n_done > n and n_resampled_steps >= n
    b.close()


def _pair(task, standing=False, dr=False, n=32, edit=None):
    import torch
    from open_duck_playground_amd import engine, randomize
    from open_duck_playground_amd.model import load_task_model
    if task.endswith(".xml"):
        from test_gpu_env import _xml_model
        model = _xml_model(task)
    else:
        model = load_task_model(task)
    bs = []
    for _ in range(2):
        cfg = engine.default_config(standing)
        if task.endswith(".xml"):
            cfg.use_imitation = 0
        cfg.episode_length = 120
        b = engine.Batch(model, n, cfg)
        if dr:
            fields, _ = randomize.domain_randomize(model, np.random.default_rng(17), n)
            randomize.apply(b, fields)
        bs.append(b)
    return torch, model, bs


@pytest.mark.parametrize("task,standing,dr", [("flat_terrain", False, False), ("flat_terrain_backlash", False, True), ("rough_terrain_backlash", False, False),
                                              ("flat_terrain", True, False), ("biped12.xml", False, False)])
def test_binding_moves_nothing_but_the_command(task, standing, dr):
    """Same seeds, same random actions, once bound and once unbound: the physics and the episode flags are bit-identical, and so is every
    output except the command slots, the reference-motion slots (a function of the command) and the command-dependent reward terms.
    info["step"] is preset near 500 so the in-step resample happens inside the window."""
    torch, model, (bu, bb) = _pair(task, standing, dr)
    n, nu = bu.nenv, model.nu
    rows = _rows(n, 3, bu.cfg)
    cmd = torch.tensor(rows, device="cuda")
    bb.bind_commands(cmd)
    for b in (bu, bb):
        b.reset(seed=9)
        I = b.info()
        I["step"][:] = 480 + np.arange(n) % 20
        b.set_records(I["_records"])
    nobs, npriv = bu.nobs, bu.npriv
    keep_obs = np.ones(nobs, bool); keep_obs[CMD] = False
    keep_priv = np.ones(npriv, bool); keep_priv[CMD] = False; keep_priv[_ref_slots(nobs, nu, standing)] = False
    # reward terms that do not read the command (metrics slots: torques, action_rate, alive, swing_peak; orientation for Standing)
    indep = [2, 3, 5, 7] + ([0] if standing else [])
    gen = torch.Generator(device="cuda").manual_seed(2)
    act = torch.empty(n, nu, device="cuda")
    n_done = 0
    for t in range(150):
        act.uniform_(-1, 1, generator=gen)
        bu.step(act); bb.step(act)
        su, sb = bu.get_state(), bb.get_state()
        for k in range(3):
            np.testing.assert_array_equal(su[k], sb[k], err_msg=f"t={t} state {k}")
        for name in ("done", "truncation"):
            np.testing.assert_array_equal(getattr(bu, name).cpu().numpy(), getattr(bb, name).cpu().numpy(), err_msg=f"t={t} {name}")
        ou, ob = bu.obs.cpu().numpy(), bb.obs.cpu().numpy()
        pu, pb = bu.priv.cpu().numpy(), bb.priv.cpu().numpy()
        np.testing.assert_array_equal(ou[:, keep_obs], ob[:, keep_obs], err_msg=f"t={t} obs")
        np.testing.assert_array_equal(pu[:, keep_priv], pb[:, keep_priv], err_msg=f"t={t} priv")
        np.testing.assert_array_equal(ob[:, CMD], rows)
        mu, mb = bu.metrics.cpu().numpy(), bb.metrics.cpu().numpy()
        np.testing.assert_array_equal(mu[:, indep], mb[:, indep], err_msg=f"t={t} metrics")
        n_done += int(bu.done.cpu().numpy().sum())
        # the random streams: the counters and keys of the records agree (the rest of info is compared through the outputs)
        Iu, Ib = bu.info(), bb.info()
        for nm in ("rng", "step", "push_step", "push_interval_steps", "push"):
            np.testing.assert_array_equal(Iu[nm], Ib[nm], err_msg=f"t={t} {nm}")
    assert n_done > 0
    bu.close(); bb.close()


BOUND_CASES = [("flat_terrain", False, 0), ("flat_terrain_backlash", False, 0), ("flat_terrain", True, 0), ("flat_terrain_backlash", False, 64)]


@pytest.mark.parametrize("task,standing,lanes", BOUND_CASES, ids=_ids(BOUND_CASES))
def test_bound_commands_match_the_oracle_env(oracle_mod, parity_log, task, standing, lanes):
    """The oracle env gets the bound row written into its `command` before every step (after reset: into its first observation's command
    slots as well, the auto-reset hands those back).  Reset: command slots equal the row, the rest within the reset bounds; steps: the
    existing parity bounds and set-aside rules.  The 64-lane case (one env per wave) is the kernel `track` runs its reports on."""
    def edit(cfg):
        cfg.episode_length = 25
    torch, model, b, envs, keep = _mk(oracle_mod, task, 32, edit, standing=standing, lanes=lanes)
    n = len(envs)
    nobs, npriv = b.nobs, b.npriv
    rows = _rows(n, 11, b.cfg)
    cmd = torch.tensor(rows, device="cuda")
    b.bind_commands(cmd)
    b.reset(seed=17)
    for i, e in enumerate(envs):
        e.reset(17, i)
    obs = b.obs.cpu().numpy(); priv = b.priv.cpu().numpy()
    np.testing.assert_array_equal(obs[:, CMD], rows)
    np.testing.assert_array_equal(priv[:, CMD], rows)
    refs = _ref_slots(nobs, model.nu, standing)
    ill = _ill_resets(envs, model, nobs)
    WR = dict(obs=0.0, acc=0.0)
    for i, e in enumerate(envs):
        # the oracle drew its own command: compare everything that does not follow from the command
        o_gpu, p_gpu = obs[i].copy(), priv[i].copy()
        o_gpu[CMD] = e["obs"][:nobs][CMD]; p_gpu[CMD] = e["priv"][:npriv][CMD]
        for k in refs:
            p_gpu[k] = e["priv"][k]
        o, a = _obs_err(o_gpu, p_gpu, e, nobs, npriv)
        WR["obs"] = max(WR["obs"], o); WR["acc"] = max(WR["acc"], 0.0 if i in ill else a)
        # from here on the oracle env carries the bound command: info, and the first observation the auto-reset hands back
        e["command"][:7] = rows[i]
        e["first_obs"][6:13] = rows[i]; e["first_priv"][6:13] = rows[i]
        for k in refs:
            e["first_priv"][k] = priv[i, k]
    rng = np.random.default_rng(8)
    W = _new_W()
    W["reset_ill"] = ill
    for t in range(40):
        _resync(b, envs, model)
        for i, e in enumerate(envs):
            e["command"][:7] = rows[i]
        act = rng.uniform(-1, 1, (n, 14)).astype(np.float32)
        _step_and_compare(torch, b, envs, act, nobs, npriv, t, W)
        np.testing.assert_array_equal(b.obs.cpu().numpy()[:, CMD], rows)
    assert W["n_done"] > 0
    b.close()
    tag = f"bound_commands/{task}/{'standing' if standing else 'joystick'}{_lt(lanes)}"
    parity_log.check(tag + "/reset", dict(obs=RESET_BOUNDS["obs"], acc=RESET_BOUNDS["acc"]), **WR)
    parity_log.check(tag, {**ENV_BOUNDS, **SET_ASIDE}, **_errs(W))


def test_a_captured_step_follows_the_buffer_and_unbinding_restores_the_sampler():
    import torch
    from open_duck_playground_amd import joystick
    env = joystick.Joystick(task="flat_terrain", num_envs=64)
    b = env.batch
    n = env.num_envs
    cmd = torch.zeros(n, 7, device="cuda")
    env.set_commands(cmd)
    assert env.commands is cmd
    env.reset(3)
    act = torch.zeros(n, 14, device="cuda")
    off = b.record_field("command")[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.step(act)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.step(act)
    rng = np.random.default_rng(0)
    for k in range(4):
        new = torch.tensor(rng.uniform(-0.5, 0.5, (n, 7)).astype(np.float32), device="cuda")
        cmd.copy_(new)                                   # stream-ordered write between two replays
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(b.records()[:, off:off + 7], new.cpu().numpy())
        np.testing.assert_array_equal(b.obs.cpu().numpy()[:, CMD], new.cpu().numpy())
    del g
    # unbinding: the sampler is back -- preset info["step"] = 500, the next step draws fresh commands
    last = cmd.cpu().numpy().copy()
    env.set_commands(None)
    assert env.commands is None
    I = b.info()
    I["step"][:] = 500
    b.set_records(I["_records"])
    b.step(act)
    now = b.records()[:, off:off + 7]
    changed = np.any(now != last, axis=1)
    assert changed.sum() >= n // 2, changed.sum()
    lo = np.array([b.cfg.cmd_range[k][0] for k in range(7)]); hi = np.array([b.cfg.cmd_range[k][1] for k in range(7)])
    assert np.all((now >= lo - 1e-6) & (now <= hi + 1e-6))
    for bad in (torch.zeros(n, 7, device="cuda", dtype=torch.float64), torch.zeros(n, 6, device="cuda"), torch.zeros(7, n, device="cuda").t(),
                torch.zeros(n, 7)):
        with pytest.raises(Exception):
            env.set_commands(bad)
    b.close()
