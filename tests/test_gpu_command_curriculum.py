"""GPU checks of the command curriculum: `odk_curriculum_step` / `Batch.curriculum_step` and `odk_curriculum_update` /
`Batch.curriculum_update` held bit for bit against the numpy restatements (`command_curriculum.curriculum_step_reference` /
`curriculum_update_reference`, themselves checked in tests/test_command_curriculum_host.py), and `CommandCurriculum` inside
`ppo.train.rollout` / `train` on the duck on flat terrain.  There is no tolerance on a device result in this file."""
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
HEAD = [(-0.34, 1.1), (-0.78, 0.78), (-1.5, 1.5), (-0.5, 0.5)]
N, CALLS, GUARD = 70, 40, 3
BOUNDARY, NANS = 5, 6      # the env that sits on both `<=`, the env whose velocities are NaN
BOUNDARY_ROW = np.array([0.125, -0.125, 0.5, 0.0, 0.0, 0.0, 0.0], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def tbits(t):
    return bits(t.detach().cpu().numpy())


def _same(got, want, what, call):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    same = np.array_equal(got, want) if got.dtype == np.int32 else np.array_equal(bits(got), bits(want))
    if not same:
        bad = np.argwhere((got != want) if got.dtype == np.int32 else (bits(got) != bits(want)))
        raise AssertionError(f"{what} after call {call}: at {bad[:5].tolist()} got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")


@functools.lru_cache(maxsize=None)
def _batch(n):
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import load_task_model
    return engine.Batch(load_task_model("flat_terrain"), n)


def step_struct(seed=0x9E3779B1, offset=1000, tol_lin=0.25, **kw):
    from open_duck_playground_amd import command_curriculum as CC
    spec = CC.curriculum_spec("vx=-0.15:0.222:2,wz=-1.2:1.2:2", None, period=6, skip=1, min_samples=3, tol_lin=tol_lin, tol_yaw=0.5, **kw)
    return CC.curriculum_struct(spec, HEAD, seed, offset)


def done_pattern(n):
    """[CALLS, n] done and truncation: env 0 never ends, env 1 ends on every call (a fall and a truncation in turn), env 2 falls on call 4 and
    is truncated on call 5, env 3 ends on call 6 -- its first stint began with the first call, so STEP reaches the period of 6 on that very
    call -- the others end now and then."""
    rng = np.random.default_rng(n)
    done = (rng.random((CALLS, n)) < 0.06).astype(np.float32)
    trunc = done * (rng.random((CALLS, n)) < 0.5).astype(np.float32)
    done[:, 0] = trunc[:, 0] = 0.0
    done[:, 1], trunc[:, 1] = 1.0, np.arange(CALLS) % 2
    done[:7, 2:4] = trunc[:7, 2:4] = 0.0
    done[4, 2], done[5, 2], trunc[5, 2], done[6, 3] = 1.0, 1.0, 1.0, 1.0
    done[:, BOUNDARY] = trunc[:, BOUNDARY] = 0.0
    return done, trunc


def velocity_errors(n):
    """[n, 3] what an env's velocities are off its command by: well inside the tolerances (0.25 planar, 0.5 yaw), just inside, just beyond
    one of them, far beyond; the BOUNDARY env exactly on both (its command row is kept at BOUNDARY_ROW, so that the differences are exact:
    every sample adds 0.0625 and 0.25, and SQLIN == 0.0625 SAMPLES, SQYAW == 0.25 SAMPLES to the bit); NaN for one env."""
    kinds = np.array([[0.01, -0.02, 0.05], [0.17, 0.17, 0.49], [0.18, 0.18, 0.1], [0.05, 0.05, 0.51], [1.0, -1.0, 3.0]], np.float32)
    err = kinds[np.arange(n) % len(kinds)].copy()
    err[BOUNDARY], err[NANS] = (0.25, 0.0, 0.5), np.nan
    return err


def _capture(torch, launch, tensors):
    keep = [x.clone() for x in tensors]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    for x, k in zip(tensors, keep):
        x.copy_(k)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for x, k in zip(tensors, keep):                         # (capturing launches nothing; all the same)
        x.copy_(k)
    return graph.replay


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_step_kernel_has_the_restatements_bits(captured):
    """nenv = 70: a second, partly empty wave, and about 17 envs per bin, so the atomics collide; 40 calls of period 6."""
    import torch
    from open_duck_playground_amd import command_curriculum as CC, engine as E
    b = _batch(N)
    nobs, npriv = b.nobs, b.npriv
    cur = step_struct()
    levels = np.array([5, 1, 0, 3], np.int32)
    w_cdf = np.cumsum(levels).astype(np.int32)
    done, trunc = done_pattern(N)
    err = velocity_errors(N)
    G = lambda k: torch.full((N + GUARD, k), SENTINEL, device="cuda")
    g_state, g_cmd, g_obs, g_priv = G(E.CURR_NSTATE), G(7), G(nobs), G(npriv)
    state, cmd, obs, priv = g_state[:N], g_cmd[:N], g_obs[:N], g_priv[:N]
    state.zero_()
    cdf, counts = torch.from_numpy(w_cdf).cuda(), torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    done_d, trunc_d = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    w_state, w_cmd = np.zeros((N, E.CURR_NSTATE), np.float32), np.full((N, 7), SENTINEL, np.float32)
    w_obs, w_priv, w_counts = np.full((N, nobs), SENTINEL, np.float32), np.full((N, npriv), SENTINEL, np.float32), np.zeros((4, 2), np.int32)
    b.bind_commands(cmd)
    try:
        launch = lambda: b.curriculum_step(cur, priv, done_d, trunc_d, cdf, counts, state, cmd, obs=obs)
        if captured:
            launch = _capture(torch, launch, (state, cmd, obs, priv, counts))
        drew = np.zeros(N)
        for c in range(CALLS):
            w_cmd[BOUNDARY] = BOUNDARY_ROW
            with np.errstate(invalid="ignore"):
                w_priv[:, nobs + 9], w_priv[:, nobs + 10], w_priv[:, nobs + 2] = w_cmd[:, 0] + err[:, 0], w_cmd[:, 1] + err[:, 1], w_cmd[:, 2] + err[:, 2]
            cmd.copy_(torch.from_numpy(w_cmd)); priv.copy_(torch.from_numpy(w_priv))
            done_d.copy_(torch.from_numpy(done[c])); trunc_d.copy_(torch.from_numpy(trunc[c]))
            launch()
            drew += CC.curriculum_step_reference(cur, nobs, w_priv, done[c], trunc[c], w_cdf, w_counts, w_state, w_cmd, w_obs)
            for got, want, what in ((state, w_state, "state"), (cmd, w_cmd, "commands"), (obs, w_obs, "obs"), (priv, w_priv, "priv"),
                                    (counts, w_counts, "counts")):
                _same(got, want, what, c)
        # what the pattern was built for
        assert drew[0] == 1 + (CALLS - 1) // 6 and drew[1] == CALLS and w_state[1, E.CURR_EPISODE] == CALLS and w_state[0, E.CURR_EPISODE] == 1
        assert (w_state[:, E.CURR_HEAD] == CALLS).all() and w_counts[:, 0].sum() > 100 and 0 < w_counts[:, 1].sum() < w_counts[:, 0].sum()
        assert (w_counts[2] == 0).all(), "a closed bin is never drawn"
        assert (w_obs[:, :6] == SENTINEL).all() and (w_obs[:, 13:] == SENTINEL).all() and (w_priv[:, :6] == SENTINEL).all()
        assert np.array_equal(w_obs[:, 6:13], w_priv[:, 6:13]) and np.isnan(w_priv[NANS, nobs + 9])
        for g in (g_state, g_cmd, g_obs, g_priv):
            assert (g[N:] == SENTINEL).all()
        assert np.array_equal(cdf.cpu().numpy(), w_cdf), "the cdf is only read"
        # the envs alone (their own counts): the boundary env succeeds, and fails once the tolerance is one ulp smaller; NaN never succeeds
        def alone(e, tol_lin=0.25):
            one = step_struct(offset=1000 + e, tol_lin=tol_lin)
            s, k, p, cnt = np.zeros((1, E.CURR_NSTATE), np.float32), np.zeros((1, 7), np.float32), np.zeros((1, npriv), np.float32), np.zeros((4, 2), np.int32)
            for c in range(CALLS):
                if e == BOUNDARY:
                    k[0] = BOUNDARY_ROW
                with np.errstate(invalid="ignore"):
                    p[0, nobs + 9], p[0, nobs + 10], p[0, nobs + 2] = k[0, 0] + err[e, 0], k[0, 1] + err[e, 1], k[0, 2] + err[e, 2]
                CC.curriculum_step_reference(one, nobs, p, done[c, e:e + 1], trunc[c, e:e + 1], w_cdf, cnt, s, k)
            assert np.array_equal(bits(s), bits(w_state[e:e + 1])), e
            return cnt.sum(0).tolist()
        tries, wins = alone(BOUNDARY)
        assert tries == wins >= 3 and alone(BOUNDARY, float(np.nextafter(np.float32(0.25), np.float32(0))))[1] == 0
        tries, wins = alone(NANS)
        assert tries >= 1 and wins == 0
        assert alone(2)[0] >= 1 and alone(3)[0] >= 1      # the fall and the truncation in a row; the period's end on a done call
        # done = None: only the first call draws (period 6: five more calls end nothing)
        state.zero_()
        b.curriculum_step(cur, priv, None, None, cdf, counts, state, cmd, obs=obs)
        first = cmd.clone()
        for _ in range(5):
            b.curriculum_step(cur, priv, None, None, cdf, counts, state, cmd, obs=None, patch_priv=False)
        assert torch.equal(cmd, first) and (state[:, E.CURR_HEAD] == 6).all() and (state[:, E.CURR_EPISODE] == 1).all() and (state[:, E.CURR_STEP] == 5).all()
        # total == 0: the zero command for every env
        state.zero_(); cdf.zero_()
        b.curriculum_step(cur, priv, None, None, cdf, counts, state, cmd, obs=obs)
        assert not cmd.any() and (state[:, E.CURR_BIN] == -1).all() and not obs[:, 6:13].any() and (obs[:, 13:] == SENTINEL).all()
    finally:
        b.bind_commands(None)


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 3, 5), (16, 16, 16)], ids=["1", "105", "4096"])
def test_update_kernel_has_the_restatements_bits(shape):
    """105 bins: more than one wave's width and no multiple of 64.  Counters random, with runs of adjacent bins all judged and promoted in the
    same call (a lane's neighbour in the next lane, and 64 bins on in the same lane: the read-before-zero hazard); levels at 0, in the
    middle and at LMAX; three updates in a row, fresh tries added between them."""
    import torch
    from open_duck_playground_amd import command_curriculum as CC, engine as E
    b = _batch(5)
    nbins = int(np.prod(shape))
    spec = CC.curriculum_spec(f"vx=0:1:{shape[0]},vy=0:1:{shape[1]},wz=0:1:{shape[2]}", "vx=0:1,vy=0:1,wz=0:1", min_tries=8, promote_rate=0.75)
    cur = CC.curriculum_struct(spec, HEAD)
    rng = np.random.default_rng(nbins)
    w_levels = rng.choice(np.array([0, 0, 2, 3, 5], np.int32), nbins).astype(np.int32)
    w_levels[0] = 0
    w_cdf, w_counts, w_stats = np.full(nbins, -3, np.int32), np.zeros((nbins, 2), np.int32), np.array([3, 2, 1, 0], np.int32)
    G = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1), np.full(4, 77, np.int32)])).cuda()
    g = [G(a) for a in (w_levels, w_cdf, w_counts, w_stats)]
    levels, cdf, counts, stats = g[0][:nbins], g[1][:nbins], g[2][:2 * nbins].view(nbins, 2), g[3][:4]
    for update in range(3):
        tries = rng.integers(0, 14, nbins)
        wins = np.minimum(tries, rng.integers(0, 14, nbins))
        fresh = np.stack([tries, wins], 1).astype(np.int32)
        fresh[(np.arange(nbins) // 9) % 5 == update] = (12, 11)          # runs of nine adjacent bins, all promoted
        fresh[0] = (8, 6)                                                # exactly min_tries, exactly the rate
        w_counts += fresh
        counts.copy_(torch.from_numpy(w_counts))
        b.curriculum_update(cur, levels, cdf, counts, stats)
        before = w_levels.copy()
        CC.curriculum_update_reference(cur, w_levels, w_cdf, w_counts, w_stats)
        for got, want, what in ((levels, w_levels, "levels"), (cdf, w_cdf, "cdf"), (counts, w_counts, "counts"), (stats, w_stats, "stats")):
            _same(got, want, what, update)
        assert (w_levels >= before).all() and (w_levels > before).any() and np.array_equal(w_cdf, np.cumsum(w_levels)) and w_counts[0].tolist() == [0, 0]
    assert w_stats[E.CURR_STAT_UPDATES] == 6 and w_stats[E.CURR_STAT_PROMOTED] > 1 and (nbins == 1 or ((w_counts[:, 0] > 0).any() and (w_levels == 5).any()))
    for t in g:
        assert (t[-4:] == 77).all()


def test_the_binding_and_the_entries_refuse_by_name():
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine as E
    n = 5
    b = _batch(n)
    cur = step_struct()
    I = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    F = lambda *s: torch.full(s, SENTINEL, device="cuda")
    cdf, counts, levels, stats = I(4), I(4, 2), I(4), I(4)
    state, cmd, obs, priv, done = torch.zeros(n, E.CURR_NSTATE, device="cuda"), F(n, 7), F(n, b.nobs), F(n, b.npriv), torch.zeros(n, device="cuda")
    done_p = C.c_void_p(done.data_ptr())
    with pytest.raises(E.OdkError, match="curriculum_step: cmd is not the tensor bound to the batch"):
        b.curriculum_step(cur, priv, done, done, cdf, counts, state, cmd)
    b.bind_commands(cmd)
    try:
        step = lambda **kw: b.curriculum_step(*[kw.get(k, v) for k, v in (("cur", cur), ("priv", priv), ("done", done), ("truncation", done), ("cdf", cdf),
                                                                          ("counts", counts), ("state", state), ("cmd", cmd))], obs=kw.get("obs", obs))
        wide, never = step_struct(), step_struct()
        wide.n[0], never.period = 17, 0
        for kw, message in ((dict(cur=None), "curriculum_step: curriculum: expected an engine.Curriculum"),
                            (dict(cur=wide), r"curriculum_step: curriculum: n\[0\] = 17"),
                            (dict(cur=never), "curriculum_step: period = 0"),
                            (dict(cdf=I(5)), "curriculum_step: cdf: shape"),
                            (dict(cdf=cdf.float()), "curriculum_step: cdf: dtype"),
                            (dict(counts=I(4)), "curriculum_step: counts: shape"),
                            (dict(state=state[:4]), "curriculum_step: state: shape"),
                            (dict(priv=priv.cpu()), "curriculum_step: priv: the tensor must live on cuda"),
                            (dict(obs=obs[:, :50]), "curriculum_step: obs: shape"),
                            (dict(cmd=cmd.clone()), "curriculum_step: cmd is not the tensor bound"),
                            (dict(truncation=None), "curriculum_step: done and truncation come together"),
                            (dict(done=done[:4]), "curriculum_step: done: shape")):
            with pytest.raises(E.OdkError, match=message):
                step(**kw)
        few = step_struct()
        few.min_tries = 0
        for args, message in (((cur, levels, cdf, I(4), stats), "curriculum_update: counts: shape"),
                              ((cur, levels.long(), cdf, counts, stats), "curriculum_update: levels: dtype"),
                              ((cur, levels, cdf, counts, I(3)), "curriculum_update: stats: shape"),
                              ((few, levels, cdf, counts, stats), "curriculum_update: min_tries = 0"),
                              ((wide, levels, cdf, counts, stats), r"curriculum_update: curriculum: n\[0\] = 17")):
            with pytest.raises(E.OdkError, match=message):
                b.curriculum_update(*args)
        # the C entry points' own refusals: every null pointer, the buffer that is not the bound one, the grid, every overlap; nothing launched
        # (one allocation, a slot of 4096 floats per array: what overlaps what is ours to say)
        L = E.load_library()
        big = F(8 * 4096)
        slot = lambda k, off=0: C.c_void_p(big.data_ptr() + 4 * (4096 * k + off))
        counts, state, cmd, obs, priv, cdf, levels, stats = range(8)
        bound = big[4096 * cmd:4096 * cmd + 7 * n].view(n, 7)
        b.bind_commands(bound)
        P, at = slot, slot
        last = lambda: L.odk_last_error().decode()
        full = lambda: [b._b, C.byref(cur), P(priv), done_p, done_p, P(cdf), P(counts), P(state), P(cmd), P(obs), P(priv), None]
        for k, name in ((0, "batch"), (1, "curriculum"), (2, "priv_dev"), (5, "cdf_dev"), (6, "counts_dev"), (7, "state_dev"), (8, "cmd_dev"),
                        (4, "truncation_dev")):
            args = full()
            args[k] = None
            assert L.odk_curriculum_step(*args) == E.ERR_INVALID and f"odk_curriculum_step: null {name}" in last(), name
        args = full()
        args[8] = slot(cmd, 7)
        assert L.odk_curriculum_step(*args) == E.ERR_INVALID and "odk_curriculum_step: cmd_dev is not the command buffer bound to the batch" in last()
        many = step_struct()
        many.n[1] = 0
        args = full(); args[1] = C.byref(many)
        assert L.odk_curriculum_step(*args) == E.ERR_INVALID and "odk_curriculum_step: n[1] = 0" in last()
        args = full(); args[1] = C.byref(wide)
        assert L.odk_curriculum_step(*args) == E.ERR_INVALID and "odk_curriculum_step: n[0] = 17" in last()
        for k, where, message in ((7, at(cmd, 7 * n - 1), "state_dev overlaps cmd_dev"), (9, at(cmd, 1), "cmd_dev overlaps obs_dev"),
                                  (6, at(state, 8 * n - 1), "counts_dev overlaps state_dev"), (10, at(obs, b.nobs * n - 1), "obs_dev overlaps priv_patch_dev"),
                                  (5, at(counts, 7), "counts_dev overlaps cdf_dev"), (2, at(state, 0), "state_dev overlaps priv_dev")):
            args = full()
            args[k] = where
            assert L.odk_curriculum_step(*args) == E.ERR_INVALID and f"odk_curriculum_step: {message}" in last(), message
        ufull = lambda: [b._b, C.byref(cur), P(levels), P(cdf), P(counts), P(stats), None]
        for k, name in ((0, "batch"), (1, "curriculum"), (2, "levels_dev"), (3, "cdf_dev"), (4, "counts_dev"), (5, "stats_dev")):
            args = ufull()
            args[k] = None
            assert L.odk_curriculum_update(*args) == E.ERR_INVALID and f"odk_curriculum_update: null {name}" in last(), name
        for k, where, message in ((3, at(levels, 3), "levels_dev overlaps cdf_dev"), (2, at(counts, 7), "levels_dev overlaps counts_dev"),
                                  (5, at(cdf, 3), "cdf_dev overlaps stats_dev")):
            args = ufull()
            args[k] = where
            assert L.odk_curriculum_update(*args) == E.ERR_INVALID and f"odk_curriculum_update: {message}" in last(), message
        args = ufull(); args[1] = C.byref(few)
        assert L.odk_curriculum_update(*args) == E.ERR_INVALID and "odk_curriculum_update: min_tries = 0" in last()
        torch.cuda.synchronize()
        assert (big == SENTINEL).all()
    finally:
        b.bind_commands(None)


# ---- the curriculum in a rollout
N_R, T_R = 64, 40


def _env(n=N_R, **overrides):
    from open_duck_playground_amd import joystick
    return joystick.Joystick(task="flat_terrain", num_envs=n, config_overrides=overrides or None)


def _net():
    import torch
    from open_duck_playground_amd.ppo.networks import PPONetworks
    torch.manual_seed(0)
    return PPONetworks(101, 212, 14).cuda()


def _curriculum(env, seed=5, **kw):
    from open_duck_playground_amd import command_curriculum as CC
    settings = dict(period=8, skip=2, min_samples=4)
    settings.update(kw)
    spec = CC.curriculum_spec("vx=-0.15:0.222:4,wz=-1.1:1.2:3", None, CC.env_command_ranges(env), CC.table_command_ranges(env), **settings)
    return CC.CommandCurriculum(env, spec, seed=seed)


@pytest.mark.parametrize("faulty, fast", [(False, True), (True, True), (False, False)], ids=["plain", "with_fault_stage", "generic_loop"])
def test_a_rollout_carries_the_curriculums_commands(faulty, fast):
    """The engine path, the engine path through a fault stage, and the generic loop (`engine_path=False`): each is held to the restatement
    replayed on its own record."""
    import torch
    from open_duck_playground_amd import command_curriculum as CC, engine as E, fault_training as FT
    from open_duck_playground_amd.ppo import train as T
    env, net, seed = _env(), _net(), 5
    cur = _curriculum(env, seed)
    stage = None
    if faulty:
        stage = FT.FaultStage(env, FT.fault_spec(FT.parse_train_sensor(["imu_delay=0:3,gyro_bias_y=-0.2:0.2"]), FT.parse_train_actuation(["noise=0.05"])), seed=seed)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    state = env.reset(seed)
    if stage is not None:
        stage.reset()
    cur.reset(state)
    assert env.commands is cur.commands
    first = cur.commands.clone()
    assert torch.equal(state.obs["state"][:, 6:13], first) and torch.equal(state.obs["privileged_state"][:, 6:13], first)
    data, state = T.rollout(env, net, state, T_R, gen, engine_path=fast, faults=stage, curriculum=cur)
    data = {k: v.cpu().numpy() for k, v in data.items()}
    # the restatement replayed on the recorded priv / done / truncation
    nobs = env.batch.nobs
    w_state, w_cmd, w_counts = np.zeros((N_R, E.CURR_NSTATE), np.float32), np.zeros((N_R, 7), np.float32), np.zeros((cur.nbins, 2), np.int32)
    w_cdf = cur.cdf.cpu().numpy()
    CC.curriculum_step_reference(cur.cur, nobs, data["priv"][:, 0].copy(), None, None, w_cdf, w_counts, w_state, w_cmd)
    assert np.array_equal(bits(w_cmd), tbits(first))
    redrawn = 0
    for t in range(T_R):
        for k in ("obs", "priv"):
            assert np.array_equal(bits(data[k][:, t, 6:13]), bits(w_cmd)), f"step {t}: {k} does not show the command in force"
        after = (data["priv"][:, t + 1] if t + 1 < T_R else data["last_priv"]).copy()
        redrawn += CC.curriculum_step_reference(cur.cur, nobs, after, data["done"][:, t], data["truncation"][:, t], w_cdf, w_counts, w_state, w_cmd).sum()
        assert np.array_equal(bits(after[:, 6:13]), bits((data["priv"][:, t + 1] if t + 1 < T_R else data["last_priv"])[:, 6:13])), t
    for got, want, what in ((cur.state, w_state, "state"), (cur.commands, w_cmd, "commands"), (cur.counts, w_counts, "counts")):
        _same(got, want, what, T_R)
    assert redrawn >= N_R * (T_R // 8) and w_counts[:, 0].sum() >= 1, "at least one stint was judged"
    assert np.array_equal(tbits(state.obs["state"][:, 6:13]), bits(w_cmd)) and float(data["done"].sum()) > 0
    lo, hi = np.float32([-0.15, -0.2, -1.1]), np.float32([0.222, 0.2, 1.2])
    assert ((w_cmd[:, :3] >= lo) & (w_cmd[:, :3] <= hi)).all() and (w_cmd[:, 0] != 0).any()
    m = cur.metrics()
    assert m["coverage"] == 0.75 and m["promotions"] == 0      # vx bins 0..2 of 4 (centres -0.1035 .. 0.0825), all three wz bins (-0.717, 0.05, 0.817)


def test_a_tiny_training_run_with_the_curriculum(tmp_path):
    import torch
    from open_duck_playground_amd import engine as E, track
    from open_duck_playground_amd.ppo import train as T
    env = _env(episode_length=30)
    cur = _curriculum(env, seed=0, min_tries=2, tol_lin=10.0, tol_yaw=10.0)      # every stint that does not fall is a success: bins promote
    log = str(tmp_path / "metrics.jsonl")
    net, metrics = T.train(env, num_timesteps=N_R * 20 * 2, seed=0, curriculum=cur, log_path=log, num_minibatches=4, num_updates_per_batch=2,
                           num_evals=2, num_eval_envs=0, tune_gemms=False)
    assert np.isfinite(metrics["training/total_loss"]) and all(torch.isfinite(p).all() for p in net.parameters())
    for k in ("coverage", "mean_level", "promotions"):
        assert f"training/curriculum_{k}" in metrics, k
    rows = [json.loads(l) for l in open(log)]
    assert rows and "training/curriculum_coverage" in rows[-1] and 0.5 <= rows[-1]["training/curriculum_coverage"] <= 1.0
    assert int(cur.stats[E.CURR_STAT_UPDATES]) == 2, "one update per training iteration"
    assert (cur.state[:, E.CURR_HEAD] == 1).all() and (cur.state[:, E.CURR_EPISODE] == 1).all(), "train resets the curriculum after the epoch's reset of the env"
    # the checkpoint carries it, and track reads it
    path = str(tmp_path / "curriculum.pt")
    T.save_checkpoint(path, net, command_curriculum=cur.describe())
    back = track.trained_with_curriculum(path)
    assert back == json.loads(json.dumps(cur.describe())) and back["spec"]["period"] == 8 and np.asarray(back["levels"]).shape == (4, 1, 3)
    assert track.trained_under(path) is None
    plain = str(tmp_path / "plain.pt")
    T.save_checkpoint(plain, net)
    assert track.trained_with_curriculum(plain) is None
