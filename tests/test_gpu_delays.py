"""GPU checks of caller-given action delays (odk_batch_bind_action_delays / Joystick.set_action_delays).  The oracle env has no hook for a
forced delay, so the bound path is held bit for bit to the sampled path, which the rest of the suite holds to the oracle: a step bound to
the delay the sampler drew IS the sampled step; the row picked is the row asked for (motor targets restated in float32 numpy from the
record's own action history); nothing but the delay moves (same random streams); a captured step follows the buffer's contents and
unbinding brings the sampler back; refusals launch nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
OUTPUTS = ("obs", "priv", "reward", "done", "truncation", "metrics")
# (task or robot file, Standing, lanes per env)
CASES = [("flat_terrain", False, 32), ("flat_terrain", False, 64), ("rough_terrain_backlash", False, 0), ("flat_terrain", True, 0),
         ("biped12.xml", False, 0)]


def _model(task):
    from open_duck_playground_amd.model import load_task_model
    if task.endswith(".xml"):
        from test_gpu_env import _xml_model
        return _xml_model(task)
    return load_task_model(task)


def _batch(model, task, standing=False, lanes=0, edit=None, n=N):
    from open_duck_playground_amd import engine
    cfg = engine.default_config(standing)
    if task.endswith(".xml"):
        cfg.use_imitation = 0
    cfg.lanes_per_env = lanes
    cfg.autoreset = 0
    if edit:
        edit(cfg)
    return engine.Batch(model, n, cfg)


def _bits(b):
    """everything a step leaves behind, as int32 bit patterns: the whole record and the six outputs"""
    out = {"records": b.records().view(np.int32)}
    for name in OUTPUTS:
        out[name] = getattr(b, name).cpu().numpy().view(np.int32).reshape(b.nenv, -1)
    return out


def _equal_rows(x, y):
    """[nenv] bool: env e's record and outputs equal bit for bit"""
    ok = np.ones(len(x["records"]), bool)
    for k in x:
        ok &= (x[k] == y[k]).all(axis=1)
    return ok


def _assert_same(x, y, msg):
    for k in x:
        np.testing.assert_array_equal(x[k], y[k], err_msg=f"{msg}: {k}")


def _actions(torch, steps, nu, seed, n=N):
    a = np.random.default_rng(seed).uniform(-1, 1, (steps, n, nu)).astype(np.float32)
    return [torch.tensor(a[t], device="cuda") for t in range(steps)]


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded (the kernel's `key_ctrl + row * action_scale` is one fused multiply-add): the product is
    exact in float64, the sum is taken with its rounding error (TwoSum), and the one case in which rounding the float64 sum again to
    float32 would differ from rounding the exact sum -- the float64 sum sits exactly half way between two float32 values while the exact sum
    does not -- is decided by the sign of that error."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    r = t.astype(np.float32)
    lo = np.where(r.astype(np.float64) > t, np.nextafter(r, np.float32(-np.inf)), r)      # the float32 neighbours around t
    hi = np.where(r.astype(np.float64) < t, np.nextafter(r, np.float32(np.inf)), r)
    tie = (lo != hi) & ((t - lo.astype(np.float64)) == (hi.astype(np.float64) - t)) & (err != 0)
    return np.where(tie, np.where(err > 0, hi, lo), r).astype(np.float32)


def motor_targets(model, cfg, info, rows, prev):
    """step_body's motor targets in float32 from the record's own action history: key_ctrl + action_history[row] * action_scale, through
    the speed-limit clamp around the previous targets when use_motor_speed_limits is on"""
    f = np.float32
    n, nu = len(rows), model.nu
    hist = info["action_history"].reshape(n, 3, nu)
    picked = hist[np.arange(n), rows]
    mt = fma32(picked, f(cfg.action_scale), np.asarray(model.a["key_ctrl"], np.float64).astype(f)[None, :nu])
    if cfg.use_motor_speed_limits:
        # (the clamp's bounds `prev -/+ max_motor_velocity * dt` are one fused multiply-add each in the compiled kernel, as its targets
        # are: with the product rounded first, 1 % of the clamped values are one ulp off -- measured, 9 of 896)
        v, dt = f(cfg.max_motor_velocity), f(cfg.ctrl_dt)
        mt = np.minimum(np.maximum(mt, fma32(-v, dt, prev)), fma32(v, dt, prev))
    return mt.astype(f)


@pytest.mark.parametrize("task,standing,lanes", CASES)
def test_bound_equals_sampled_where_the_draw_agrees(task, standing, lanes):
    """A, B0, B1, B2 and M: one model, one seed, auto-reset off, default noise, the same uniform [-1, 1] actions.  Steps 1..3 run unbound
    everywhere; step 4 is unbound in A, bound to constant 0 / 1 / 2 in B0 / B1 / B2 and to -1 in M.  For every env exactly one of B0, B1,
    B2 equals A in the whole record and every output, bit for bit (the one whose constant is the index the sampler drew); the other two
    differ from A in motor_targets (random actions keep the three history rows apart); each of 0, 1, 2 is the match for some env (64
    independent keys: a missing value has probability 3 * (2/3)^64 < 1e-10); M equals A for every env."""
    import torch
    model = _model(task)
    bs = [_batch(model, task, standing, lanes) for _ in range(5)]
    A, M = bs[0], bs[4]
    if lanes:
        assert A.lanes_per_env == lanes
    acts = _actions(torch, 4, model.nu, seed=11)
    for b in bs:
        b.reset(seed=5)
    for t in range(3):
        for b in bs:
            b.step(acts[t])
    bufs = [torch.full((N,), d, dtype=torch.int32, device="cuda") for d in (0, 1, 2, -1)]
    for b, buf in zip(bs[1:], bufs):
        b.bind_action_delays(buf)
        assert b.action_delays is buf
    for b in bs:
        b.step(acts[3])
    torch.cuda.synchronize()
    ref = _bits(A)
    got = [_bits(b) for b in bs[1:4]]
    match = np.stack([_equal_rows(g, ref) for g in got], axis=1)          # [env, constant]
    print(f"{task} standing={standing} lanes={A.lanes_per_env}: matches per constant {match.sum(0).tolist()}, per env min/max "
          f"{match.sum(1).min()}/{match.sum(1).max()}")
    assert (match.sum(1) == 1).all(), np.flatnonzero(match.sum(1) != 1)
    assert match.any(0).all(), match.sum(0)
    mt_ref = A.info()["motor_targets"].view(np.int32)
    for d in range(3):
        differs = (bs[1 + d].info()["motor_targets"].view(np.int32) != mt_ref).any(axis=1)
        np.testing.assert_array_equal(differs, ~match[:, d], err_msg=f"constant {d}: a batch that is not the sampled step differs in motor_targets")
    _assert_same(_bits(M), ref, "a -1 row is the sampled step")
    for b in bs:
        b.close()


@pytest.mark.parametrize("limits", [False, True])
def test_the_row_picked_is_the_row_asked_for(limits):
    """A per-env mix of 0, 1, 2 bound from the first step on: after each of 5 steps info["motor_targets"] equals, bit for bit,
    key_ctrl + action_history[d] * action_scale restated in float32 numpy from the record's own ring -- with use_motor_speed_limits on,
    through step_body's clamp around the targets of the step before.  Out-of-range rows: 7 behaves as 2 (clamped in the kernel), and any
    negative value behaves as -1, the sampled delay (include/odk.h): -5 gives the unbound step."""
    import torch
    model = _model("flat_terrain")

    def edit(cfg):
        cfg.use_motor_speed_limits = 1 if limits else 0
    b, b7, b2, b5, bu = (_batch(model, "flat_terrain", edit=edit) for _ in range(5))
    rows = (np.arange(N) % 3).astype(np.int32)
    b.bind_action_delays(torch.tensor(rows, device="cuda"))
    b7.bind_action_delays(torch.full((N,), 7, dtype=torch.int32, device="cuda"))
    b2.bind_action_delays(torch.full((N,), 2, dtype=torch.int32, device="cuda"))
    b5.bind_action_delays(torch.full((N,), -5, dtype=torch.int32, device="cuda"))
    all_b = (b, b7, b2, b5, bu)
    for x in all_b:
        x.reset(seed=8)
    acts = _actions(torch, 5, model.nu, seed=12)
    prev = b.info()["motor_targets"].copy()
    for t in range(5):
        for x in all_b:
            x.step(acts[t])
        I = b.info()
        np.testing.assert_array_equal(I["action_history"].reshape(N, 3, model.nu)[:, 0], acts[t].cpu().numpy(), err_msg=f"t={t}: the ring rolls")
        want = motor_targets(model, b.cfg, I, rows, prev)
        got = I["motor_targets"]
        print(f"limits={limits} t={t}: motor_targets differ in {(got.view(np.int32) != want.view(np.int32)).sum()} of {got.size} values, "
              f"worst |diff| {np.abs(got.astype(np.float64) - want).max():.3e}")
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=f"t={t}")
        prev = got.copy()
        _assert_same(_bits(b7), _bits(b2), f"t={t}: a row of 7 is a row of 2")
        _assert_same(_bits(b5), _bits(bu), f"t={t}: a row of -5 is the sampled delay")
    for x in all_b:
        x.close()


@pytest.mark.parametrize("task,standing", [("flat_terrain", False), ("flat_terrain", True), ("biped12.xml", False)])
def test_binding_moves_nothing_but_the_delay(task, standing):
    """Bound (a per-env mix of 0, 1, 2) against unbound over 3 steps, with push_step preset on both sides so that the sampled push fires
    in the second: the rng key and counter, the step counters, the push and the sampled command of every env are equal after every step."""
    import torch
    model = _model(task)
    a, b = _batch(model, task, standing), _batch(model, task, standing)
    b.bind_action_delays(torch.tensor((np.arange(N) % 3).astype(np.int32), device="cuda"))
    for x in (a, b):
        x.reset(seed=6)
        I = x.info()
        I["push_step"][:] = I["push_interval_steps"] - 2
        x.set_records(I["_records"])
    acts = _actions(torch, 3, model.nu, seed=13)
    fired = moved = 0
    for t in range(3):
        a.step(acts[t]); b.step(acts[t])
        Ia, Ib = a.info(), b.info()
        for nm in ("rng", "step", "push_step", "push_interval_steps", "push", "command"):
            np.testing.assert_array_equal(Ia[nm].view(np.int32), Ib[nm].view(np.int32), err_msg=f"t={t} {nm}")
        fired += int((np.hypot(Ia["push"][:, 0], Ia["push"][:, 1]) > 0.5).sum())
        moved += int((Ia["motor_targets"].view(np.int32) != Ib["motor_targets"].view(np.int32)).any(axis=1).sum())
    assert fired >= N and moved > N       # the push fired everywhere, and the binding did change the step
    a.close(); b.close()


def test_a_captured_step_follows_the_buffer_and_unbinding_restores_the_sampler():
    """A: delays bound, one step captured and replayed.  B: a batch of its own with a buffer of its own, stepped eagerly with the same
    contents: the two stay bit for bit equal while the buffer is rewritten between replays, and A's motor targets are those of the rows
    written (the restatement of the test above, speed limits on).  Then A is unbound and compared with a fresh batch that never bound
    and got A's records and state: bit for bit equal over 3 steps."""
    import torch
    from open_duck_playground_amd import engine, joystick
    env = joystick.Joystick(task="flat_terrain", num_envs=N)
    a = env.batch
    model = a.model
    b = engine.Batch(model, N, engine.default_config())
    da = torch.zeros(N, dtype=torch.int32, device="cuda")
    db = torch.zeros(N, dtype=torch.int32, device="cuda")
    env.set_action_delays(da)
    assert env.action_delays is da
    b.bind_action_delays(db)
    env.reset(3); b.reset(seed=3)
    acts = _actions(torch, 9, model.nu, seed=14)
    act = torch.zeros(N, model.nu, device="cuda")
    act.copy_(acts[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.step(act)                                    # warm-up: a real step
    torch.cuda.current_stream().wait_stream(s)
    b.step(acts[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.step(act)
    rng = np.random.default_rng(0)
    seen = set()
    for k in range(5):
        rows = rng.integers(0, 3, N).astype(np.int32) if k != 2 else np.full(N, -1, np.int32)      # one replay of sampled delays among them
        prev = a.info()["motor_targets"].copy()
        da.copy_(torch.tensor(rows)); db.copy_(torch.tensor(rows))      # stream-ordered writes between two replays
        act.copy_(acts[1 + k])
        g.replay()
        b.step(acts[1 + k])
        torch.cuda.synchronize()
        _assert_same(_bits(a), _bits(b), f"replay {k}")
        if k != 2:
            live = a.done.cpu().numpy() == 0           # (a done env's record is the auto-reset's)
            I = a.info()
            want = motor_targets(model, a.cfg, I, rows, prev)
            np.testing.assert_array_equal(I["motor_targets"][live].view(np.int32), want[live].view(np.int32), err_msg=f"replay {k}")
            assert live.sum() > N // 2
            seen.update(rows.tolist())
    assert seen == {0, 1, 2}
    del g
    env.set_action_delays(None)
    assert env.action_delays is None
    c = engine.Batch(model, N, engine.default_config())
    c.reset(seed=3)
    c.set_records(a.records()); c.set_state(*a.get_state())
    for t in range(3):
        a.step(acts[6 + t]); c.step(acts[6 + t])
        torch.cuda.synchronize()
        _assert_same(_bits(a), _bits(c), f"unbound t={t}")
        sa, sc = a.get_state(), c.get_state()
        for j in range(3):
            np.testing.assert_array_equal(sa[j], sc[j], err_msg=f"unbound t={t} state {j}")
    for x in (a, b, c):
        x.close()


def test_refusals_launch_nothing():
    """A float tensor, a CPU tensor, too few rows and a row stride of 0 each raise ValueError (an OdkError too) before any launch; the C
    ABI refuses row_stride 0 and host memory; the binding stays as it was (none) and the batch's records are unchanged."""
    import ctypes as C
    import torch
    from open_duck_playground_amd import engine, joystick
    env = joystick.Joystick(task="flat_terrain", num_envs=N)
    b = env.batch
    L = engine.load_library()
    env.reset(1)
    b.step(torch.zeros(N, 14, device="cuda"))
    torch.cuda.synchronize()
    before = b.records().view(np.int32).copy()
    good = torch.ones(N, dtype=torch.int32, device="cuda")
    bad = [torch.ones(N, device="cuda"), torch.ones(N, dtype=torch.int64, device="cuda"), torch.ones(N, dtype=torch.int32),
           torch.ones(N - 1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda").expand(N),
           torch.ones(N, 0, dtype=torch.int32, device="cuda"), np.ones(N, np.int32)]
    for t in bad:
        with pytest.raises(ValueError) as err:
            env.set_action_delays(t)
        assert isinstance(err.value, engine.OdkError)
        assert env.action_delays is None
    assert L.odk_batch_bind_action_delays(b._b, C.c_void_p(good.data_ptr()), 0) == engine.ERR_INVALID
    assert "row_stride 0 < 1" in L.odk_last_error().decode()
    host = np.ones(N, np.int32)
    assert L.odk_batch_bind_action_delays(b._b, host.ctypes.data_as(C.c_void_p), 1) == engine.ERR_INVALID
    assert "device memory" in L.odk_last_error().decode()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(b.records().view(np.int32), before)
    # nothing is bound: the next step is the sampled one
    c = engine.Batch(b.model, N, engine.default_config())
    c.reset(seed=1)
    c.set_records(b.records()); c.set_state(*b.get_state())
    act = _actions(torch, 1, 14, seed=15)[0]
    b.step(act); c.step(act)
    torch.cuda.synchronize()
    _assert_same(_bits(b), _bits(c), "after the refusals")
    # a wider row is legal: the stride is the tensor's, and only the first entry of a row is read
    wide = torch.full((N + 3, 4), 9, dtype=torch.int32, device="cuda")
    wide[:, 0] = 1
    env.set_action_delays(wide)
    c.bind_action_delays(good)
    b.step(act); c.step(act)
    torch.cuda.synchronize()
    _assert_same(_bits(b), _bits(c), "a wide row")
    b.close(); c.close()
