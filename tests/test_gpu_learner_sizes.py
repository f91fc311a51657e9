"""The learner kernels (csrc/odk_mlp.hip, csrc/odk_learner.hip, ppo/learner.py) against float64 at EVERY robot's network sizes -- the
table of tests/test_learner_sizes_host.py (duck, biped12, tail_biped, biped12_neck, biped_arms; Joystick and Standing) -- and at the
edges of the kernels' blocks and limits.  The float64 references and the inputs are pinned on the host in that file.

Bounds: the whole-network and weight-gradient kernels keep the bounds tests/test_gpu_learner.py asserts at the duck's sizes.  The loss
head, the sampler and the per-tensor gradients are held to four times the error of the float32 torch evaluation of the same formulas on
the same inputs against the same float64 reference (+ a few float32 ulps): `bound_from`.  Every figure is recorded
(profiles/learner_sizes/NOTES.md) before it is asserted."""
import copy

import pytest
import torch

from test_learner_sizes_host import (ENTROPY_COST, EPS, HEAD_A, MAX_A, MAX_IN, MAX_OUT, MIN_PER_CELL, MLP_ROWS, ROBOTS, ErrorLog, bound_from, cell_counts,
                                     check_fused_mlp, gae_reference, guarded, head_inputs, head_reference, head_terms, mlp_float64, mlp_pairs, mlp_params,
                                     rel_max, row, runs_fused, scaled_error, table_rows)

pytestmark = pytest.mark.gpu

HEAD_LOG, GRAD_LOG = ErrorLog("head_errors.json"), ErrorLog("gradient_errors.json")
HEAD_OUTPUTS = ("dloc", "dscale_raw", "dbaseline", "losses")


def _cuda(inp):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}


# ---- 0. refusals: host-side argument checks, nothing is launched ------------------------------------------------------------------

def test_sizes_past_the_limits_are_refused_before_any_launch():
    from open_duck_playground_amd import engine
    z = lambda *s: torch.zeros(*s, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    widths, W, b, flat, table, pf, pb = mlp_params(16, 16, g)
    wf = [table.fwd_view(pf, l) for l in range(4)]
    for n_in, n_out in ((MAX_IN + 1, 16), (16, MAX_OUT + 1)):
        with pytest.raises(engine.OdkError):
            engine.FusedMLP([dict(x=z(8, n_in), wf=wf, b=b, out=z(8, n_out))])
    n, A = 8, MAX_A + 1
    with pytest.raises(engine.OdkError):
        engine.ppo_head(z(n, 2 * A), z(n, A), z(n), z(n), None, z(n), z(n), z(n, A), z(n, 2 * A), z(n), z(4), EPS, ENTROPY_COST)
    with pytest.raises(engine.OdkError):
        engine.policy_sample(z(n, 2 * A), z(n, A))
    from open_duck_playground_amd.ppo import train as T
    for B, Tn, A in ((3, 1707, 2), (1025, 1, 2), (4, 5, MAX_A + 1)):        # B T = 5121; B = 1025; A = 17
        roll = dict(raw_action=z(B, Tn, A), log_prob=z(B, Tn), reward=z(B, Tn), termination=z(B, Tn), truncation=z(B, Tn))
        mk = lambda: engine.GaeHead(z(B * Tn, 2 * A), z(B * Tn + B), roll, z(1, B * Tn, A), torch.zeros(B, dtype=torch.int64, device="cuda"),
                                    torch.zeros(1, dtype=torch.int32, device="cuda"), z(B * Tn, 2 * A), z(B * Tn), z(4), B, Tn, T.ppo_config())
        if A > MAX_A:
            with pytest.raises(engine.OdkError):
                mk()()                                                        # the C entry point's own argument check, in front of its launch
        else:
            with pytest.raises(engine.OdkError):
                mk()


# ---- 1. whole-network kernels -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_in, n_out", mlp_pairs())
def test_fused_mlp_matches_float64_at_every_size(n_in, n_out):
    """`check_fused_mlp` (the body of test_fused_mlp_matches_torch) at every (n_in, n_out) of the table's policy and value networks and at
    the boundary widths -- n_in 5 / 16 / 96 / 224 (small, exact multiples of the 16-column padding, the limit), n_out 1 / 16 / 17 / 32 (the
    output layer's 16-column block edge, the limit: nothing clamped) -- for row counts below one tile, of one tile, with a ragged last
    tile and of whole tiles."""
    for n in MLP_ROWS:
        check_fused_mlp(n, n_in, n_out)


@pytest.mark.parametrize("robot, task", [("biped12", "joystick"), ("biped_arms", "standing"), ("biped12", "standing")])
@pytest.mark.parametrize("rows", [(320, 336), (77, 85), (16, 333)])
def test_two_networks_in_one_launch_at_other_sizes(robot, task, rows):
    """Policy and value side by side in one launch == each alone, bit for bit, and == float64: the block -> (network, tile) map depends on
    both tile counts and on which network is the costly one (value rows = policy rows + B, as in the learner; then a ragged pair, then
    a policy of one tile beside a value network of 21)."""
    from open_duck_playground_amd import engine
    A, obs, priv = row(robot, task)
    g = torch.Generator(device="cuda").manual_seed(obs + rows[0])
    nets, refs = [], []
    for n, n_in, n_out in ((rows[0], obs, 2 * A), (rows[1], priv, 1)):
        widths, W, b, flat, table, pf, pb = mlp_params(n_in, n_out, g)
        x, dout = guarded(n, n_in, g), guarded(n, n_out, g)

        def mk():
            tb = engine.FusedMLP.train_buffers(n, n_in, n_out, "cuda")
            for t in [tb["xp"], tb["doutp"]] + tb["h"] + tb["g"] + tb["dz"] + tb["bias_partial"]:
                t.fill_(float("nan"))
            return dict(x=x, wf=[table.fwd_view(pf, l) for l in range(4)], wb=[table.bwd_view(pb, l) for l in range(4)], b=b,
                        out=torch.full((n, n_out), float("nan"), device="cuda"), dout=dout, **tb)
        nets.append((mk(), mk()))
        refs.append(mlp_float64(x, W, b, dout))
    pair = engine.FusedMLP([nets[0][0], nets[1][0]])
    pair.forward(); pair.backward()
    for k in range(2):
        one = engine.FusedMLP([nets[k][1]])
        one.forward(); one.backward()
        for key in ("h", "g", "dz", "bias_partial"):
            assert all(torch.equal(a, b_) for a, b_ in zip(nets[k][0][key], nets[k][1][key]))
        for key in ("out", "xp", "doutp"):
            assert torch.equal(nets[k][0][key], nets[k][1][key])
        zs, hs, gs, dzs = refs[k]
        n = rows[k]
        assert rel_max(nets[k][0]["out"], zs[3]) < 2e-6
        for l, w in enumerate(engine.MLP_HIDDEN):
            assert rel_max(engine.quad_unpack(nets[k][0]["h"][l], n, w), hs[l + 1]) < 2e-6
            assert rel_max(engine.quad_unpack(nets[k][0]["dz"][l], n, w), dzs[l]) < 3e-6


# ---- 2. weight gradients ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robot, task", [(r, t) for r, t, *_ in table_rows()])
def test_dw_gemm_matches_float64_at_every_rows_layer_shapes(robot, task):
    """odk_dw_gemm + its finishing launch at the six layer shapes of a table row, (512, obs) (512, priv) (256, 512) (128, 256) (2A, 128)
    (1, 128), in one launch as the learner issues them, for 1280 rows and for a ragged 777: == float64 dz^T h to 2e-6 of the tensor's
    max, bit-identical when repeated over a poisoned workspace, nothing outside the layers' ranges touched."""
    from open_duck_playground_amd import engine
    A, obs, priv = row(robot, task)
    g = torch.Generator(device="cuda").manual_seed(obs)
    shapes = [(512, obs), (512, priv), (256, 512), (128, 256), (2 * A, 128), (1, 128)]
    for n, ks in ((1280, 8), (777, 16)):
        tot = sum((o * i + 7) // 4 * 4 for o, i in shapes) + 12
        flat = torch.full((tot,), 7.0, device="cuda")
        ws = torch.empty(ks * engine.DwGemm.workspace_stride(tot), device="cuda").fill_(float("nan"))
        layers, dense, off = [], [], 8
        for o, i in shapes:
            dz, h = torch.randn(n, o, device="cuda", generator=g), torch.randn(n, i, device="cuda", generator=g)
            dense.append((dz, h, off))
            layers.append((engine.quad_pack(dz), engine.quad_pack(h), o, i, off))
            off += (o * i + 7) // 4 * 4
        op = engine.DwGemm(layers, flat, ws, ks)
        op()
        first = flat.clone()
        covered = torch.zeros(tot, dtype=torch.bool, device="cuda")
        for dz, h, o in dense:
            ref = dz.double().t() @ h.double()
            got = flat[o:o + ref.numel()].view_as(ref).double()
            covered[o:o + ref.numel()] = True
            assert float((got - ref).abs().max() / ref.abs().max()) < 2e-6, (n, tuple(ref.shape))
        assert bool((flat[~covered] == 7.0).all())                         # in front, behind, and the padding between the layers
        ws.fill_(float("nan")); op()
        assert torch.equal(flat, first)


# ---- 3. the loss head and the sampler against float64 -------------------------------------------------------------------------------

def _check_head(case, inp, got, r64, r32, S):
    """Every output of the head, every element, against float64, in units of its terms' scale; recorded, then asserted."""
    fails = []
    for k in HEAD_OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), (case, k)
        parts = [(k, slice(None))] if k != "losses" else [(f"{name}_loss", slice(i, i + 1)) for i, name in enumerate(("total", "policy", "value", "entropy"))]
        for name, sl in parts:
            e32, ek = scaled_error(r32[k][sl], r64[k][sl], S[k][sl]), scaled_error(got[k][sl], r64[k][sl], S[k][sl])
            bound = bound_from(e32)
            HEAD_LOG.rec(case, name, e32, ek, bound)
            if not ek <= bound:
                fails.append((name, ek, bound))
    HEAD_LOG.dump()
    assert not fails, (case, fails)


@pytest.mark.parametrize("kind", ["random", "crafted"])
@pytest.mark.parametrize("n", [640, 77, 1000])                       # a multiple of the 16 samples per wave / 64 per workgroup, and two that are not
@pytest.mark.parametrize("A", HEAD_A)
def test_ppo_head_matches_float64(A, n, kind):
    """`engine.ppo_head` == `head_reference` in float64: dloc, dscale_raw, dbaseline for every sample and lane, the four loss sums.  The
    crafted set holds saturated actions (|a| up to 8), raw_scale from -15 (scale -> 0.001) to 30 (the branch above 20) and target ratios
    0.5 ... 2.0 with both advantage signs, so the gradient's choice by clip region and sign (`dmin_drho`) is exercised in all six cells;
    no sample is excluded (the host test shows float32 keeps every sample in its cell)."""
    from open_duck_playground_amd import engine
    inp = head_inputs(A, n, kind)
    r64, r32 = head_reference(inp), head_reference(inp, torch.float32, eager=True)
    _, S = head_terms(inp)
    assert min(cell_counts(r64["cell"])) >= MIN_PER_CELL(n)
    d = _cuda(inp)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    dlogits, dbase, losses = nan(n, 2 * A), nan(n), torch.zeros(4, device="cuda")
    engine.ppo_head(d["logits"], d["raw_action"], d["old_logp"], d["adv"], None, d["vs"], d["baseline"], d["noise"], dlogits, dbase, losses, EPS, ENTROPY_COST)
    got = dict(dloc=dlogits[:, :A], dscale_raw=dlogits[:, A:], dbaseline=dbase, losses=losses)
    _check_head(f"ppo_head/{kind}/A={A}/n={n}", inp, got, r64, r32, S)
    # the advantage normalisation on the device (`stats`: mean, 1 / (std + 1e-8)) and grad_scale
    raw_adv = (3.0 * d["adv"] + 0.5).contiguous()
    stats = torch.tensor([0.5, 1.0 / 3.0], device="cuda")
    inp2 = dict(inp, adv=((raw_adv.double() - stats[0].double()) * stats[1].double()).cpu())
    r64b, r32b = head_reference(inp2), head_reference(inp2, torch.float32, eager=True)
    assert torch.equal(r64b["cell"], r64["cell"])
    dlogits.fill_(float("nan")); dbase.fill_(float("nan")); losses.zero_()
    engine.ppo_head(d["logits"], d["raw_action"], d["old_logp"], raw_adv, stats, d["vs"], d["baseline"], d["noise"], dlogits, dbase, losses, EPS, ENTROPY_COST, 0.5)
    got = dict(dloc=2 * dlogits[:, :A], dscale_raw=2 * dlogits[:, A:], dbaseline=2 * dbase, losses=losses)
    _check_head(f"ppo_head+stats/{kind}/A={A}/n={n}", inp2, got, r64b, r32b, head_terms(inp2)[1])


@pytest.mark.parametrize("kind", ["random", "crafted"])
@pytest.mark.parametrize("B, Tn", [(16, 20), (37, 5), (256, 20), (3, 7)])       # B T = 320, 185, 5120, 21: whole and ragged 32-sample workgroups, the LDS limit
@pytest.mark.parametrize("A", HEAD_A)
def test_fused_gae_head_matches_float64(A, B, Tn, kind):
    """`engine.GaeHead` (GAE + advantage statistics + loss head in one launch, rollout rows through the schedule's trajectory indices,
    noise from the pool slot under the cursor) against float64: adv / vs / stats against `gae_reference` on doubles, the head's
    gradients and loss sums against `head_reference` fed the advantage the launch itself reports (every workgroup redoes the recursion in
    its own LDS, only the first writes adv_out: a workgroup whose recursion went wrong shows in its samples' gradients)."""
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.ppo import train as T
    n, n_traj, steps, cur = B * Tn, B + 3, 3, 1
    cfg = T.ppo_config()
    g = torch.Generator().manual_seed(B + A)
    rew, val, boot = torch.randn(B, Tn, generator=g), torch.randn(B, Tn, generator=g), torch.randn(B, generator=g)
    term = (torch.rand(B, Tn, generator=g) < 0.1).float()
    trunc = (torch.rand(B, Tn, generator=g) < 0.05).float() * (1 - term)
    vs64, adv64 = gae_reference(trunc, term, rew, val, boot, cfg["gae_lambda"], cfg["discounting"])
    vs32, adv32 = gae_reference(trunc, term, rew, val, boot, cfg["gae_lambda"], cfg["discounting"], torch.float32)
    inp = head_inputs(A, n, kind, seed=7)
    # the minibatch's trajectories sit at shuffled places of a larger rollout; the schedule's slice under the cursor names them
    perm = torch.randperm(n_traj, generator=g)
    sched = torch.stack([torch.randperm(n_traj, generator=g)[:B] for _ in range(steps)])
    sched[cur] = perm[:B]
    place = lambda t: torch.full((n_traj,) + t.shape[1:], float("nan")).index_copy_(0, perm[:B], t)
    roll = {k: place(v).cuda() for k, v in dict(raw_action=inp["raw_action"].view(B, Tn, A), log_prob=inp["old_logp"].view(B, Tn), reward=rew, termination=term,
                                                 truncation=trunc).items()}
    pool = torch.full((steps, n, A), float("nan")); pool[cur] = inp["noise"]
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    dlogits, dvalues, adv_o, vs_o, stats_o = nan(n, 2 * A), nan(n + B), nan(n), nan(n), nan(2)
    parts = nan((n + engine.GAE_HEAD_SAMPLES - 1) // engine.GAE_HEAD_SAMPLES, 4)
    values = torch.cat([val.reshape(-1), boot]).cuda()
    for normalize in (True, False):
        c = dict(cfg, normalize_advantage=normalize)
        op = engine.GaeHead(inp["logits"].cuda(), values, roll, pool.cuda(), sched.reshape(-1).cuda().contiguous(), torch.tensor([cur], dtype=torch.int32, device="cuda"),
                            dlogits, dvalues, torch.zeros(4, device="cuda"), B, Tn, c, adv=adv_o, vs=vs_o, stats=stats_o, loss_partials=parts)
        op()
        case = f"gae_head/{kind}/A={A}/B={B}/T={Tn}/norm={int(normalize)}"
        # GAE: absolute errors in units of the largest |vs| (the recursion's running sum), statistics relative
        sc = float(vs64.abs().max())
        fails = []
        mean64, std64 = adv64.mean(), adv64.std(unbiased=False)
        mean32, std32 = adv32.mean(), adv32.std(unbiased=False)
        for name, got_, r32_, r64_, s_ in (("adv", adv_o.view(B, Tn), adv32, adv64, sc), ("vs", vs_o.view(B, Tn), vs32, vs64, sc),
                                            ("adv_mean", stats_o[0], mean32, mean64, sc), ("adv_rstd", stats_o[1], 1 / (std32 + 1e-8), 1 / (std64 + 1e-8), float(1 / std64))):
            e32, ek = scaled_error(r32_, r64_, torch.tensor(s_)), scaled_error(got_, r64_, torch.tensor(s_))
            bound = bound_from(e32)
            HEAD_LOG.rec(case, name, e32, ek, bound)
            if not ek <= bound:
                fails.append((name, ek, bound))
        HEAD_LOG.dump()
        assert not fails, (case, fails)
        # the head, on the advantage the launch reports
        advn = adv_o.double().cpu()
        if normalize:
            advn = (advn - stats_o[0].double().cpu()) * stats_o[1].double().cpu()
        inp_k = dict(inp, adv=advn, vs=vs_o.double().cpu(), baseline=val.reshape(-1))
        r64, r32 = head_reference(inp_k), head_reference(inp_k, torch.float32, eager=True)
        if n >= 150:
            assert min(cell_counts(r64["cell"])) >= 1, cell_counts(r64["cell"])
        got = dict(dloc=dlogits[:, :A], dscale_raw=dlogits[:, A:], dbaseline=dvalues[:n], losses=parts.sum(0))
        _check_head(case, inp_k, got, r64, r32, head_terms(inp_k)[1])
        assert bool(torch.isnan(dvalues[n:]).all())                          # the bootstrap rows get no gradient from this launch
        dlogits.fill_(float("nan")); dvalues.fill_(float("nan")); parts.fill_(float("nan"))


@pytest.mark.parametrize("kind", ["random", "crafted"])
@pytest.mark.parametrize("A", HEAD_A)
def test_policy_sample_matches_float64(A, kind):
    """`engine.policy_sample` == float64: raw = loc + scale z, action = tanh(raw), log-prob of raw (bounded in units of the sum of its
    terms' magnitudes, which grows with |raw|: the result cancels, the rounding does not)."""
    from open_duck_playground_amd import engine
    for n in (1000, 64):
        inp = head_inputs(A, n, kind, seed=3)
        logits, z = inp["logits"], inp["noise"]
        out = {}
        for dtype in (torch.float64, torch.float32):
            loc, rs = logits[:, :A].to(dtype), logits[:, A:].to(dtype)
            scale = torch.nn.functional.softplus(rs) + 0.001 if dtype == torch.float32 else torch.logaddexp(rs, torch.zeros_like(rs)) + 0.001
            raw = loc + scale * z.to(dtype)
            out[dtype] = (raw, torch.tanh(raw), scale)
        raw64, act64, scale64 = out[torch.float64]
        # the density of each evaluation's OWN float32 raw action against float64 at that same action (raw actions that differ by a rounding
        # have densities that differ by that rounding / scale: not an error of either evaluation)
        raw_k, act_k, logp_k = engine.policy_sample(logits.cuda(), z.cuda())
        fails = []
        case = f"policy_sample/{kind}/A={A}/n={n}"
        S_raw = logits[:, :A].double().abs() + (scale64 * z.double()).abs()
        S_act = act64.abs() + S_raw * (1 - act64 ** 2)                          # tanh's own rounding + the raw action's, through tanh'
        checks = [("raw", raw_k, out[torch.float32][0], raw64, S_raw), ("action", act_k, out[torch.float32][1], act64, S_act)]
        err = {}
        for who, raw_own, logp_own in (("kernel", raw_k.cpu(), logp_k), ("torch", out[torch.float32][0], None)):
            q = dict(inp, raw_action=raw_own, old_logp=torch.zeros(n), adv=torch.ones(n), vs=torch.zeros(n), baseline=torch.zeros(n))
            ref, S = head_reference(q)["logp"], head_terms(q)[1]["logp"]
            err[who] = scaled_error(head_reference(q, torch.float32, eager=True)["logp"] if logp_own is None else logp_own, ref, S)
        e32, ek = err["torch"], err["kernel"]
        bound = bound_from(e32)
        HEAD_LOG.rec(case, "logp", e32, ek, bound)
        if not ek <= bound:
            fails.append(("logp", ek, bound))
        for name, got_, r32_, r64_, S_ in checks:
            assert bool(torch.isfinite(got_).all())
            e32, ek = scaled_error(r32_, r64_, S_), scaled_error(got_, r64_, S_)
            bound = bound_from(e32)
            HEAD_LOG.rec(case, name, e32, ek, bound)
            if not ek <= bound:
                fails.append((name, ek, bound))
        HEAD_LOG.dump()
        assert not fails, (case, fails)


# ---- 4. the assembled learner step, per parameter tensor ----------------------------------------------------------------------------

def _fake_rollout(N, T, dev, obs, priv, A, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    done = (torch.rand(N, T, device=dev, generator=g) < 0.08).float()
    trunc = (torch.rand(N, T, device=dev, generator=g) < 0.5).float() * done
    return dict(obs=r(N, T, obs), priv=r(N, T, priv), raw_action=0.7 * r(N, T, A), log_prob=-12 + r(N, T), reward=0.05 * r(N, T).abs(),
                done=done, truncation=trunc, last_priv=r(N, priv))


LEARNER_ROWS = [("duck", "joystick"), ("biped12", "joystick"), ("tail_biped", "joystick"), ("biped_arms", "standing"), ("biped_arms", "joystick")]


@pytest.mark.parametrize("robot, task", LEARNER_ROWS)
@pytest.mark.parametrize("normalize_advantage, N, fused", [(True, 64, True), (False, 64, True), (True, 1024, True), (True, 64, False), (True, 64, None)])
def test_flat_learner_gradients_match_float64_autograd_per_tensor(robot, task, normalize_advantage, N, fused, monkeypatch):
    """test_flat_learner_gradients_match_autograd at the table's sizes, against autograd of `ppo_loss` in FLOAT64 (a double copy of the
    networks on double data), PER PARAMETER TENSOR: max |g - g_ref| over the tensor relative to the tensor's own max |g_ref| -- each weight
    and bias of both networks -- bounded by four times the error of the float32 autograd path (the eager learner) for that tensor, plus
    the global 2e-4 of the older test.  Which path runs is asserted: the whole-network kernels for rows whose input widths are within 224
    AND whose action dimension is even; the library path for Joystick biped_arms (230 privileged observations) and for tail_biped
    (A = 15: the value network's weights start 2 A floats behind a multiple of 4, `_FlatMLP.fused_ok`)."""
    from open_duck_playground_amd.ppo import learner as LM
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.learner import FlatLearner, prepare_rollout
    from open_duck_playground_amd.ppo.networks import PPONetworks
    A, obs, priv = row(robot, task)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    if fused is False:
        monkeypatch.setattr(LM, "_FUSED_MLP", False)
    net = (PPONetworks(obs, priv, A) if fused is not None else PPONetworks(obs, priv, A, policy_hidden=(256, 128), value_hidden=(256, 256, 64))).to(dev)
    cfg = T.ppo_config(); cfg["normalize_advantage"] = normalize_advantage
    Tn, nmb = 20, 4
    data = _fake_rollout(N, Tn, dev, obs, priv, A)
    net.norm_obs.update(data["obs"]); net.norm_priv.update(data["priv"])
    ref32 = copy.deepcopy(net)
    ref64 = copy.deepcopy(net).double()
    lr = FlatLearner(net, cfg, N // nmb, Tn, use_graph=False)
    idx = torch.arange(3, 3 + N // nmb, device=dev)
    lr.load_minibatch(prepare_rollout(net, data, cfg), idx)
    assert (lr.fused is not None) == (fused is True and runs_fused(A, obs, priv))
    assert (robot, task, runs_fused(A, obs, priv)) in [("duck", "joystick", True), ("biped12", "joystick", True), ("tail_biped", "joystick", False),
                                                      ("biped_arms", "standing", True), ("biped_arms", "joystick", False)]
    lr._draw_noise(); lr._loss_and_grads()
    mb = {k: v[idx] for k, v in data.items()}
    mb["noise"] = lr.noise.view(N // nmb, Tn, A).clone()
    loss32, met32 = T.ppo_loss(ref32, mb, cfg)
    loss32.backward()
    loss64, met64 = T.ppo_loss(ref64, {k: v.double() for k, v in mb.items()}, cfg)
    loss64.backward()
    got = lr.last_step_losses()
    for k, want in enumerate((loss64.detach(), met64["policy_loss"], met64["v_loss"], met64["entropy_loss"])):
        torch.testing.assert_close(got[k].double(), want, rtol=2e-4, atol=1e-6)
    params = lambda m: list(m.policy.named_parameters(prefix="policy")) + list(m.value.named_parameters(prefix="value"))
    flat_ref = torch.cat([p.grad.reshape(-1) for _, p in params(ref64)])
    case = f"{robot}/{task}/norm={int(normalize_advantage)}/N={N}/fused={fused}"
    fails, off = [], 0
    for (name, p64), (_, p32) in zip(params(ref64), params(ref32)):
        k = p64.numel()
        g = lr.flat_g[off:off + k].view_as(p64).double()
        off += k
        top = p64.grad.abs().max().clamp_min(1e-300)
        e32, ek = float((p32.grad.double() - p64.grad).abs().max() / top), float((g - p64.grad).abs().max() / top)
        bound = bound_from(e32)
        GRAD_LOG.rec(case, name, e32, ek, bound)
        if not ek <= bound:
            fails.append((name, ek, bound))
    assert off == lr.flat_g.numel()
    err = float((lr.flat_g.double() - flat_ref).abs().max() / flat_ref.abs().max())
    GRAD_LOG.rec(case, "all (flat)", float((torch.cat([p.grad.reshape(-1) for _, p in params(ref32)]).double() - flat_ref).abs().max() / flat_ref.abs().max()), err, 2e-4)
    GRAD_LOG.dump()
    assert err < 2e-4, err
    assert not fails, (case, fails)


def test_indexed_step_equals_the_gathered_step_at_sixteen_actions(monkeypatch):
    """Four steps of the indexed, graph-captured learner at Standing biped_arms sizes (A = 16: no idle lane in a sample's row; 95 / 169
    inputs) == the same steps on the gathered path, bit for bit: the cursor, the noise pool's slot and the forward launch's row indices
    all index with A and n_in."""
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.learner import FlatLearner, prepare_rollout
    from open_duck_playground_amd.ppo.networks import PPONetworks
    A, obs, priv = row("biped_arms", "standing")
    dev = torch.device("cuda")
    cfg = T.ppo_config(); cfg.update(num_minibatches=4, num_updates_per_batch=1, tune_gemms=False)
    N, Tn = 64, 20
    data = _fake_rollout(N, Tn, dev, obs, priv, A, seed=9)
    nets, lrs = [], []
    for max_rows in (FlatLearner.INDEXED_MAX_ROWS, 0):              # the indexed form, then (no minibatch within the limit) the gathered one
        monkeypatch.setattr(FlatLearner, "INDEXED_MAX_ROWS", max_rows)
        torch.manual_seed(4)
        n = PPONetworks(obs, priv, A).to(dev)
        n.norm_obs.update(data["obs"]); n.norm_priv.update(data["priv"])
        nets.append(n)
        lrs.append(FlatLearner(n, cfg, N // 4, Tn, use_graph=True))
    a, b = lrs
    assert a.indexed and not b.indexed and a.gae_head is not None and a.fused is not None and b.fused is not None
    perms = torch.randperm(N, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    a.load_rollout_from(nets[0], data, cfg)
    a.set_schedule(perms)
    prep = prepare_rollout(nets[1], data, cfg)
    for k in range(4):
        b.load_minibatch(prep, perms[k * 16:(k + 1) * 16].contiguous())
        b.noise.copy_(a.noise)
        a.step(); b.step()
        assert torch.equal(a.flat_g, b.flat_g), k
        assert torch.equal(a.adv, b.adv) and torch.equal(a.vs, b.vs) and torch.equal(a.stats, b.stats), k
        assert torch.equal(a.flat_p, b.flat_p), k
    assert int(a.cursor) == 4 and float(a.acc[1]) == 4.0 and bool(torch.isfinite(a.flat_p).all())
    torch.testing.assert_close(a.losses, b.losses, rtol=1e-5, atol=1e-6)      # (sums of float atomics: order differs)


def test_batches_report_the_tables_sizes():
    """`Batch.nobs` / `Batch.npriv` of a robot that is not the duck == its table row, on both tasks."""
    import os
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model
    from test_learner_sizes_host import ASSETS
    for robot in ("biped12", "biped_arms"):
        m = Model.from_xml(os.path.join(ASSETS, ROBOTS[robot][0]))
        for kind, task in enumerate(("joystick", "standing")):
            batch = engine.Batch(m, 32, engine.default_config(standing=bool(kind)), device=0)
            try:
                assert (int(m.nu), batch.nobs, batch.npriv) == row(robot, task)
            finally:
                batch.close()
