"""The learner's network sizes per robot and task, and the float64 reference of the PPO loss head that the GPU tests of
tests/test_gpu_learner_sizes.py hold the kernels to -- both pinned here, without a GPU:

* `ROBOTS` against the compiled models (`engine.model_obs_sizes`, what the envs size their networks with);
* `head_reference` (the loss head restated in plain double-precision torch, gradients by autograd) against `ppo.train.ppo_loss`
  in float64 on a tiny network, and against its own closed-form gradients (`head_terms`);
* the crafted head inputs: every sample lands in the same (clip region x advantage sign) cell in float32 and in float64.

The helpers of the whole-network kernel tests (`mlp_params`, `packed_reference`, `check_fused_mlp`) live here as well, so that
tests/test_gpu_learner.py and tests/test_gpu_learner_sizes.py run one body."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")

# robot -> (model: task name or xml under tests/assets, action dimension A, Joystick (obs, priv), Standing (obs, priv)).
# obs = 17 + 6 nu, priv = obs + 69 + 3 nu (Joystick); obs = 15 + 5 nu, priv = obs + 26 + 3 nu (Standing).
# biped12_neck has the duck's actuator count and therefore the duck's sizes; it has no compiled kernel shape in a plain build (tools/new_shape.py
# --add generates one), so the host test below reads its actuator count from the xml and applies the formulas.
ROBOTS = {
    "duck": ("flat_terrain", 14, (101, 212), (85, 153)),
    "biped12": ("biped12.xml", 12, (89, 194), (75, 137)),
    "tail_biped": ("tail_biped.xml", 15, (107, 221), (90, 161)),
    "biped12_neck": ("biped12_neck.xml", 14, (101, 212), (85, 153)),
    "biped_arms": ("biped_arms.xml", 16, (113, 230), (95, 169)),
}
TASKS = ("joystick", "standing")
MAX_IN, MAX_OUT, MAX_A = 224, 32, 16            # ODK_MLP_MAX_IN, NOUT_MAX of csrc/odk_mlp.hip; lanes of a sample's row in csrc/odk_learner.hip
# widths that belong to no robot: the edges of the kernels' blocks and limits
BOUNDARY_N_IN = (5, 16, 96, 224)
BOUNDARY_N_OUT = (1, 16, 17, 32)
BOUNDARY_A = (1, 16)
HEAD_A = (1, 12, 14, 15, 16)
MLP_ROWS = (5, 16, 77, 320)                     # fewer rows than one 16-row tile, one whole tile, a ragged last tile, whole tiles


def table_rows():
    """(robot, task, A, obs, priv) of every cell of the table."""
    return [(r, t, v[1], *v[2 + k]) for r, v in ROBOTS.items() for k, t in enumerate(TASKS)]


def row(robot, task):
    v = ROBOTS[robot]
    return (v[1],) + tuple(v[2 + TASKS.index(task)])


def mlp_pairs():
    """Distinct (n_in, n_out) of the table's policy and value networks that the whole-network kernels take, then the boundary pairs."""
    pairs = []
    for _, _, A, obs, priv in table_rows():
        for p in ((obs, 2 * A), (priv, 1)):
            if p[0] <= MAX_IN and p not in pairs:
                pairs.append(p)
    return pairs + [(i, o) for i in BOUNDARY_N_IN for o in BOUNDARY_N_OUT if (i, o) not in pairs]


def runs_fused(A, obs, priv):
    """Whether `FlatLearner` trains this row on the whole-network kernels (csrc/odk_mlp.hip) or on the library path.  Two conditions
    (`_FlatMLP.fused_ok`): both input widths within ODK_MLP_MAX_IN, and every weight at a flat offset that is a multiple of 4 -- the
    value network sits behind the policy's last bias (2 A floats), so an ODD action dimension (tail_biped, A = 15) takes the library path too."""
    return obs <= MAX_IN and priv <= MAX_IN and 2 * A <= MAX_OUT and (2 * A) % 4 == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the loss head in double precision

LOG2, HALF_LOG_2PI = math.log(2.0), 0.5 * math.log(2.0 * math.pi)


def _softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))          # exact at every x (F.softplus switches to the identity above 20)


def _ldj(x):
    return 2.0 * (LOG2 - x - _softplus(-2.0 * x))           # log |d tanh(x) / dx|


def head_reference(inp, dtype=torch.float64, eager=False):
    """brax `compute_ppo_loss`'s head on n samples as a function of the network outputs: tanh-normal log-prob of the taken raw action,
    clipped surrogate, value loss, sampled entropy; total = policy + value + entropy loss, each a mean over the samples.
    inp: logits [n, 2A] = (loc | raw_scale), raw_action [n, A], old_logp [n], adv [n] (already normalised), vs [n], baseline [n],
    noise [n, A], eps, entropy_cost.  Everything is cast to `dtype` first; gradients w.r.t. logits and baseline by autograd.
    `eager`: the project's own torch functions (`tanh_normal_log_prob`, `tanh_normal_entropy`, F.softplus) in place of the restatement --
    in float32 that is the arithmetic of the CPU / autograd path, the yardstick of the kernels' error.
    Checked in this file against `ppo.train.ppo_loss` in float64 (losses to 1e-12, parameter gradients of a small network to 1e-10) and
    against the closed-form gradients of `head_terms`."""
    c = lambda k: inp[k].detach().to(dtype)
    logits, base = c("logits").requires_grad_(True), c("baseline").requires_grad_(True)
    A = logits.shape[1] // 2
    loc, rs = logits[:, :A], logits[:, A:]
    a, z, old, adv, vs = c("raw_action"), c("noise"), c("old_logp"), c("adv"), c("vs")
    eps, ec = float(inp["eps"]), float(inp["entropy_cost"])
    if eager:
        from open_duck_playground_amd.ppo.networks import tanh_normal_entropy, tanh_normal_log_prob
        scale = F.softplus(rs) + 0.001
        logp = tanh_normal_log_prob(loc, scale, a)
        ent = tanh_normal_entropy(loc, scale, loc + scale * z)
    else:
        scale = _softplus(rs) + 0.001
        u = (a - loc) / scale
        logp = (-0.5 * u * u - torch.log(scale) - HALF_LOG_2PI - _ldj(a)).sum(-1)
        ent = (0.5 + HALF_LOG_2PI + torch.log(scale) + _ldj(loc + scale * z)).sum(-1)
    rho = torch.exp(logp - old)
    policy = -torch.min(rho * adv, rho.clamp(1 - eps, 1 + eps) * adv).mean()
    value = 0.25 * ((vs - base) ** 2).mean()
    entropy = -ec * ent.mean()
    total = policy + value + entropy
    total.backward()
    region = (rho.detach() > 1 + eps).long() - (rho.detach() < 1 - eps).long()              # -1 below, 0 inside, +1 above the clip range
    return dict(dloc=logits.grad[:, :A], dscale_raw=logits.grad[:, A:], dbaseline=base.grad, logp=logp.detach(), rho=rho.detach(),
                losses=torch.stack([total, policy, value, entropy]).detach(), cell=3 * (adv > 0).long() + region + 1)


def head_terms(inp):
    """Float64 closed forms of the same head: the gradients (a second derivation, compared with autograd in this file) and, per output
    element, the SUM OF THE MAGNITUDES of the terms that are added up to give it -- the scale a float32 evaluation's rounding error is
    proportional to (the result itself may cancel).  d log|tanh'(x)| / dx = -2 tanh(x) counts as a term of size 2: autograd forms it as
    2 (2 sigmoid(-2x) - 1)."""
    d = lambda k: inp[k].detach().double()
    logits, base, a, z, old, adv, vs = d("logits"), d("baseline"), d("raw_action"), d("noise"), d("old_logp"), d("adv"), d("vs")
    eps, ec = float(inp["eps"]), float(inp["entropy_cost"])
    n, A = a.shape
    loc, rs = logits[:, :A], logits[:, A:]
    scale = _softplus(rs) + 0.001
    u = (a - loc) / scale
    lp_terms = [0.5 * u * u, torch.log(scale), torch.full_like(u, HALF_LOG_2PI), 2 * LOG2 + 0 * u, 2 * a, 2 * _softplus(-2 * a)]
    logp = (-0.5 * u * u - torch.log(scale) - HALF_LOG_2PI - _ldj(a)).sum(-1)
    x = loc + scale * z
    ent_terms = [torch.full_like(u, 0.5 + HALF_LOG_2PI), torch.log(scale), 2 * LOG2 + 0 * u, 2 * x, 2 * _softplus(-2 * x)]
    ent = (0.5 + HALF_LOG_2PI + torch.log(scale) + _ldj(x)).sum(-1)
    rho = torch.exp(logp - old)
    inside = (rho >= 1 - eps) & (rho <= 1 + eps)
    s1, s2 = rho * adv, rho.clamp(1 - eps, 1 + eps) * adv
    dmin = torch.where(inside | (s1 < s2), adv, torch.zeros_like(adv))
    dl = (-dmin * rho / n)[:, None]
    ce, th, sg = -ec / n, torch.tanh(x), torch.sigmoid(rs)
    g = dict(dloc=dl * u / scale + ce * (-2 * th), dscale_raw=(dl * (u * u - 1) / scale + ce * (1 / scale - 2 * th * z)) * sg,
             dbaseline=-0.5 * (vs - base) / n)
    S_lp, S_ent = sum(t.abs() for t in lp_terms).sum(-1), sum(t.abs() for t in ent_terms).sum(-1)
    # the ratio rho = exp(logp - old_logp) carries the log-prob's ABSOLUTE rounding error (in units of S_lp) as a RELATIVE error: whatever
    # is proportional to rho -- the surrogate inside the clip range and the gradients through it -- has the scale |term| (1 + S_lp)
    amp = (1 + S_lp)[:, None]                                 # (u^2 - 1 is a sum of the terms u^2 and 1)
    S = dict(logp=S_lp, dloc=(dl * u / scale).abs() * amp + abs(ce) * 2,
             dscale_raw=((dl * (u * u + 1) / scale).abs() * amp + abs(ce) * (1 / scale + 2 * z.abs())) * sg,
             dbaseline=0.5 * (vs.abs() + base.abs()) / n)
    S_l = torch.stack([(torch.minimum(s1, s2).abs() + (dmin * rho).abs() * S_lp).sum() / n, 0.25 * ((vs - base) ** 2).sum() / n, ec * S_ent.sum() / n])
    S["losses"] = torch.cat([S_l.sum()[None], S_l])
    return g, S


def gae_reference(trunc, term, rew, values, boot, lambda_, discount, dtype=torch.float64):
    """`ppo.train.compute_gae` (dtype-agnostic: plain torch ops) on [B, T] tensors cast to `dtype` -> (vs, adv) as [B, T]."""
    from open_duck_playground_amd.ppo import train as T
    tm = lambda x: x.to(dtype).transpose(0, 1)
    vs, adv = T.compute_gae(tm(trunc), tm(term), tm(rew), tm(values), boot.to(dtype), lambda_, discount)
    return vs.transpose(0, 1).contiguous(), adv.transpose(0, 1).contiguous()


RAW_SCALES = (-15.0, -5.0, 0.0, 5.0, 19.9, 20.1, 30.0)      # scale -> 0.001 ... the softplus branch above 20
RHO_TARGETS = (0.5, 0.9, 1.0, 1.1, 2.0)
EPS, ENTROPY_COST = 0.2, 0.005                              # ppo_config(): clipping_epsilon, entropy_cost
EDGE_MARGIN = 1e-3


def _old_logp_for(inp, rho_star):
    """old_logp (float32) such that the float64 ratio of the float32 inputs is rho_star up to old_logp's own rounding."""
    tmp = dict(inp, old_logp=torch.zeros_like(rho_star), adv=torch.ones_like(rho_star), vs=torch.zeros_like(rho_star), baseline=torch.zeros_like(rho_star))
    return (head_reference(tmp)["logp"] - torch.log(rho_star.double())).float()


def head_inputs(A, n, kind, seed=0, adv=None):
    """Inputs of the loss head on the CPU (float32; move them to the device as they are).
    kind "random": 2 randn logits as in the older tests, raw actions drawn from that policy (as a rollout does), ratios exp(0.25 randn).
    kind "crafted": raw actions out to |a| = 8 (the first two samples AT +-8), raw_scale cycling through RAW_SCALES, the mean placed
    within three standard deviations of the action (so that exp() of the log-ratio stays finite in float32), target ratios cycling
    through RHO_TARGETS, both advantage signs: sample i has target i % 5 and sign (i // 5) % 2, so all six (clip region x sign) cells
    occur every ten samples.
    Every target ratio keeps EDGE_MARGIN from 1 +- eps.  `adv`: advantages from elsewhere (the fused launch computes its own)."""
    g = torch.Generator().manual_seed(1000 * A + n + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    i = torch.arange(n)
    if kind == "random":
        logits, z = 2.0 * r(n, 2 * A), r(n, A)
        a = logits[:, :A] + (F.softplus(logits[:, A:]) + 0.001) * r(n, A)          # an action the policy itself sampled, as in a rollout
        rho_star = torch.exp(0.25 * r(n))
        for edge in (1 - EPS, 1 + EPS):
            near = (rho_star - edge).abs() < 2 * EDGE_MARGIN
            rho_star = torch.where(near, rho_star + 4 * EDGE_MARGIN, rho_star)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    else:
        a = torch.empty(n, A).uniform_(-8.0, 8.0, generator=g)
        a[0], a[1 % n] = 8.0, -8.0
        rs = torch.tensor(RAW_SCALES)[(i[:, None] * A + torch.arange(A)[None]) % len(RAW_SCALES)]
        scale = (_softplus(rs.double()) + 0.001)
        loc = (a.double() - scale * r(n, A).clamp(-3, 3).double()).float()
        logits, z = torch.cat([loc, rs], 1), r(n, A)
        rho_star = torch.tensor(RHO_TARGETS)[i % len(RHO_TARGETS)]
        sign = torch.where((i // len(RHO_TARGETS)) % 2 == 0, 1.0, -1.0)
    inp = dict(logits=logits, raw_action=a, noise=z, eps=EPS, entropy_cost=ENTROPY_COST)
    inp["old_logp"] = _old_logp_for(inp, rho_star)
    inp["adv"] = sign * (0.2 + r(n).abs()) if adv is None else adv
    inp["vs"], inp["baseline"] = r(n), r(n)
    inp["rho_star"] = rho_star
    return inp


def cell_counts(cell):
    return torch.bincount(cell.reshape(-1).cpu(), minlength=6).tolist()


F32_ULP = 2.0 ** -23
MIN_PER_CELL = lambda n: max(1, n // 25)      # samples every (clip region x advantage sign) cell must hold: a tenth of the crafted set falls in each outer cell


def scaled_error(got, ref, S):
    """max over ALL elements of |got - ref| / S: the error in units of the terms that were added up (`head_terms`)."""
    return float(((got.detach().double().cpu() - ref.double().cpu()).abs() / S.double().cpu().clamp_min(1e-300)).max())


def bound_from(err32, ulps=8.0):
    """The bound a kernel is held to, from the float32 torch evaluation's error on the SAME inputs against the same float64 reference:
    four times that (the kernels use __expf / __logf / a reciprocal where torch uses the precise forms; both sum at most 16 float32 terms)
    plus a floor of `ulps` float32 ulps of the terms' scale (an evaluation that happens to round luckily must not set a bound of zero)."""
    return 4.0 * err32 + ulps * F32_ULP


class ErrorLog:
    """Records (float32 reference error, kernel error, bound) per case and output; `dump` merges them into
    $ODK_LEARNER_SIZES_OUT/<name> when that directory is given (profiles/learner_sizes/NOTES.md)."""

    def __init__(self, name):
        self.name, self.d = name, {}

    def rec(self, case, output, err32, err_kernel, bound):
        self.d.setdefault(case, {})[output] = dict(float32_torch=err32, kernel=err_kernel, bound=bound)

    def dump(self):
        out = os.environ.get("ODK_LEARNER_SIZES_OUT")
        if not out or not self.d:
            return
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, self.name)
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for k, v in self.d.items():
            old.setdefault(k, {}).update(v)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# whole-network kernels: shared body of test_fused_mlp_matches_torch (tests/test_gpu_learner.py) and the size sweep

def mlp_params(n_in, n_out, g):
    """Random swish MLP n_in -> 512 -> 256 -> 128 -> n_out as the learner keeps it: one flat buffer (W1 b1 W2 b2 ...), the weight
    table, and the two packed copies built by odk_pack_weights."""
    from open_duck_playground_amd import engine
    widths = (n_in,) + engine.MLP_HIDDEN + (n_out,)
    W = [torch.randn(widths[l + 1], widths[l], device="cuda", generator=g) * (1.5 / widths[l] ** 0.5) for l in range(4)]
    b = [0.3 * torch.randn(widths[l + 1], device="cuda", generator=g) for l in range(4)]
    offs, off = [], 0
    for l in range(4):
        offs.append(off); off += W[l].numel() + b[l].numel()
    flat = torch.cat([t.reshape(-1) for l in range(4) for t in (W[l], b[l])])
    table = engine.WeightTable([(offs[l], widths[l + 1], widths[l], l > 0) for l in range(4)])
    pf, pb = torch.zeros(table.fwd_size, device="cuda"), torch.zeros(table.bwd_size, device="cuda")
    engine.pack_weights(flat, pf, pb, table)
    return widths, W, b, flat, table, pf, pb


def packed_reference(Wk):
    """[K, N] matrix (reduction index first) -> the packed layout [pad16(K) / 4][N][4], zero padding."""
    K, N = Wk.shape
    K16 = (K + 15) // 16 * 16
    full = torch.zeros(K16, N, device=Wk.device)
    full[:K] = Wk
    return full.view(K16 // 4, 4, N).permute(0, 2, 1).contiguous().reshape(-1)


def guarded(n, w, g=None):
    """An [n, w] tensor inside a larger NaN-filled allocation (16 floats of NaN in front, a row and more behind): a kernel that reads a
    row past its end, or a tile past the last row, multiplies NaN into its result."""
    front = 16
    big = torch.full((front + (n + 1) * w + 64,), float("nan"), device="cuda")
    t = big[front:front + n * w].view(n, w)
    t.copy_(torch.randn(n, w, device="cuda", generator=g))
    return t


def mlp_float64(x, W, b, dout):
    """float64 forward and backward-data chain of the swish MLP -> (z[4], h[4] (h[0] = x), swish'[3], dz[3])."""
    zs, hs = [], [x.double()]
    for l in range(4):
        z = hs[-1] @ W[l].double().t() + b[l].double()
        zs.append(z)
        if l < 3:
            hs.append(z * torch.sigmoid(z))
    gs, dzs, dzl = [None] * 3, [None] * 3, dout.double()
    for l in (2, 1, 0):
        sg = torch.sigmoid(zs[l])
        gs[l] = sg * (1 + zs[l] * (1 - sg))
        dzl = (dzl @ W[l + 1].double()) * gs[l]
        dzs[l] = dzl
    return zs, hs, gs, dzs


def rel_max(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def check_fused_mlp(n, n_in, n_out):
    """odk_mlp_forward / odk_mlp_backward (one launch per direction for the whole swish MLP) vs float64 torch: output, hidden
    activations, swish', every dz, and the bias gradients through odk_colsum_fold; the zero rows past n; inference-only mode writes
    `out` alone; the packed weight copies against their definition.  Outputs and training buffers start as NaN (an unwritten element
    cannot pass), x and dout sit inside NaN-filled allocations (an over-read cannot pass)."""
    from open_duck_playground_amd import engine
    g = torch.Generator(device="cuda").manual_seed(n + n_in)
    widths, W, b, flat, table, pf, pb = mlp_params(n_in, n_out, g)
    for l in range(4):
        assert torch.equal(table.fwd_view(pf, l), packed_reference(W[l].t()))
        if l > 0:
            assert torch.equal(table.bwd_view(pb, l), packed_reference(W[l]))
    assert table.bwd_view(pb, 0) is None
    x, dout = guarded(n, n_in, g), guarded(n, n_out, g)
    tiles = (n + 15) // 16
    buf = lambda w: torch.full((n, w), float("nan"), device="cuda")
    wf, wb = [table.fwd_view(pf, l) for l in range(4)], [table.bwd_view(pb, l) for l in range(4)]
    tb = engine.FusedMLP.train_buffers(n, n_in, n_out, "cuda")
    for t in [tb["xp"], tb["doutp"]] + tb["h"] + tb["g"] + tb["dz"] + tb["bias_partial"]:
        t.fill_(float("nan"))
    raw = dict(x=x, wf=wf, wb=wb, b=b, out=buf(n_out), dout=dout, **tb)
    op = engine.FusedMLP([raw])
    op.forward(); op.backward()
    # quad-row buffers: rows past the batch are zeros (the weight-gradient launch reads whole tiles); unpack the rest
    np_ = engine.quad_rows(n)
    for key in ("h", "g", "dz"):
        for l, w in enumerate(engine.MLP_HIDDEN):
            assert float(engine.quad_unpack(raw[key][l], np_, w)[n:].abs().sum()) == 0.0
    assert torch.equal(engine.quad_unpack(raw["xp"], n, n_in), x) and torch.equal(engine.quad_unpack(raw["doutp"], n, n_out), dout)
    assert float(engine.quad_unpack(raw["doutp"], np_, n_out)[n:].abs().sum()) == 0.0
    assert bool(torch.isfinite(raw["xp"]).all())              # (its rows past n repeat the last row: they meet zero rows of dz in the weight-gradient launch)
    net = dict(out=raw["out"], bias_partial=raw["bias_partial"], **{key: [engine.quad_unpack(raw[key][l], n, w) for l, w in enumerate(engine.MLP_HIDDEN)]
                                                                    for key in ("h", "g", "dz")})
    for t in [net["out"]] + net["h"] + net["g"] + net["dz"]:
        assert bool(torch.isfinite(t).all())
    zs, hs, gs, dz_ref = mlp_float64(x, W, b, dout)
    assert rel_max(net["out"], zs[3]) < 2e-6
    for l in (2, 1, 0):
        assert rel_max(net["h"][l], hs[l + 1]) < 2e-6 and rel_max(net["g"][l], gs[l]) < 2e-6
        assert rel_max(net["dz"][l], dz_ref[l]) < 3e-6
    gb = [torch.full((w,), float("nan"), device="cuda") for w in widths[1:]]
    engine.ColsumFold([(net["bias_partial"][l], gb[l]) for l in range(4)], tiles)()
    for l in range(3):
        assert rel_max(gb[l], dz_ref[l].sum(0)) < 3e-6
    assert rel_max(gb[3], dout.double().sum(0)) < 3e-6
    # inference only: nothing but `out`
    inf = dict(x=x, wf=wf, b=b, out=buf(n_out))
    engine.FusedMLP([inf]).forward()
    assert torch.equal(inf["out"], net["out"])
    with pytest.raises(engine.OdkError):
        engine.FusedMLP([dict(x=torch.zeros(8, 300, device="cuda"), wf=wf, b=b, out=buf(n_out)[:8])])


# ------------------------------------------------------------------------------------------------------------------------------------
# host tests

def _model(name):
    from open_duck_playground_amd.model import Model, load_task_model
    return Model.from_xml(os.path.join(ASSETS, name)) if name.endswith(".xml") else load_task_model(name)


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_the_size_table_matches_the_compiled_models(robot):
    """Each row of ROBOTS == what the env kernels report for the robot's model (`engine.model_obs_sizes`, host only: the number the
    runner sizes the networks with) == the reference's layout formulas with the robot's actuator count; and which rows the learner
    trains on the whole-network kernels."""
    from open_duck_playground_amd import engine
    name, A, joy, stand = ROBOTS[robot]
    m = _model(name)
    nu = int(m.nu)
    assert nu == A <= MAX_A
    assert joy == (17 + 6 * nu, 17 + 6 * nu + 69 + 3 * nu) and stand == (15 + 5 * nu, 15 + 5 * nu + 26 + 3 * nu)
    if robot == "biped12_neck":          # no compiled kernel shape in a plain build: the loader says so by name, the formulas above stand
        with pytest.raises(engine.OdkError, match="no compiled kernel"):
            engine.model_obs_sizes(m, 0)
    else:
        assert engine.model_obs_sizes(m, 0) == joy and engine.model_obs_sizes(m, 1) == stand
    assert (engine.MLP_MAX_IN, engine.MLP_MAX_OUT) == (MAX_IN, MAX_OUT)
    want = {"duck": (True, True), "biped12": (True, True), "tail_biped": (False, False), "biped12_neck": (True, True), "biped_arms": (False, True)}[robot]
    assert (runs_fused(A, *joy), runs_fused(A, *stand)) == want


def test_runs_fused_is_what_the_learner_decides():
    """`runs_fused` restates `_FlatMLP.fused_ok` for the table: checked against the method itself on CPU tensors (it only looks at shapes
    and flat offsets)."""
    from open_duck_playground_amd.ppo import learner as LM
    from open_duck_playground_amd.ppo.networks import PPONetworks
    for robot, task, A, obs, priv in table_rows():
        net = PPONetworks(obs, priv, A)
        n_par = sum(p.numel() for p in list(net.policy.parameters()) + list(net.value.parameters()))
        fp, fg = torch.zeros(n_par), torch.zeros(n_par)
        pol = LM._FlatMLP(net.policy, fp, fg, 0)
        val = LM._FlatMLP(net.value, fp, fg, pol.end)
        assert (pol.fused_ok() and val.fused_ok()) == runs_fused(A, obs, priv), (robot, task)


def test_the_boundary_rows_are_the_kernels_limits():
    assert max(BOUNDARY_N_IN) == MAX_IN and max(BOUNDARY_N_OUT) == MAX_OUT and max(BOUNDARY_A) == MAX_A == max(HEAD_A)
    pairs = mlp_pairs()
    assert len(pairs) == len(set(pairs)) and all(i <= MAX_IN and o <= MAX_OUT for i, o in pairs)
    assert {(89, 24), (194, 1), (95, 32), (169, 1), (107, 30), (224, 32), (16, 16), (96, 17), (5, 1)} <= set(pairs) and (230, 1) not in pairs


def test_head_reference_matches_ppo_loss_in_float64():
    """The float64 restatement the GPU tests use == `ppo.train.ppo_loss` evaluated in float64 on a small network and the same minibatch:
    the four loss scalars, and every parameter gradient when the restatement's gradients w.r.t. logits and baseline are pushed back
    through the network; GAE and the advantage normalisation by `gae_reference` and the formula of ppo_loss."""
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.networks import PPONetworks
    torch.manual_seed(0)
    B, Tn, A, od, pd = 6, 5, 3, 7, 9
    net = PPONetworks(od, pd, A, policy_hidden=(8, 8), value_hidden=(8,)).double()
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    done = (torch.rand(B, Tn, generator=g) < 0.2).double()
    mb = dict(obs=r(B, Tn, od), priv=r(B, Tn, pd), raw_action=1.5 * r(B, Tn, A), log_prob=-3 + 0.3 * r(B, Tn), reward=0.05 * r(B, Tn).abs(), done=done,
              truncation=(torch.rand(B, Tn, generator=g) < 0.5).double() * done, last_priv=r(B, pd), noise=r(B, Tn, A))
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64))
        net.norm_obs.mean.copy_(0.1 * r(od)); net.norm_priv.std.copy_(1 + 0.1 * r(pd).abs())
    for normalize in (True, False):
        cfg = T.ppo_config(); cfg["normalize_advantage"] = normalize
        net.zero_grad()
        loss, met = T.ppo_loss(net, mb, cfg)
        loss.backward()
        want = [p.grad.clone() for p in net.parameters() if p.grad is not None]
        # the same through the restatement
        n = B * Tn
        logits = net.policy(net.norm_obs(mb["obs"])).reshape(n, 2 * A)
        vals = net.values(mb["priv"])
        term = mb["done"] * (1 - mb["truncation"])
        vs, adv = gae_reference(mb["truncation"], term, mb["reward"] * cfg["reward_scaling"], vals.detach(), net.values(mb["last_priv"]).detach(),
                                cfg["gae_lambda"], cfg["discounting"])
        if normalize:
            adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        inp = dict(logits=logits, raw_action=mb["raw_action"].reshape(n, A), noise=mb["noise"].reshape(n, A), old_logp=mb["log_prob"].reshape(n),
                   adv=adv.reshape(n), vs=vs.reshape(n), baseline=vals.reshape(n), eps=cfg["clipping_epsilon"], entropy_cost=cfg["entropy_cost"])
        ref = head_reference(inp)
        for k, key in enumerate(("total_loss", "policy_loss", "v_loss", "entropy_loss")):
            assert abs(float(ref["losses"][k]) - float(met[key])) < 1e-12 * max(1.0, abs(float(met[key])))
        assert len(set(cell_counts(ref["cell"]))) > 1                      # the minibatch is not all in one cell
        params = [p for p in net.parameters() if p.grad is not None]
        got = torch.autograd.grad([logits, vals.reshape(n)], params, [torch.cat([ref["dloc"], ref["dscale_raw"]], 1), ref["dbaseline"]], allow_unused=True)
        assert len(got) == len(want)
        for a_, b_ in zip(got, want):
            a_ = torch.zeros_like(b_) if a_ is None else a_
            assert float((a_ - b_).abs().max()) <= 1e-10 * max(1.0, float(b_.abs().max()))


@pytest.mark.parametrize("A", HEAD_A)
@pytest.mark.parametrize("kind", ["random", "crafted"])
def test_head_inputs_cover_the_cells_and_stay_in_them_in_float32(A, kind):
    """The inputs the GPU tests feed the loss head: all six (clip region x advantage sign) cells occur; the float32 and the float64
    evaluation put EVERY sample in the same cell (every target ratio keeps 1e-3 from 1 +- eps, float32 moves a ratio by ~1e-5), so no
    sample has to be set aside on the GPU; the ratios are the targets; closed-form gradients == autograd; everything is finite in
    float32; the crafted set reaches |a| = 8 and every raw_scale of RAW_SCALES."""
    for n in (77, 640):
        inp = head_inputs(A, n, kind)
        r64, r32, r32e = head_reference(inp), head_reference(inp, torch.float32), head_reference(inp, torch.float32, eager=True)
        counts = cell_counts(r64["cell"])
        assert min(counts) >= MIN_PER_CELL(n), counts
        assert torch.equal(r64["cell"], r32["cell"]) and torch.equal(r64["cell"], r32e["cell"])
        assert float((r64["rho"] / inp["rho_star"].double() - 1).abs().max()) < 1e-4
        for edge in (1 - EPS, 1 + EPS):
            assert float((r64["rho"] - edge).abs().min()) > 0.9 * EDGE_MARGIN and float((r32["rho"].double() - edge).abs().min()) > 0.9 * EDGE_MARGIN
        for r_ in (r32, r32e):
            assert all(bool(torch.isfinite(r_[k]).all()) for k in ("dloc", "dscale_raw", "dbaseline", "logp", "rho", "losses"))
        g, S = head_terms(inp)
        for k in ("dloc", "dscale_raw", "dbaseline"):
            assert scaled_error(g[k], r64[k], S[k]) < 1e-10, k                 # two float64 derivations: 1e-16 x the log-prob terms (up to 1e3)
            assert scaled_error(r32e[k], r64[k], S[k]) < 1e-3, k              # the float32 yardstick is a sane evaluation of the same head
        if kind == "crafted":
            assert float(inp["raw_action"].abs().max()) == 8.0
            assert set(inp["logits"][:, A:].reshape(-1).tolist()) == set(torch.tensor(RAW_SCALES).tolist()) or n * A < len(RAW_SCALES)
