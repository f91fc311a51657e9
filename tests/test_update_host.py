"""The update half of a minibatch step -- clip + Adam and the packed weight copies (odk_adam_clip, odk_adam_clip_packed[_tail],
odk_pack_weights) -- restated in numpy float64, and the inputs, cases and bounds tests/test_gpu_update_sizes.py holds these kernels to, pinned here without
a GPU:

* `adam_reference`: optax `clip_by_global_norm` followed by `adam`, as csrc/odk_learner.hip documents it;
* `packed_layout_reference`: the two packed copies of every weight of a table, written from the layout comments of csrc/odk_mlp.hip and
  `engine.WeightTable`, held to `packed_reference` of tests/test_learner_sizes_host.py (it takes each weight's offsets from the table:
  that the table's offsets are consecutive padded blocks is asserted separately, the restatement is not independent of them);
* the power of the GPU test: deliberately wrong variants of the update differ from the reference, on the GPU test's own inputs and in
  the quantities it judges, by more than ten times the bounds it asserts.

Figures: profiles/update_kernels/NOTES.md."""
import math

import numpy as np
import pytest

# ---- hyper-parameters: ppo_config()'s learning rate and clip, optax adam's defaults; the kernels receive them as float32 ------------------
LR, B1, B2, EPS, MAX_NORM = 3e-4, 0.9, 0.999, 1e-8, 1.0
STEP_COUNTS = (1, 2, 1000)                                   # t: 1 - b2^t cancels most at the first steps; 1000: both corrections near their limit
NORM_TARGETS = {"below": 0.5, "3x": 3.0, "far": 1000.0}      # |g| against MAX_NORM = 1: no clip, a moderate clip, a clip by three orders
KINDS = tuple(NORM_TARGETS)

# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
# m = b1 m + (1 - b1) g c, v = b2 v + (1 - b2) (g c)^2 with c the clip factor.  From float32 inputs: the products b1 m and (1 - b1) (g c)
# round once each (2^-24 relative), g c once more, the sum once; (g c)^2 doubles g c's error: <= 4 roundings for m, <= 6 for v when the
# terms have one sign (v always; m by the choice of inputs below), i.e. 3.6e-7, fused multiply-adds only remove roundings.  c itself is
# max_norm / sqrt(sq): two roundings plus HALF the relative error of the float32 squared norm, which enters v twice -- the fold of
# positive terms is a tree (SQNORM_BOUND below is its worst case; its error on random data is a fraction of an ulp per level and the
# levels do not add up coherently).  5e-7 = 8.4 * 2^-24 leaves the norm two ulps.
MV_BOUND = 5e-7
MV_FLOOR = 1e-12
# acc[0] = sum g^2 in float32, fixed order: a thread adds ceil(n / (blocks * 256)) <= 4 squares (n <= 1 M: blocks = ceil(n / 1024)), each
# square rounds once (1 + 3 additions), the wave butterfly adds 6 levels, the block's 4 waves 4 additions, then every block folds the
# <= 1024 partials: 4 per thread, 6 butterfly levels, 4 waves: 1 + 3 + 6 + 4 + 4 + 6 + 4 = 28 roundings of positive terms on any path,
# 28 * 2^-24 = 1.7e-6.
SQNORM_BOUND = 2e-6
# p: |p - p_ref| <= ulp32(|p_old|) + LR * eps_u * max(|u_ref|, U_FLOOR), u = the step in units of the learning rate.  The first term is
# the rounding of the stored float32 p.  eps_u, the relative error of the step, cannot be derived tightly: 1 - powf(b2, t) = 0.002 at
# t = 2 carries powf's absolute error (an ulp of 0.998 is 6e-8) as a RELATIVE error of 3e-5 per ulp, half of which reaches u through the
# square root.  It is MEASURED, per step count (the cancellation is a property of t: none at t = 1, where 1 - b2 is exact, the worst at
# t = 2, next to none at t = 1000), as the worst case of tests/test_gpu_update_sizes.py over all its cases, and asserted at about three
# times that: profiles/update_kernels/NOTES.md.  One bound over all step counts would be set by t = 2 and could not tell t = 1000 from
# t = 1001, which moves the step by 2.9e-4 of itself.
EPS_U_BOUND = {1: 3e-6, 2: 1e-4, 1000: 3e-6}
U_FLOOR = 1e-3


def eps_u_bound(t):
    """the bound of the largest tabulated step count <= t: the cancellation in 1 - b^t only gets milder as t grows"""
    return EPS_U_BOUND[max(k for k in EPS_U_BOUND if k <= t)]


def bounds(t):
    return dict(eps_u=eps_u_bound(t), m_rel=MV_BOUND, v_rel=MV_BOUND, sqnorm_rel=SQNORM_BOUND)

# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
# single weights (rows = n_out, cols = n_in) against adam_tiled_kernel's 16 x 64 tile, each followed by its bias
SINGLE_SHAPES = ((16, 64), (17, 65), (15, 63), (4, 4), (5, 3), (1, 128), (28, 128), (33, 101))
PLAIN_SIZES = (1, 3, 4, 5, 1023, 1025, 493469)              # odk_adam_clip: around the float4 body / one block of 1024; the duck's parameter count
TAIL_COUNTS = (1, 15, 16, 17, 160)                           # loss partials: below / at / past the fold's 16 slices, the learner's 160
EIGHT_SHAPES = ((17, 65, True), (5, 3, True), (1, 128, True), (33, 101, False), (16, 64, True), (4, 4, True), (28, 128, True), (15, 63, True))


def f32(x):
    """the float32 value a kernel receives for the Python float x, as a float64"""
    return np.float64(np.float32(x))


def pad16(k):
    return (int(k) + 15) // 16 * 16


def single_entries(rows, cols, bwd):
    """[(offset, rows, cols, backward copy?)] and the parameter count: one weight at offset 0 and its bias behind it"""
    return [(0, rows, cols, bwd)], rows * cols + rows


def eight_entries():
    """The limit of eight weights: three parameters in FRONT of the first weight, a bias (rows floats) in every gap, NOTHING behind the last
    weight, one weight without a backward copy, a total that is no multiple of 4 (asserted below) -- so most weights start off the
    16-byte grid of the torch-layout streams."""
    entries, off = [], 3
    for k, (r, c, bw) in enumerate(EIGHT_SHAPES):
        entries.append((off, r, c, bw))
        off += r * c + (r if k + 1 < len(EIGHT_SHAPES) else 0)
    return entries, off


def unordered(entries):
    """the same weights listed out of ascending order: the host falls back from adam_tiled_kernel to adam_packed_kernel"""
    return [entries[k] for k in (3, 0, 7, 1, 6, 2, 5, 4)]


# ---- the reference -------------------------------------------------------------------------------------------------------------------------

def adam_reference(p, g, m, v, t, lr, b1, b2, eps, max_norm):
    """optax.chain(clip_by_global_norm(max_norm), adam(lr, b1, b2, eps)) on flat buffers, step count t (1 at the first step), in float64.
    The hyper-parameters count as the float32 values the kernel receives.  -> dict(p, m, v, u = the step in units of lr, sq = sum g^2)."""
    lr, b1, b2, eps, max_norm = (f32(x) for x in (lr, b1, b2, eps, max_norm))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    sq = float(np.sum(g * g))
    norm = math.sqrt(sq)
    if max_norm > 0 and not norm < max_norm:
        g = g * (max_norm / norm)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return dict(p=p - lr * u, m=m, v=v, u=u, sq=sq, gc=g)


VARIANTS = ("no_b2_correction", "eps_in_sqrt", "clip_on_m", "clip_at_equality", "t_plus_one", "clip_below_too", "m_sign")


def wrong_update(variant, p, g, m, v, t, lr, b1, b2, eps, max_norm):
    """`adam_reference` with ONE deliberate mistake (variant None: none -- equal to adam_reference bit for bit, asserted below):
    no_b2_correction  v is not divided by 1 - b2^t;
    eps_in_sqrt       sqrt(vhat + eps) for sqrt(vhat) + eps;
    clip_on_m         the clip factor scales the new first moment instead of the gradient (v sees the raw gradient);
    clip_at_equality  clips when norm > max_norm, not when norm >= max_norm;
    t_plus_one        the bias corrections of the next step;
    clip_below_too    g * max_norm / norm whatever the norm (scales small gradients UP);
    m_sign            b1 m - (1 - b1) g."""
    lr, b1, b2, eps, max_norm = (f32(x) for x in (lr, b1, b2, eps, max_norm))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    sq = float(np.sum(g * g))
    norm = math.sqrt(sq)
    clips = max_norm > 0 and (not norm <= max_norm if variant == "clip_at_equality" else not norm < max_norm)
    if variant == "clip_below_too":
        clips = max_norm > 0 and norm > 0
    c = max_norm / norm if clips else 1.0
    if variant == "clip_on_m":
        m, v = c * (b1 * m + (1 - b1) * g), b2 * v + (1 - b2) * g * g
    else:
        g = g * c if clips else g
        m, v = b1 * m + (-1 if variant == "m_sign" else 1) * (1 - b1) * g, b2 * v + (1 - b2) * g * g
    tt = t + 1 if variant == "t_plus_one" else t
    vhat = v if variant == "no_b2_correction" else v / (1 - b2 ** tt)
    den = np.sqrt(vhat + eps) if variant == "eps_in_sqrt" else np.sqrt(vhat) + eps
    u = (m / (1 - b1 ** tt)) / den
    return dict(p=p - lr * u, m=m, v=v, u=u, sq=sq, gc=g)


def packed_layout_reference(flat_p, table):
    """(forward-packed, backward-packed) buffers of `table` (an engine.WeightTable) for the flat parameters `flat_p`, zeros in every slot
    no weight element owns.  Weight k = flat_p[off : off + rows * cols] as [rows = n_out][cols = n_in]; its forward copy sits at the
    table's forward offset as [ceil(cols / 4)][rows][4] -- element (o, i) at ((i // 4) * rows + o) * 4 + i % 4 -- and its backward copy (if it
    has one) at the backward offset as [ceil(rows / 4)][cols][4] -- element (o, i) at ((o // 4) * cols + i) * 4 + o % 4.  The table reserves
    pad16(cols) * rows and pad16(rows) * cols floats for them."""
    flat_p = np.asarray(flat_p)
    pf, pb = np.zeros(table.fwd_size, flat_p.dtype), np.zeros(table.bwd_size, flat_p.dtype)
    for (off, rows, cols, _), (fo, _), back in zip(table.entries, table.fwd, table.bwd):
        W = flat_p[off:off + rows * cols].reshape(rows, cols)
        o, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        pf[fo + ((i // 4) * rows + o) * 4 + i % 4] = W
        if back is not None:
            pb[back[0] + ((o // 4) * cols + i) * 4 + o % 4] = W
    return pf, pb


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

def update_inputs(n, kind, t, seed=0, signs="same"):
    """float32 (p, g, m, v) of n parameters for step count t:
    p ~ N(0, 0.05^2), the scale of initialised weights (unit-scale weights would bury the step under p's own rounding);
    g ~ N(0, 1), every fourth element (index % 4 == 1) a further 1e-4 smaller -- units that are almost dead, whose second moment sits at
      the level of eps: without them `eps_in_sqrt` changes nothing that float32 resolves -- scaled to the norm NORM_TARGETS[kind];
    m, v = the moments a reference step from zero leaves for a previous gradient of the same norm and, element by element, the SAME SIGN:
      m's sum b1 m + (1 - b1) g then never cancels, which a relative bound on m needs (a cancelling float32 sum has no such bound).
      signs = "mixed": the previous gradient's signs are drawn independently, as in training; m cancels in half of the elements, and the
      results are judged by `judged_mixed`."""
    rng = np.random.default_rng([seed, n, t, KINDS.index(kind)] + ([1] if signs == "mixed" else []))
    p = (0.05 * rng.standard_normal(n)).astype(np.float32)
    small = np.where(np.arange(n) % 4 == 1, 1e-4, 1.0)
    z = rng.standard_normal(n) * small
    g = (z * (NORM_TARGETS[kind] / np.linalg.norm(z))).astype(np.float32)
    sgn = np.where(g < 0, -1.0, 1.0) if signs == "same" else rng.choice([-1.0, 1.0], n)
    zp = np.abs(rng.standard_normal(n)) * small * sgn
    gp = (zp * (NORM_TARGETS[kind] / np.linalg.norm(zp))).astype(np.float32)
    prev = adam_reference(np.zeros(n), gp, np.zeros(n), np.zeros(n), 1, LR, B1, B2, EPS, MAX_NORM)
    return dict(p=p, g=g, m=prev["m"].astype(np.float32), v=prev["v"].astype(np.float32))


def tail_partials(count, seed=0):
    """[count, 4] float32 per-workgroup loss sums of mixed sign and uneven size"""
    rng = np.random.default_rng([seed, count])
    return (rng.standard_normal((count, 4)) * 10.0 ** rng.uniform(-2, 1, (count, 4))).astype(np.float32)


def tail_bound(partials):
    """per component: the fold's depth -- ceil(count / 16) additions per slice, 4 butterfly levels, the += -- in float32 roundings of sum |partial|"""
    count = partials.shape[0]
    return (count / 16 + 5) * 2.0 ** -24 * np.abs(partials.astype(np.float64)).sum(0)


# ---- the judged quantities -------------------------------------------------------------------------------------------------------------------

def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def rel_err(got, ref, floor=MV_FLOOR):
    """max over all elements of |got - ref| / max(|ref|, floor)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), floor)).max())


def step_err(got_p, ref, p_old, lr=LR, slack=0.0):
    """eps_u: max over all elements of (|p - p_ref| - ulp32(|p_old|))+ / (lr max(|u_ref|, U_FLOOR)): the error of the step, in units of the
    step, beyond the rounding of the stored p (`slack`: a further allowance per element, in units of lr -- `judged_mixed`)"""
    excess = np.abs(np.asarray(got_p, dtype=np.float64) - ref["p"]) - ulp32(p_old) - f32(lr) * slack
    return float((np.maximum(excess, 0.0) / (f32(lr) * np.maximum(np.abs(ref["u"]), U_FLOOR))).max())


def judged(got, ref, p_old):
    """the quantities of BOUNDS for a result dict(p, m, v[, sq])"""
    q = dict(eps_u=step_err(got["p"], ref, p_old), m_rel=rel_err(got["m"], ref["m"]), v_rel=rel_err(got["v"], ref["v"]))
    if "sq" in got:
        q["sqnorm_rel"] = abs(float(got["sq"]) - ref["sq"]) / ref["sq"] if ref["sq"] > 0 else abs(float(got["sq"]))
    return q


def judged_mixed(got, ref, inp, t):
    """`judged` for moments of mixed sign, where b1 m + (1 - b1) g c may cancel and m has no relative bound: m is judged ABSOLUTELY, in
    units of |b1 m| + |(1 - b1) g c| (<= twice the larger term: MV_BOUND there is the same four roundings), and the step is allowed what
    that error of m becomes in u: MV_BOUND (|b1 m| + |(1 - b1) g c|) / (1 - b1^t) / (sqrt(vhat) + eps)."""
    b1, b2, eps = f32(B1), f32(B2), f32(EPS)
    mag = np.abs(b1 * inp["m"].astype(np.float64)) + np.abs((1 - b1) * ref["gc"])
    slack = MV_BOUND * mag / (1 - b1 ** t) / (np.sqrt(ref["v"] / (1 - b2 ** t)) + eps)
    q = dict(eps_u=step_err(got["p"], ref, inp["p"], slack=slack), v_rel=rel_err(got["v"], ref["v"]),
             m_rel=float((np.abs(np.asarray(got["m"], dtype=np.float64) - ref["m"]) / np.maximum(mag, MV_FLOOR)).max()))
    if "sq" in got:
        q["sqnorm_rel"] = abs(float(got["sq"]) - ref["sq"]) / ref["sq"]
    return q


def update_cases():
    """(name, n) of every size the GPU test runs the arithmetic at (its FlatLearner tables have the networks' own parameter counts, between
    the last two plain sizes); each runs every (t, kind) of STEP_COUNTS x KINDS"""
    cases = [(f"{r}x{c}", single_entries(r, c, True)[1]) for r, c in SINGLE_SHAPES]
    cases.append(("eight", eight_entries()[1]))
    return cases + [(f"plain{n}", n) for n in PLAIN_SIZES]


def hyper():
    return LR, B1, B2, EPS, MAX_NORM


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------

def test_reference_against_a_scalar_restatement_and_torch_adam():
    """adam_reference element by element in plain Python floats, and against torch.optim.Adam in float64 (no clip: norm below max_norm)"""
    import torch
    inp = update_inputs(37, "below", 3)
    lr, b1, b2, eps, mx = (float(f32(x)) for x in hyper())
    ref = adam_reference(inp["p"], inp["g"], inp["m"], inp["v"], 3, *hyper())
    for k in range(37):
        g, m, v = float(inp["g"][k]), float(inp["m"][k]), float(inp["v"][k])
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        want = float(inp["p"][k]) - lr * (m / (1 - b1 ** 3)) / (math.sqrt(v / (1 - b2 ** 3)) + eps)
        assert abs(ref["p"][k] - want) <= 1e-15 and abs(ref["m"][k] - m) <= 1e-18 and abs(ref["v"][k] - v) <= 1e-20
    # three steps of torch's Adam from zero moments == three reference steps (torch: eps outside the root of the corrected v, as optax)
    p = torch.tensor(inp["p"], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    q, m, v = inp["p"].astype(np.float64), np.zeros(37), np.zeros(37)
    for t in (1, 2, 3):
        p.grad = torch.tensor(inp["g"], dtype=torch.float64)
        opt.step()
        r = adam_reference(q, inp["g"], m, v, t, *hyper())
        q, m, v = r["p"], r["m"], r["v"]
    assert np.abs(p.detach().numpy() - q).max() < 1e-12 * LR
    # the clip: a gradient of norm 3 gives the update of the same gradient scaled to norm 1; max_norm = 0 switches the clip off
    big = update_inputs(37, "3x", 3)
    a = adam_reference(big["p"], big["g"], big["m"], big["v"], 3, *hyper())
    b = adam_reference(big["p"], big["g"].astype(np.float64) / math.sqrt(a["sq"]), big["m"], big["v"], 3, *hyper())
    c = adam_reference(big["p"], big["g"], big["m"], big["v"], 3, LR, B1, B2, EPS, 0.0)
    assert np.abs(a["p"] - b["p"]).max() < 1e-15 and abs(math.sqrt(a["sq"]) - 3.0) < 1e-6
    assert np.abs(c["m"] - (f32(B1) * big["m"] + (1 - f32(B1)) * big["g"].astype(np.float64))).max() == 0.0
    assert all(np.array_equal(wrong_update(None, big["p"], big["g"], big["m"], big["v"], 3, *hyper())[k], a[k]) for k in ("p", "m", "v", "u"))


def test_inputs_are_what_the_gpu_test_assumes():
    for kind in KINDS:
        for n in (1, 5, 84, 1025):
            inp = update_inputs(n, kind, 2)
            norm = float(np.linalg.norm(inp["g"].astype(np.float64)))
            assert abs(norm / NORM_TARGETS[kind] - 1) < 1e-6                               # far from max_norm on either side: float32 and float64 agree on the clip
            assert all(a.dtype == np.float32 and a.shape == (n,) for a in inp.values())
            assert np.all(inp["m"] * inp["g"] >= 0) and np.all(inp["v"] >= 0) and (n < 2 or np.all(inp["m"] != 0))
    p = update_inputs(493469, "3x", 2)["p"]
    assert abs(float(p.std()) - 0.05) < 1e-3
    mixed = update_inputs(1025, "3x", 2, signs="mixed")
    agree = float(np.mean(mixed["m"] * mixed["g"] > 0))
    assert 0.4 < agree < 0.6 and np.array_equal(mixed["g"], update_inputs(1025, "3x", 2)["g"]) is False
    entries, n = eight_entries()
    assert len(entries) == 8 and n % 4 != 0 and entries[0][0] == 3 and entries[-1][0] + entries[-1][1] * entries[-1][2] == n
    assert sum(1 for e in entries if not e[3]) == 1 and sum(1 for e in entries if e[0] % 4) >= 4
    assert sorted(unordered(entries)) == sorted(entries) and unordered(entries) != sorted(entries)
    assert any(a[0] > b[0] for a, b in zip(unordered(entries), unordered(entries)[1:]))


def _tables():
    from open_duck_playground_amd import engine
    out = [engine.WeightTable(single_entries(r, c, bw)[0]) for r, c in SINGLE_SHAPES for bw in (True, False)]
    entries, n = eight_entries()
    return out + [engine.WeightTable(entries), engine.WeightTable(unordered(entries)), engine.WeightTable([(0, 64, 64, True), (4160, 40, 21, False)])]


def test_packed_layout_reference_against_packed_reference_and_the_tables_offsets():
    """The restated layout == `packed_reference` (the helper the whole-network kernel tests hold odk_pack_weights to) for every weight of
    every table the GPU test uses, forward copy = the transposed weight with the input index as reduction index, backward copy = the weight
    itself; every float outside the weights' elements is zero; the table's offsets are consecutive blocks of pad16(cols) * rows and
    pad16(rows) * cols floats, each a multiple of 4."""
    import torch
    from test_learner_sizes_host import packed_reference
    rng = np.random.default_rng(3)
    for table in _tables():
        n = max(o + r * c for o, r, c, _ in table.entries) + 5
        flat = rng.standard_normal(n).astype(np.float32)
        flat[flat == 0] = 1.0
        pf, pb = packed_layout_reference(flat, table)
        assert pf.dtype == np.float32 and pf.shape == (table.fwd_size,) and pb.shape == (table.bwd_size,)
        fo = bo = 0
        for k, (off, rows, cols, bw) in enumerate(table.entries):
            W = torch.from_numpy(flat[off:off + rows * cols].reshape(rows, cols))
            assert table.fwd[k] == (fo, pad16(cols) * rows) and fo % 4 == 0 and table.c.fwd_off[k] == fo
            assert np.array_equal(pf[fo:fo + pad16(cols) * rows], packed_reference(W.t()).numpy())
            fo += pad16(cols) * rows
            if bw:
                assert table.bwd[k] == (bo, pad16(rows) * cols) and bo % 4 == 0 and table.c.bwd_off[k] == bo
                assert np.array_equal(pb[bo:bo + pad16(rows) * cols], packed_reference(W).numpy())
                bo += pad16(rows) * cols
            else:
                assert table.bwd[k] is None and table.c.bwd_off[k] == -1
        assert (fo, max(bo, 4)) == (table.fwd_size, table.bwd_size)
        assert np.count_nonzero(pf) == sum(r * c for _, r, c, _ in table.entries)
        assert np.count_nonzero(pb) == sum(r * c for _, r, c, bw in table.entries if bw)


def separation_table(signs="same"):
    """variant -> {(t, kind): the largest judged quantity over `update_cases`, in units of its bound}"""
    sep = {v: {} for v in VARIANTS}
    for _, n in update_cases():
        for t in STEP_COUNTS:
            for kind in KINDS:
                inp = update_inputs(n, kind, t, signs=signs)
                args = (inp["p"], inp["g"], inp["m"], inp["v"], t) + hyper()
                ref = adam_reference(*args)
                for variant in VARIANTS:
                    got = wrong_update(variant, *args)
                    q = judged(got, ref, inp["p"]) if signs == "same" else judged_mixed(got, ref, inp, t)
                    f = max(q[k] / bounds(t)[k] for k in q)
                    sep[variant][(t, kind)] = max(sep[variant].get((t, kind), 0.0), f)
    return sep


SEPARATION = 10.0
ALL_CELLS = [(t, k) for t in STEP_COUNTS for k in KINDS]
LIVE = {
    "no_b2_correction": ALL_CELLS,
    "eps_in_sqrt": ALL_CELLS,
    "clip_on_m": [(t, k) for t in STEP_COUNTS for k in ("3x", "far")],
    "clip_below_too": [(t, "below") for t in STEP_COUNTS],
    "t_plus_one": ALL_CELLS,
    "m_sign": ALL_CELLS,
}


def _assert_separation(sep):
    for variant, cells in sep.items():
        print(variant, {f"t={t}/{kind}": float(f"{f:.3g}") for (t, kind), f in sorted(cells.items())})
    for variant, cells in LIVE.items():
        weak = {c: sep[variant][c] for c in cells if not sep[variant][c] > SEPARATION}
        assert not weak, (variant, weak)


def test_wrong_variants_separate_from_the_reference_by_ten_bounds():
    """The power of tests/test_gpu_update_sizes.py, on its own inputs (every size of `update_cases`, every t and gradient norm) and in the
    quantities it judges: each wrong variant of the update misses the reference by more than SEPARATION times the asserted bound in EVERY
    (t, norm) cell in which the mistake is live: the missing correction, the misplaced eps, the step count and m's sign everywhere, the
    clip on m where the clip acts, the clip below max_norm where it must not.

    `clip_at_equality` CANNOT separate, on any finite input: at norm == max_norm the clip factor max_norm / norm is exactly 1, so clipping
    and not clipping give the same bits (and a NaN norm fails both comparisons alike).  That identity is asserted instead, on a gradient
    whose float32 and float64 norms are exactly max_norm."""
    sep = separation_table()
    _assert_separation(sep)
    assert max(sep["clip_at_equality"].values()) == 0.0
    n = 4
    p, g, m, v = np.full(n, 0.05, np.float32), np.full(n, 0.5, np.float32), np.full(n, 0.01, np.float32), np.full(n, 1e-4, np.float32)
    assert float(np.sum(g.astype(np.float64) ** 2)) == 1.0
    a, b = adam_reference(p, g, m, v, 2, *hyper()), wrong_update("clip_at_equality", p, g, m, v, 2, *hyper())
    assert all(np.array_equal(a[k], b[k]) for k in ("p", "m", "v"))


def test_wrong_variants_separate_with_moments_of_mixed_sign_too():
    """the same with the previous gradient's signs drawn independently, in the quantities of `judged_mixed`"""
    _assert_separation(separation_table(signs="mixed"))


def test_tail_bound_and_partials():
    for count in TAIL_COUNTS:
        part = tail_partials(count)
        assert part.shape == (count, 4) and part.dtype == np.float32 and (part > 0).any() and (part < 0).any()
        assert np.all(tail_bound(part) > 0) and np.all(tail_bound(part) < 1e-5 * np.abs(part).sum(0))
