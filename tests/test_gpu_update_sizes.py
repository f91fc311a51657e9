"""The update half of a minibatch step -- odk_adam_clip (adam_kernel, sqnorm_kernel), odk_adam_clip_packed[_tail] (adam_tiled_kernel,
adam_packed_kernel, sqnorm_p_kernel, step_tail) and odk_pack_weights (pack_weights_kernel) -- against the float64 restatement of
tests/test_update_host.py, PER ELEMENT, and the packed weight copies against the restated layout BIT FOR BIT, at the shapes where the
tiled kernel's edges lie and at every robot's network sizes.  Inputs, cases, bounds and their derivations: tests/test_update_host.py
(which also shows, without a GPU, that wrong variants of the update miss these bounds ten times over on these inputs).

Judged per element against float64:
* m, v: relative, floor 1e-12, at MV_BOUND = 5e-7: four / six float32 roundings of same-signed terms plus the clip factor's error;
* p: |p - p_ref| <= ulp32(|p_old|) + lr eps_u(t) max(|u_ref|, 1e-3); eps_u is kept per step count; its rule is about three times the
  recorded worst case, and its present figures are estimates from the arithmetic (profiles/update_kernels/NOTES.md);
* acc[0] = sum g^2: relative 2e-6 = 28 float32 roundings of positive terms on the longest path of the fold for n <= 1 M: a thread adds
  <= 4 squares (1 + 3), 6 butterfly levels, 4 waves, then <= 1024 partials: 4 per thread, 6 levels, 4 waves;
* acc[1] == t exactly.
Every figure goes through `parity_log` under update_kernels/t=<t> before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_learner_sizes import LEARNER_ROWS
from test_learner_sizes_host import row, runs_fused
from test_update_host import (B1, B2, EPS, KINDS, LR, MAX_NORM, MV_BOUND, PLAIN_SIZES, SINGLE_SHAPES, STEP_COUNTS, TAIL_COUNTS, U_FLOOR, adam_reference,
                              bounds, eight_entries, f32, judged, judged_mixed, packed_layout_reference, rel_err, single_entries, tail_bound,
                              tail_partials, ulp32, unordered, update_inputs)

pytestmark = pytest.mark.gpu

CELLS = [(t, kind) for t in STEP_COUNTS for kind in KINDS]


@functools.lru_cache(maxsize=None)
def _case(n, kind, t, signs="same", max_norm=MAX_NORM):
    """(inputs, float64 reference) of one case: computed once, shared by every test that runs it, never written to"""
    inp = update_inputs(n, kind, t, signs=signs)
    ref = adam_reference(inp["p"], inp["g"], inp["m"], inp["v"], t, LR, B1, B2, EPS, max_norm)
    for a in list(inp.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return inp, ref


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(inp, t, table=None, max_norm=MAX_NORM, **tail):
    """One call of odk_adam_clip (table None) or odk_adam_clip_packed[_tail] with acc[1] preset to t - 1 and every other float of acc
    to a value no result may keep; the packed buffers start as zeros, as FlatLearner allocates them."""
    from open_duck_playground_amd import engine
    p, g, m, v = (torch.from_numpy(np.array(inp[k])).cuda() for k in ("p", "g", "m", "v"))
    acc = torch.full((engine.ADAM_ACC_FLOATS,), 7.0, device="cuda")
    acc[1] = float(t - 1)
    out = {}
    if table is None:
        engine.adam_clip(p, g, m, v, acc, LR, max_norm, B1, B2, EPS)
    else:
        pf, pb = torch.zeros(table.fwd_size, device="cuda"), torch.zeros(table.bwd_size, device="cuda")
        engine.adam_clip_packed(p, g, m, v, acc, pf, pb, table, LR, max_norm, B1, B2, EPS, **tail)
        rf, rb = torch.zeros_like(pf), torch.zeros_like(pb)
        engine.pack_weights(p, rf, rb, table)
        out.update(pf=pf.cpu().numpy(), pb=pb.cpu().numpy(), rf=rf.cpu().numpy(), rb=rb.cpu().numpy())
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), torch.from_numpy(np.array(inp["g"])))
    out.update(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), sq=float(acc[0]), t=float(acc[1]))
    return out


def _check_update(plog, got, inp, ref, t, signs="same"):
    assert got["t"] == float(t)
    assert all(np.isfinite(got[k]).all() for k in ("p", "m", "v"))
    q = judged(got, ref, inp["p"]) if signs == "same" else judged_mixed(got, ref, inp, t)
    plog.check(f"update_kernels/t={t}" + ("" if signs == "same" else "/mixed_signs"), bounds(t), **q)


def _check_layout(got, table):
    """pf, pb == the restated layout of the p the same call returned, padding included, == a fresh odk_pack_weights of that p"""
    pf, pb = packed_layout_reference(got["p"], table)
    assert np.array_equal(_bits(got["pf"]), _bits(pf)) and np.array_equal(_bits(got["pb"]), _bits(pb))
    assert np.array_equal(_bits(got["rf"]), _bits(pf)) and np.array_equal(_bits(got["rb"]), _bits(pb))


def _gap_mask(table, n):
    mask = np.ones(n, bool)
    for off, rows, cols, _ in table.entries:
        mask[off:off + rows * cols] = False
    return mask


def _check_gaps(got, plain, inp, ref, table):
    """The parameters outside every weight (the biases) are updated exactly once: == the plain kernel's result (another compilation of
    the same arithmetic: m, v at MV_BOUND; p within an ulp of the stored value + MV_BOUND of the step), and none keeps its old value
    where the reference step exceeds p's own rounding."""
    k = _gap_mask(table, inp["p"].size)
    if not k.any():
        return
    assert rel_err(got["m"][k], plain["m"][k]) <= MV_BOUND and rel_err(got["v"][k], plain["v"][k]) <= MV_BOUND
    dp = np.abs(got["p"][k].astype(np.float64) - plain["p"][k])
    assert np.all(dp <= np.maximum(ulp32(inp["p"][k]), ulp32(plain["p"][k])) + f32(LR) * MV_BOUND * np.maximum(np.abs(ref["u"][k]), U_FLOOR))
    moved = f32(LR) * np.abs(ref["u"][k]) > ulp32(inp["p"][k])
    assert moved.any() and np.all(got["p"][k][moved] != inp["p"][k][moved])


def _sweep(plog, table, n, cells=CELLS):
    for t, kind in cells:
        inp, ref = _case(n, kind, t)
        got = _run(inp, t, table)
        _check_update(plog, got, inp, ref, t)
        _check_layout(got, table)
        _check_gaps(got, _run(inp, t), inp, ref, table)


# ---- 1. the plain kernel ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", PLAIN_SIZES)
def test_adam_clip_matches_float64(parity_log, n):
    """odk_adam_clip around its four-element pieces and one block's 1024 parameters, and at the duck's parameter count"""
    for t, kind in CELLS:
        inp, ref = _case(n, kind, t)
        _check_update(parity_log, _run(inp, t), inp, ref, t)


# ---- 2. the packed kernels ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bwd", [True, False])
@pytest.mark.parametrize("rows, cols", SINGLE_SHAPES)
def test_one_weight_and_its_bias(parity_log, rows, cols, bwd):
    """adam_tiled_kernel on one weight around its 16 x 64 tile, with a bias behind it: update, both packed copies, the bias"""
    from open_duck_playground_amd import engine
    entries, n = single_entries(rows, cols, bwd)
    _sweep(parity_log, engine.WeightTable(entries), n)


@pytest.mark.parametrize("variant", ["tiled", "unordered", "linear"])
def test_eight_weights(parity_log, variant, monkeypatch):
    """The limit of eight weights (a gap in front, biases between, nothing behind, one weight without a backward copy, n % 4 != 0) on
    adam_tiled_kernel, and on adam_packed_kernel, which the host falls back to when the weights are listed out of ascending order or
    ODK_ADAM_LINEAR is set (read per call): the same answers, the same layouts."""
    from open_duck_playground_amd import engine
    entries, n = eight_entries()
    if variant == "linear":
        monkeypatch.setenv("ODK_ADAM_LINEAR", "1")
    _sweep(parity_log, engine.WeightTable(unordered(entries) if variant == "unordered" else entries), n)


@pytest.mark.parametrize("rows, cols", [(33, 101), (5, 3)])
def test_element_wise_variant_on_one_weight(parity_log, rows, cols, monkeypatch):
    from open_duck_playground_amd import engine
    monkeypatch.setenv("ODK_ADAM_LINEAR", "1")
    entries, n = single_entries(rows, cols, True)
    _sweep(parity_log, engine.WeightTable(entries), n, cells=[(2, "3x"), (1000, "below")])


@pytest.mark.parametrize("robot, task", LEARNER_ROWS)
def test_the_learners_own_tables(parity_log, robot, task):
    """One step on the weight table FlatLearner builds for the robot's networks (rows on the whole-network kernels), or -- rows on the
    library path, where the learner keeps no packed copies -- of odk_adam_clip at the networks' parameter count"""
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.learner import FlatLearner
    from open_duck_playground_amd.ppo.networks import PPONetworks
    A, obs, priv = row(robot, task)
    torch.manual_seed(0)
    lr = FlatLearner(PPONetworks(obs, priv, A).to("cuda"), T.ppo_config(), 8, 20, use_graph=False)
    n, table = lr.flat_p.numel(), (lr.wtable if lr.fused is not None else None)
    assert (table is not None) == runs_fused(A, obs, priv)
    if table is None:
        inp, ref = _case(n, "3x", 2)
        _check_update(parity_log, _run(inp, 2), inp, ref, 2)
    else:
        assert len(table.entries) == 8 and table.fwd_size == lr.packed_f.numel() and table.bwd_size == lr.packed_b.numel()
        _sweep(parity_log, table, n, cells=[(2, "3x")])


def test_moments_of_mixed_sign(parity_log):
    """The training case: m and g differ in sign in half of the elements, b1 m + (1 - b1) g cancels.  m absolutely, in units of the terms'
    magnitudes, the step with what that becomes in u (`judged_mixed`); tiled, element-wise and plain kernel."""
    from open_duck_playground_amd import engine
    entries, n = eight_entries()
    for t, kind in CELLS:
        inp, ref = _case(n, kind, t, "mixed")
        for table in (engine.WeightTable(entries), engine.WeightTable(unordered(entries)), None):
            _check_update(parity_log, _run(inp, t, table), inp, ref, t, "mixed")


def test_zero_gradient_and_no_clip(parity_log):
    from open_duck_playground_amd import engine
    entries, n = eight_entries()
    inp, _ = _case(n, "3x", 2)
    zero = np.zeros(n, np.float32)
    for table in (engine.WeightTable(entries), engine.WeightTable(unordered(entries)), None):
        # g = 0 and m = v = 0: 0 / (0 + eps), p keeps its bits; g = 0 with moments: finite, == the reference
        got = _run(dict(p=inp["p"], g=zero, m=zero, v=zero), 1, table)
        assert np.array_equal(_bits(got["p"]), _bits(inp["p"])) and got["sq"] == 0.0 and not got["m"].any() and not got["v"].any()
        quiet = dict(inp, g=zero)
        got = _run(quiet, 2, table)
        ref = adam_reference(quiet["p"], zero, quiet["m"], quiet["v"], 2, LR, B1, B2, EPS, MAX_NORM)
        q = judged(got, ref, quiet["p"])
        assert q.pop("sqnorm_rel") == 0.0
        parity_log.check("update_kernels/t=2", bounds(2), **q)
        # max_norm = 0: a gradient of norm 3 is NOT clipped
        ref0 = _case(n, "3x", 2, "same", 0.0)[1]
        got = _run(inp, 2, table, max_norm=0.0)
        _check_update(parity_log, got, inp, ref0, 2)
        assert rel_err(got["m"], _case(n, "3x", 2)[1]["m"]) > 0.1


# ---- 3. the step tail ----------------------------------------------------------------------------------------------------------------------------

def _tail_call(table, inp, count, losses0, cursor0, with_cursor=True, with_partials=True):
    part = tail_partials(count)
    cursor = torch.tensor([cursor0], dtype=torch.int32, device="cuda")
    losses = torch.from_numpy(np.array(losses0, np.float32)).cuda()
    kw = {}
    if with_cursor:
        kw["cursor"] = cursor
    if with_partials:
        kw.update(loss_partials=torch.from_numpy(part).cuda(), losses=losses)
    got = _run(inp, 2, table, **kw)
    torch.cuda.synchronize()
    return got, int(cursor.item()), losses.cpu().numpy(), part


@pytest.mark.parametrize("variant", ["tiled", "linear"])
@pytest.mark.parametrize("shape", ["4x4", "eight"])
def test_step_tail_cursor_and_loss_fold(parity_log, shape, variant, monkeypatch):
    """step_tail in both kernels, on the smallest grids (element-wise on 20 parameters: ONE block, which is first and last; tiled: one tile
    + one block for the bias) and on the eight-weight table: the cursor advances by exactly 1 per call; losses += the partials' sums within
    the fold's depth -- ceil(count / 16) additions per slice, 4 butterfly levels, the += : (count / 16 + 5) 2^-24 sum |partials| -- and
    the same bits on a second identical call; the update itself is what it is without a tail; without a tail nothing is touched."""
    from open_duck_playground_amd import engine
    if variant == "linear":
        monkeypatch.setenv("ODK_ADAM_LINEAR", "1")
    entries, n = single_entries(4, 4, True) if shape == "4x4" else eight_entries()
    table = engine.WeightTable(entries)
    inp, ref = _case(n, "3x", 2)
    plain = _run(inp, 2, table)
    zeros = np.zeros(4, np.float32)
    for count in TAIL_COUNTS:
        got, cur, losses, part = _tail_call(table, inp, count, zeros, 41)
        want = part.astype(np.float64).sum(0)
        err = np.abs(losses.astype(np.float64) - want) / tail_bound(part)
        parity_log.check("update_kernels/loss_fold", dict(in_units_of_the_folds_depth=1.0), in_units_of_the_folds_depth=err.max())
        assert cur == 42
        assert all(np.array_equal(_bits(got[k]), _bits(plain[k])) for k in ("p", "m", "v", "pf", "pb")) and got["t"] == 2.0
        _, cur2, losses2, _ = _tail_call(table, inp, count, zeros, 41)
        assert cur2 == 42 and np.array_equal(_bits(losses2), _bits(losses))
        # on top of running sums: the += rounds at the new sum
        _, cur3, losses3, _ = _tail_call(table, inp, count, losses, cur)
        assert cur3 == 43
        assert np.all(np.abs(losses3.astype(np.float64) - (losses.astype(np.float64) + want)) <= tail_bound(part) + ulp32(losses3))
    before = np.array([1.5, -2.0, 0.25, 3.0], np.float32)
    _, cur, losses, _ = _tail_call(table, inp, 17, before, 7, with_cursor=False, with_partials=False)
    assert cur == 7 and np.array_equal(_bits(losses), _bits(before))
    _, cur, losses, _ = _tail_call(table, inp, 17, before, 7, with_partials=False)
    assert cur == 8 and np.array_equal(_bits(losses), _bits(before))
    _, cur, losses, part = _tail_call(table, inp, 17, before, 7, with_cursor=False)
    assert cur == 7 and not np.array_equal(_bits(losses), _bits(before))


# ---- 4. refusals: host-side checks, nothing is launched ----------------------------------------------------------------------------------------------

def test_bad_tables_and_buffers_are_refused_before_any_launch():
    from open_duck_playground_amd import engine
    entries, n = eight_entries()
    inp, _ = _case(n, "3x", 2)
    good = engine.WeightTable(entries)
    t = {k: torch.from_numpy(np.array(inp[k])).cuda() for k in ("p", "g", "m", "v")}
    t.update(acc=torch.zeros(engine.ADAM_ACC_FLOATS, device="cuda"), pf=torch.full((good.fwd_size + 8,), 3.0, device="cuda"),
             pb=torch.full((good.bwd_size + 8,), 3.0, device="cuda"))
    keep = {k: v.clone() for k, v in t.items()}

    def refused(table, n_par=n, nf=None, nb=None, pack=True, **tail):
        pf, pb = t["pf"][:nf or t["pf"].numel()], t["pb"][:nb or t["pb"].numel()]
        with pytest.raises(engine.OdkError):
            engine.adam_clip_packed(t["p"][:n_par], t["g"][:n_par], t["m"][:n_par], t["v"][:n_par], t["acc"], pf, pb, table, LR, MAX_NORM, **tail)
        if pack:
            with pytest.raises(engine.OdkError):
                engine.pack_weights(t["p"][:n_par], pf, pb, table)
        torch.cuda.synchronize()
        assert all(torch.equal(t[k], keep[k]) for k in t)

    with pytest.raises(engine.OdkError):                                       # nine weights: the table itself, and the library behind it
        engine.WeightTable(entries + [(n, 4, 4, True)])
    nine = engine.WeightTable(entries)
    nine.c.count = 9
    refused(nine)
    for field in ("fwd_off", "bwd_off"):                                       # a packed offset that is not a multiple of 4
        odd = engine.WeightTable(entries)
        getattr(odd.c, field)[1] += 2
        refused(odd)
    refused(good, n_par=n - 1)                                                 # the last weight ends past n
    refused(good, nf=good.fwd_size - 4)                                        # packed buffers shorter than the table asks for
    refused(good, nb=good.bwd_size - 4)
    part = torch.ones(17, 4, device="cuda")                                    # loss partials without losses
    refused(good, pack=False, loss_partials=part)
    refused(good, pack=False, loss_partials=part, cursor=torch.zeros(1, dtype=torch.int32, device="cuda"))
