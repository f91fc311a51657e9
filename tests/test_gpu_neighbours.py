"""Every env's results are independent of its wave neighbour: the same env with the same inputs stores the same BITS whoever shares its wave
and whichever slot it sits in.

At 32 lanes per env two envs share one wave and one LDS allocation and the env kernels let them interact on purpose (over forty ballot-guarded
branches, the height-field pair loop in which a row of env B works a prism of env A's foot, foot_foot_sat called by the whole wave, readlane
statics, the dead slot of an odd batch that re-runs the last env).  The oracle tests see a leak between partners only when it exceeds their
bounds at a typical state; here nothing is compared with an oracle and nothing has a tolerance: every stored array as uint32 words (NaN payloads
and the sign of zero count), across arrangements of the SAME subject beside neighbours of nine kinds -- itself, another ordinary state, a state
with overlapping feet, NaN in qpos, NaN in qvel, a joint velocity of 3e38, a base 1e5 m off the height field's grid, an upside-down robot, the
dead slot -- once in slot 0 and once in slot 1 (tests/neighbours_cases.py lays the batch out, tests/test_neighbours_host.py holds the layout).

The one sanctioned exception is modelled, not tolerated: `any_ffa` (csrc/odk_kernels.h) factors BOTH envs of a wave on the virtual tree when
EITHER has an active foot-foot row -- other arithmetic, other rounding.  So a subject's results fall into groups per forward pass -- plain / virtual,
decided from that pass's own debug image (neighbours_cases.env_flag) -- and the rule is bit equality WITHIN a group; contact_dist is computed
before the switch and must agree without exception.  The 64-lane instantiations (one env per wave) run the same batches as a control of the
machinery.  What was found and measured: profiles/neighbours/NOTES.md.

Every test arms a watchdog that ends the whole process when it is still running after LIMIT seconds (a hang: nothing more is started on the
GPU), and after a test that ended on an engine error the others of this file fail at once without a launch."""
import faulthandler
import time

import numpy as np
import pytest

import neighbours_cases as NC
from test_gpu_parity import torch_cuda  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

LIMIT = 120      # seconds per test: > 20 x the slowest measured on an MI355X (profiles/neighbours/NOTES.md); ends a hang, measures nothing
N_CHAIN = 10
STATE = ("qpos", "qvel", "warm")
DEBUG = ("sensordata", "actuator_force", "qacc")
_ended_badly = []


class _Guard:
    """the time limit of one test, and the latch that keeps the rest of the file off the GPU after an engine error"""

    def __enter__(self):
        assert not _ended_badly, f"not started: an earlier test of this file ended on an engine error ({_ended_badly[0]})"
        faulthandler.dump_traceback_later(LIMIT, exit=True)
        return self

    def __exit__(self, et, ev, tb):
        faulthandler.cancel_dump_traceback_later()
        if et is not None and issubclass(et, Exception) and not issubclass(et, AssertionError):
            _ended_badly.append(f"{et.__name__}: {ev}")
        return False


def _make(torch, name, config, A, P, **cfg_over):
    """the case's batch in one configuration, every per-env input following the env's pool row"""
    from open_duck_playground_amd import engine, randomize
    _, _, spec, lanes, _ = NC.case(name)
    cfg = NC._config(engine, spec, lanes, False, config)
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    b = engine.Batch(P["model"], A["nenv"], cfg)
    assert b.lanes_per_env == lanes, (name, b.lanes_per_env)
    keep = {}
    if config == "everything":
        from test_gpu_reward_terms import _all_terms
        I = NC.everything_inputs(P)
        src = A["src"]
        randomize.apply(b, {k: np.asarray(v)[src] for k, v in I["fields"].items()})
        b.set_reward_terms(_all_terms(P["model"]))
        keep = dict(cmd=torch.tensor(I["cmd"][src], device="cuda"), push=torch.tensor(I["push"][src], device="cuda"),
                    delay=torch.tensor(I["delay"][src], device="cuda"), action=torch.tensor(I["action"][src], device="cuda"))
        b.bind_commands(keep["cmd"]); b.bind_pushes(keep["push"]); b.bind_action_delays(keep["delay"])
    else:
        rng = np.random.default_rng(5)
        keep = dict(action=torch.tensor(rng.uniform(-1, 1, (len(P["qpos"]), P["model"].nu)).astype(np.float32)[A["src"]], device="cuda"))
    return b, keep


def _r0c(oracle_mod, P):
    """(first contact row of the kernels' row arrays: the rows before it are the friction-loss and limit rows, the oracle counts its equality rows
    first; an elliptic model's (mu of the foot-foot pair, impratio), else None)"""
    d = oracle_mod.OracleData(P["om"])
    d["qpos"][: P["om"].nq] = P["qpos"][0]
    d.forward()
    ell = P["name"] in NC.ELLIPTIC
    cone = (float(d["contact_friction"][8]), float(np.asarray(P["model"].a["opt_impratio"]).reshape(-1)[0])) if ell else None
    return d.i("nefc") - d.i("ne") - (36 if ell else 48), cone


def _flags(b, P, A, rows, name, check_rows):
    """per env: does it turn its wave to the virtual tree in the pass whose debug image the batch holds (neighbours_cases.env_flag)"""
    img = b.lds_image()
    o_cd, o_D, o_jar = b.lds_offset("contact_dist"), b.lds_offset("efc_D"), b.lds_offset("jar")
    r0c, cone = rows
    ell = cone is not None
    flags = []
    for e in range(A["nenv"]):
        cd = img[e, o_cd: o_cd + 12]
        D, jar = img[e, o_D + r0c + 32: o_D + r0c + 48], img[e, o_jar + r0c + 32: o_jar + r0c + 48]
        flags.append(NC.env_flag(cd, D, jar, cone))
        if check_rows and A["sid"][e] >= 0:      # the rows read ARE the foot-foot rows: a row has D > 0 exactly when its contact penetrates
            assert np.isfinite(cd).all() and np.isfinite(D).all(), (name, e)
            rows_on = int((D.reshape(4, 4)[:, 0] > 0).sum()) if ell else int((D > 0).sum()) // 4      # (elliptic: the normal row; its fourth lane has no row)
            assert rows_on == int((cd[8:12] < 0).sum()) and (ell or int((D > 0).sum()) % 4 == 0), (name, e, cd[8:12].tolist(), D.tolist())
    return flags


def _keys(flags, A, lanes, name):
    """the group of every env in one pass; at 64 lanes (one env per wave: the control) there is ONE group"""
    if lanes != 32:
        return ["alone"] * A["nenv"]
    return NC.wave_keys(flags, A["nenv"], lanes, name in NC.ALWAYS_VIRTUAL, A["src"])


def _own(flags):
    """an env's own flag as an array: made of its own data before the switch, so it is held to the rule like contact_dist"""
    return np.array([("no", "yes", "unknown").index(f) for f in flags], np.int32)


def _report(parity_log, tag, bad, sizes):
    print(tag, "occurrences (plain, virtual, undecided) per pass:", sizes, "mismatches:", len(bad))
    for line in bad[:20]:
        print("  ", line)
    parity_log.rec(tag, plain=max(s[0] for s in sizes), virtual=max(s[1] for s in sizes), undecided=max(s[2] for s in sizes))
    parity_log.check(tag, dict(mismatches=0), mismatches=len(bad))


@pytest.mark.parametrize("config", NC.ENV_CONFIGS)
@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_physics_kernels(torch_cuda, oracle_mod, parity_log, name, config):
    """Leg P.  physics_step(ctrl, 1) ten times in a row; after each launch: contact_dist of every subject agrees across all arrangements that entered
    the launch with the same state (all of them at the first), and qpos, qvel, warm, sensordata, actuator_force, qacc agree within the subject's
    group, the group being the history of the wave's plain / virtual passes so far.  Then one physics_step(ctrl, 10) from the start state equals the
    tenth chained launch wherever the wave stayed plain throughout.  Every duck case must have a non-empty virtual group."""
    torch = torch_cuda
    t0 = time.time()
    with _Guard():
        P = NC.pools(oracle_mod, name)
        A = NC.arrangement(P)
        lanes = NC.case(name)[3]
        b, keep = _make(torch, name, config, A, P)
        try:
            r0c = _r0c(oracle_mod, P)
            ctrl = torch.tensor(P["ctrl"][A["src"]], dtype=torch.float32, device="cuda")
            b.set_state(A["qpos"], A["qvel"], A["warm"])
            n = A["nenv"]
            hist = [()] * n
            bad, sizes = [], []
            last = None
            for t in range(N_CHAIN):
                b.physics_step(ctrl, 1)
                torch.cuda.synchronize()
                dbg = b.get_debug()
                q, v, w = b.get_state()
                flags = _flags(b, P, A, r0c, name, t == 0)
                keys = _keys(flags, A, lanes, name)
                entered = hist
                hist = [h + (k,) for h, k in zip(hist, keys)]
                bad += NC.mismatches(A, entered, dict(contact_dist=dbg["contact_dist"], own_flag=_own(flags)), f"launch {t}: ")
                last = dict(qpos=q, qvel=v, warm=w, **{k: dbg[k] for k in DEBUG})
                bad += NC.mismatches(A, hist, last, f"launch {t}: ")
                sizes.append(NC.group_sizes(A, keys))
            # ten substeps in ONE launch from the start state against the tenth chained launch, wherever every pass of the wave was plain
            b.set_state(A["qpos"], A["qvel"], A["warm"])
            b.physics_step(ctrl, N_CHAIN)
            torch.cuda.synchronize()
            dbg = b.get_debug()
            q, v, w = b.get_state()
            one = dict(qpos=q, qvel=v, warm=w, **{k: dbg[k] for k in DEBUG})
            plain = [e for e in range(n) if A["sid"][e] >= 0 and all(k in ("P", "alone") or name in NC.ALWAYS_VIRTUAL for k in hist[e])]
            assert len(plain) >= NC.N_ORD, (name, len(plain))
            for k in one:
                wa, wb = NC.bits(last[k]), NC.bits(one[k])
                for e in plain:
                    if not np.array_equal(wa[e], wb[e]):
                        bad.append(f"ten substeps in one launch != ten launches: {k} env {e} (subject {A['sid'][e]}, beside {A['kind'][e]})")
        finally:
            b.close()
        if lanes == 32:
            assert sizes[0][1] > 0, f"{name}: no subject in the virtual group at the first launch {sizes[0]}"
        if lanes == 32 and name not in NC.ALWAYS_VIRTUAL:
            assert sizes[0][0] > 0, f"{name}: no subject in the plain group {sizes[0]}"
        _report(parity_log, f"neighbours/physics/{name}/{config}", bad, sizes)
    print(f"{name}/{config}: {A['nenv']} envs, {len(A['subjects'])} subjects, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("config", NC.ENV_CONFIGS)
@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_step_kernel_one_substep(torch_cuda, oracle_mod, parity_log, name, config):
    """Leg S1.  The product step kernel (n_substeps = 1, autoreset off; its forward pass is the hot-constant instantiation, which the physics kernel
    does not run) on the same arrangements: records made of a donor row (RNG key, counters, info: the reset record of the env's pool row) with
    qpos, qvel, warm replaced by the constructed state.  obs, priv, reward, done, truncation, metrics, xmetrics and the records agree within the
    group of the step's single pass, which a debug-image replay of the same step decides."""
    torch = torch_cuda
    from lds_poison_driver import _snapshot
    with _Guard():
        P = NC.pools(oracle_mod, name)
        A = NC.arrangement(P)
        lanes = NC.case(name)[3]
        b, keep = _make(torch, name, config, A, P, n_substeps=1, autoreset=0)
        L = b.L
        try:
            r0c = _r0c(oracle_mod, P)
            nq, nv = P["model"].nq, P["model"].nv
            L.odk_set_debug_dump(0)
            b.reset(seed=21)
            rec = b.records()[A["src"]].copy()
            rec[:, :nq] = A["qpos"]; rec[:, nq: nq + nv] = A["qvel"]; rec[:, nq + nv: nq + 2 * nv] = A["warm"]
            b.set_records(rec)
            b.step(keep["action"])
            torch.cuda.synchronize()
            out = _snapshot(b)
            b.set_records(rec)
            L.odk_set_debug_dump(1)      # the same step again, by the kernel that leaves the debug image
            b.step(keep["action"])
            torch.cuda.synchronize()
            flags = _flags(b, P, A, r0c, name, False)
            keys = _keys(flags, A, lanes, name)
        finally:
            L.odk_set_debug_dump(0)
            b.close()
        done = out["done"][A["sid"] >= 0]
        assert np.isfinite(out["obs"][A["sid"] >= 0]).all() and np.isfinite(out["reward"][A["sid"] >= 0]).all()
        planted = {k: out["done"][(A["kind"] == k) & (A["sid"] < 0)] for k in ("nan_qpos", "nan_qvel", "upside_down")}
        assert all(len(v) and (v == 1).all() for v in planted.values()), {k: v.tolist() for k, v in planted.items()}      # (the neighbours did what they were planted for)
        bad = NC.mismatches(A, keys, out) + NC.mismatches(A, [()] * A["nenv"], dict(own_flag=_own(flags)))
        _report(parity_log, f"neighbours/step1/{name}/{config}", bad, [NC.group_sizes(A, keys)])
        print(f"{name}/{config}: done among the subjects {int(done.sum())} of {len(done)}")


def _dist_replay(b, L, rec, act, envs):
    """contact_dist[8:12] of the given envs in a debug-image replay of one step from the records `rec`"""
    b.set_records(rec)
    L.odk_set_debug_dump(1)
    try:
        b.step(act)
        b.torch.cuda.synchronize()
        cd = b.get_debug()["contact_dist"]
    finally:
        L.odk_set_debug_dump(0)
    return {int(e): cd[e, 8:12].tolist() for e in envs if 0 <= e < b.nenv}


# Seed of a case's rollout (reset and actions).  The duck's feet do not meet in random-action rollouts; the robots' do, and a stream whose partner's
# feet overlap is factored on the virtual tree in one batch and not in the other -- the sanctioned exception, which this leg has no group for.  A
# rollout whose only mismatch is that switch gets another seed, recorded here and in profiles/neighbours/NOTES.md.
S10_SEEDS = {"D-32": 23, "E-32": 40}      # (21 and 22 end in the switch: profiles/neighbours/NOTES.md)
S10_SEED = 21
# tests/assets/tail_biped_equality.xml pins a foot to the world and its feet meet within two steps of EVERY rollout (seeds 21 .. 80 tried).  For this case
# a stream leaves the comparison from the step on at which an env of its wave -- in W or in S -- has a negative foot-foot distance in ANY of the step's
# ten forward passes (the necessary condition of the switch: a superset of it), read from debug-image replays of the step's first k substeps, k = 1 .. 10
# (the last pass alone misses feet that meet and part inside one step: measured, stream 28 of seed 21 at step 10).  The others are held to the rule as
# everywhere; at least S10_COMPARED_MIN stream-steps (five whole steps' worth) must have been compared.
S10_TAINT = ("C-32-equality",)
S10_COMPARED_MIN = 5 * 32


def _rollout(torch, name, seed):
    """-> (facts, None) or (facts, the first mismatch with the foot-foot distances of a debug-image replay of that step)"""
    from open_duck_playground_amd import engine, randomize
    from lds_poison_driver import _snapshot
    from test_gpu_reward_terms import _all_terms
    _, _, spec, lanes, _ = NC.case(name)
    model = NC._model(spec)
    nW = 33
    fields, _ = randomize.domain_randomize(model, np.random.default_rng(17), nW)
    rng = np.random.default_rng(3)
    cmd = np.zeros((nW, 7), np.float32)
    cmd[:, :3] = rng.uniform(-0.2, 0.2, (nW, 3)); cmd[:, 3:] = rng.uniform(-0.5, 0.5, (nW, 4)); cmd[nW - 1] = 0.0
    delay = rng.integers(-1, 3, nW).astype(np.int32)
    batches = []
    facts = dict(trunc=0, done=0, nan_done=0, clean=nW - 1, compared=0)
    taint = name in S10_TAINT and lanes == 32
    clean = np.ones(nW - 1, bool)      # stream j + 1 (W env j + 1, S env j) is still compared
    try:
        for off in (0, 1):
            b = engine.Batch(model, nW - off, NC._config(engine, spec, lanes, False, "everything"))
            assert b.lanes_per_env == lanes
            randomize.apply(b, {k: np.asarray(v)[off:] for k, v in fields.items()})
            b.set_reward_terms(_all_terms(model))
            t_cmd, t_push, t_delay = torch.tensor(cmd[off:], device="cuda"), torch.zeros(nW - off, 2, device="cuda"), torch.tensor(delay[off:], device="cuda")
            b.bind_commands(t_cmd); b.bind_pushes(t_push); b.bind_action_delays(t_delay)
            batches.append((b, t_push, (t_cmd, t_delay)))
        (W, pW, _), (S, pS, _) = batches
        L = W.L
        L.odk_set_debug_dump(0)
        W.reset(seed=seed, env_id_offset=0); S.reset(seed=seed, env_id_offset=1)
        torch.cuda.synchronize()
        gen = torch.Generator(device="cuda").manual_seed(seed + 7)

        def compare(label, prev, act):
            a, c = _snapshot(W), _snapshot(S)
            for k in a:
                wa, wc = NC.bits(a[k][1:])[clean], NC.bits(c[k])[clean]
                if not np.array_equal(wa, wc):
                    j = int(np.flatnonzero(clean)[np.flatnonzero((wa != wc).any(axis=1))[0]])
                    wa, wc = NC.bits(a[k][1:]), NC.bits(c[k])
                    msg = f"{name} seed {seed} {label}: {k} of stream {j + 1} (W env {j + 1} slot {(j + 1) & 1}, S env {j} slot {j & 1}) differs in {int((wa[j] != wc[j]).sum())} words"
                    if prev is not None:      # contact_dist[8:12] of both waves' envs in a debug-image replay of this step
                        dW = _dist_replay(W, L, prev[0], act, (j + 1, (j + 1) ^ 1))
                        dS = _dist_replay(S, L, prev[1], act[1:].contiguous(), (j, j ^ 1))
                        msg += f"; foot-foot distances of the replayed step: W {dW}, S {dS}"
                    return a, msg
            return a, None
        _, msg = compare("reset", None, None)
        for t in range(30):
            if msg:
                break
            for p in (pW, pS):
                p.zero_()
                if t in (3, 9):
                    p[:, 0] = 0.3
            pW[::2, 1] = -0.2 if t in (3, 9) else 0.0
            pS[1::2, 1] = -0.2 if t in (3, 9) else 0.0      # (stream j + 1 = S's env j)
            if t == 16:      # the rest of the run on the sampled push
                W.bind_pushes(None); S.bind_pushes(None)
            if t == 12:      # a NaN into qvel of streams 5 and 10: their partners differ between W (4, 11) and S (6, 9)
                for b_, off in ((W, 0), (S, 1)):
                    q, v, w = b_.get_state()
                    v[5 - off, 7] = np.nan; v[10 - off, 9] = np.nan
                    b_.set_state(q, v, w)
            prev = (W.records(), S.records())
            act = torch.empty(nW, model.nu, device="cuda").uniform_(-1, 1, generator=gen)
            if taint:      # this step's first k substeps by the debug-image kernel: which envs' feet overlap in pass k; then config and records put back
                fW, fS = np.zeros(nW, bool), np.zeros(nW - 1, bool)
                for k in range(1, 11):
                    for b_ in (W, S):
                        b_.cfg.n_substeps = k; b_.set_config(b_.cfg)
                    with np.errstate(invalid="ignore"):
                        fW |= np.fmin.reduce(np.array(list(_dist_replay(W, L, prev[0], act, range(nW)).values())), axis=1) < 0
                        fS |= np.fmin.reduce(np.array(list(_dist_replay(S, L, prev[1], act[1:].contiguous(), range(nW - 1)).values())), axis=1) < 0
                assert W.cfg.n_substeps == 10 and S.cfg.n_substeps == 10
                W.set_records(prev[0]); S.set_records(prev[1])
                for j in range(nW - 1):
                    pw, ps = NC.partner(j + 1, nW, 32), NC.partner(j, nW - 1, 32)
                    if fW[j + 1] or fW[pw] or fS[j] or fS[ps]:
                        clean[j] = False
                facts["clean"] = int(clean.sum())
            W.step(act); S.step(act[1:].contiguous())
            torch.cuda.synchronize()
            a, msg = compare(f"step {t}", prev, act)
            facts["compared"] += int(clean.sum())
            facts["trunc"] += int(a["truncation"].sum()); facts["done"] += int(a["done"].sum())
            if t == 12:
                facts["nan_done"] = int(a["done"][5] + a["done"][10])
            for k in ("obs", "reward", "qpos", "qvel"):
                assert np.isfinite(a[k]).all(), (name, t, k)
    finally:
        for b, *_ in batches:
            b.close()
    return facts, msg


@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_product_rollout_shifted_by_one_slot(torch_cuda, oracle_mod, parity_log, name):
    """Leg S10.  The reset and step kernels as shipped (10 substeps, autoreset on), everything on (and bound action delays): batch W has 33 envs at
    env_id_offset 0, batch S 32 envs at offset 1 with W's input rows [1:], so env j of S is env j + 1 of W in the OTHER slot beside ANOTHER
    partner (W's last env sits beside the dead slot, in S beside a live one).  30 random-action steps with episodes of 8 (truncations and falls
    auto-reset), a NaN set into qvel of two streams mid-run: every stored array of every common stream agrees at the reset and after every
    step.  No exception in this leg (S10_SEEDS)."""
    with _Guard():
        facts, msg = _rollout(torch_cuda, name, S10_SEEDS.get(name, S10_SEED))
        assert msg is None, msg
        assert facts["trunc"] > 0 and facts["done"] > facts["trunc"] and facts["nan_done"] == 2, facts
        assert facts["compared"] >= (S10_COMPARED_MIN if name in S10_TAINT and NC.case(name)[3] == 32 else 30 * 32), facts
        parity_log.check(f"neighbours/rollout/{name}", dict(mismatches=0), mismatches=0)
        print(name, facts)
