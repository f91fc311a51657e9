"""One family of LDS-using kernels on whatever library ODK_LIB names, every output stored (tests/test_gpu_lds_poison.py runs it twice --
libodk.so, then libodk_poison.so, whose kernels start from NaN-filled LDS: csrc/odk_poison.h -- and compares the two files bit for bit).

    python tests/lds_poison_driver.py --family env|learner --out FILE.npz [--only NAME-PREFIX]

Not collected by pytest.  The case tables below are module-level data: tests/test_lds_poison_host.py reads them without a GPU.

env: every compiled (shape, lanes, floor) instantiation of csrc/odk_shapes.h's ODK_ENV_SET_* lines, reached the way the GPU tests reach it
(task model, lanes_per_env, opt_cone, primitive feet, a robot's xml), NENV = 5 envs (three workgroups at 32 lanes, the last with a dead slot),
with the defaults and with everything on; per configuration reset, 24 product steps, one step at the command-resample point, 3 debug-image
steps, physics_step 1 and 10.  learner: the suite's own float64 checks (check_fused_mlp, the head / GAE / update bodies of
tests/test_gpu_learner*.py and test_gpu_update_sizes.py, at their own bounds) run with a recorder around every engine call that launches a
kernel with LDS; a check that fails under the poison library is stored as such and the run goes on.

Keys: <run>/<array>.  `<run>/refused` holds the message of a configuration the library refused (OdkError); `.../nan_words` (the NaN words
of the debug image after each dumped launch) and arrays marked `@unordered` (loss sums folded by float atomics, whose order is not fixed)
are stored for the test to read, not to compare bit for bit."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

NENV = 5
N_STEPS, N_DUMPED = 24, 3
DUCK_HEAD = [5, 6, 7, 8]

# (name, kernel-set triple it reaches, how the model is made, lanes per env, also run Standing).  model: a task name, ("cone", task) = the
# task's model with opt_cone = 1, ("prim", task, kinds) = sphere / capsule feet (tests/test_gpu_parity.py), or a robot's xml under tests/assets.
ENV_CASES = [
    ("A-32", ("A", 32, 0), "flat_terrain", 32, True),
    ("A-64", ("A", 64, 0), "flat_terrain", 64, True),
    ("B-32-plane", ("B", 32, 0), "flat_terrain_backlash", 32, True),
    ("B-32-hfield-hull", ("B", 32, 1), "rough_terrain_backlash", 32, True),
    ("B-32-hfield-prim", ("B", 32, 2), ("prim", "rough_terrain_backlash", ("capsule", "sphere")), 32, False),
    ("B-64", ("B", 64, 0), "flat_terrain_backlash", 64, True),
    ("AE-32", ("AE", 32, 0), ("cone", "flat_terrain"), 32, False),
    ("BE-32-plane", ("BE", 32, 0), ("cone", "flat_terrain_backlash"), 32, False),
    ("BE-32-hfield", ("BE", 32, 1), ("cone", "rough_terrain_backlash"), 32, False),
    ("C-32", ("C", 32, 0), "tail_biped.xml", 32, True),
    ("C-32-equality", ("C", 32, 0), "tail_biped_equality.xml", 32, False),
    ("C-32-loop", ("C", 32, 0), "tail_biped_loop.xml", 32, False),
    ("D-32", ("D", 32, 0), "biped12.xml", 32, True),
    ("E-32", ("E", 32, 0), "biped_arms.xml", 32, True),
]
ENV_CONFIGS = ("defaults", "everything")
# user shapes (csrc/odk_shapes_user.h, written by tools/new_shape.py --add: sets U<k>) are not part of a plain build and are not covered
NOT_COVERED = "U<k>"

FINITE = ("obs", "priv", "reward", "done", "truncation", "metrics", "xmetrics", "qpos", "qvel", "warm")

# learner cases: (name, module, function, args).  `PLOG` / `MONKEY` stand for the parity log and a monkeypatch of the driver's own.
PLOG, MONKEY = "<parity_log>", "<monkeypatch>"
LEARNER_CASES = (
    [(f"mlp/rows={n}", "test_learner_sizes_host", "check_fused_mlp", (n, 101, 28)) for n in (1, 15, 17, 77)]
    # the boundary rows of the size table (tests/test_learner_sizes_host.py: BOUNDARY_N_IN x BOUNDARY_N_OUT), row counts from MLP_ROWS in turn
    + [(f"mlp/boundary/{i}x{o}", "test_learner_sizes_host", "check_fused_mlp", ((5, 16, 77, 320)[(a + b) % 4], i, o))
       for a, i in enumerate((5, 16, 96, 224)) for b, o in enumerate((1, 16, 17, 32))]
    + [("mlp/two_networks", "test_gpu_learner_sizes", "test_two_networks_in_one_launch_at_other_sizes", ("biped12", "joystick", (77, 85)))]
    + [("dw_gemm", "test_gpu_learner", "test_dw_gemm_matches_torch_mm_and_is_reproducible", ())]
    + [(f"gae/{B}x{T}", "test_gpu_learner", "test_gae_kernel_matches_torch_reference", (B, T)) for B, T in ((256, 20), (37, 5), (300, 20), (1200, 40))]
    + [("gae/1x1", "lds_poison_driver", "gae_one_by_one", ())]
    + [(f"gae_head/A={A}/{B}x{T}/{kind}", "test_gpu_learner_sizes", "test_fused_gae_head_matches_float64", (A, B, T, kind))
       for A, B, T, kind in ((14, 256, 20, "crafted"), (16, 37, 5, "random"), (1, 3, 7, "crafted"))]
    + [(f"ppo_head/A={A}/n={n}/{kind}", "test_gpu_learner_sizes", "test_ppo_head_matches_float64", (A, n, kind))
       for A, n, kind in ((14, 77, "crafted"), (16, 640, "random"), (1, 77, "random"))]
    + [(f"adam/plain/n={n}", "test_gpu_update_sizes", "test_adam_clip_matches_float64", (PLOG, n)) for n in (5, 1025)]
    + [(f"adam/tiled/{r}x{c}", "test_gpu_update_sizes", "test_one_weight_and_its_bias", (PLOG, r, c, True)) for r, c in ((17, 65), (5, 3))]
    + [(f"adam/eight/{v}", "test_gpu_update_sizes", "test_eight_weights", (PLOG, v, MONKEY)) for v in ("tiled", "linear")]
    + [(f"colsum/rows={n}", "lds_poison_driver", "colsum_width_30", (n,)) for n in (65, 130)]
    + [(f"moments/{r}x{w}", "lds_poison_driver", "moments", (r, w)) for r, w in ((33, 70), (4097, 7))]
)


# ---- env family ----------------------------------------------------------------------------------------------------------------------

def _model(spec):
    from open_duck_playground_amd.model import Model, load_task_model
    if isinstance(spec, tuple) and spec[0] == "cone":
        m = load_task_model(spec[1])
        return Model({**m.a, "opt_cone": np.array([1], np.int32)})
    if isinstance(spec, tuple) and spec[0] == "prim":
        from test_gpu_parity import _prim_feet_variant
        return _prim_feet_variant(spec[1], spec[2])
    if spec.endswith(".xml"):
        return Model.from_xml(os.path.join(HERE, "assets", spec), sim_dt=0.002)
    return load_task_model(spec)


def _snapshot(b):
    qpos, qvel, warm = b.get_state()
    out = {k: getattr(b, k).cpu().numpy().copy() for k in ("obs", "priv", "reward", "done", "truncation", "metrics")}
    if b.xmetrics is not None:
        out["xmetrics"] = b.xmetrics.cpu().numpy().copy()
    out.update(qpos=qpos.copy(), qvel=qvel.copy(), warm=warm.copy(), records=b.records().copy())
    return out


def _config(engine, spec, lanes, standing, config):
    """The env config of one configuration (tests/neighbours_cases.py runs the same two): "defaults", or "everything" = noise, sampled
    pushes every 5 .. 15 env steps, episodes of 8 steps, the duck's imitation reward (the bound rows, the DR rows and the reward terms
    are the caller's: _run_env below)."""
    robot = isinstance(spec, str) and spec.endswith(".xml")
    cfg = engine.default_config(standing)
    cfg.lanes_per_env = lanes
    if robot:
        cfg.use_imitation = 0
    if config == "everything":
        cfg.noise_level = 1.0
        cfg.push_enable = 1.0
        cfg.push_interval_range[0] = 0.1; cfg.push_interval_range[1] = 0.3      # a sampled push every 5 .. 15 env steps
        cfg.episode_length = 8
        if not robot and not standing:
            cfg.use_imitation = 1
    return cfg


def _run_env(torch, engine, spec, lanes, standing, config):
    """One configuration -> ({array name: [launch, ...] stack}, launch labels, facts for the product run's own assertions)."""
    from open_duck_playground_amd import randomize
    model = _model(spec)
    robot = isinstance(spec, str) and spec.endswith(".xml")
    cfg = _config(engine, spec, lanes, standing, config)
    everything = config == "everything"
    b = engine.Batch(model, NENV, cfg)
    L = engine.load_library()
    n, nu = NENV, model.nu
    cmd = push = None
    try:
        if standing and robot:
            b.set_head_joints(DUCK_HEAD)
        if everything:
            fields, _ = randomize.domain_randomize(model, np.random.default_rng(17), n)
            randomize.apply(b, fields)
            from test_gpu_reward_terms import _all_terms
            b.set_reward_terms(_all_terms(model))
            rng = np.random.default_rng(3)
            rows = np.zeros((n, 7), np.float32)
            rows[:, :3] = rng.uniform(-0.2, 0.2, (n, 3)); rows[:, 3:] = rng.uniform(-0.5, 0.5, (n, 4)); rows[n - 1] = 0.0
            cmd = torch.tensor(rows, device="cuda")
            push = torch.zeros(n, 2, device="cuda")
            b.bind_commands(cmd); b.bind_pushes(push)
        gen = torch.Generator(device="cuda").manual_seed(7)
        act = torch.empty(n, nu, device="cuda")
        stacks, labels, nan_words = {}, [], []
        facts = dict(trunc=0, done=0, pushed=0)

        def store(label, dumped):
            torch.cuda.synchronize()
            for k, v in _snapshot(b).items():
                stacks.setdefault(k, []).append(v)
            labels.append(label)
            nan_words.append(int(np.isnan(b.lds_image()).sum()) if dumped else -1)
            facts["trunc"] += int(b.truncation.sum()); facts["done"] += int(b.done.sum())
            facts["pushed"] += int((np.abs(b.info()["push"]).sum(axis=1) > 0).sum())

        L.odk_set_debug_dump(0)
        b.reset(seed=21)
        store("reset", False)
        for t in range(N_STEPS):      # the product step kernel
            if everything:
                push.zero_()
                if t in (3, 9):
                    push[:, 0] = 0.3; push[::2, 1] = -0.2
                if t == 16:           # the rest of the run on the sampled push
                    b.bind_pushes(None)
            act.uniform_(-1, 1, generator=gen)
            b.step(act)
            store(f"step{t}", False)
        I = b.info()                  # the step that takes info["step"] past 500 resamples the command (tests/test_gpu_env.py)
        I["step"][:] = 500
        b.set_records(I["_records"])
        act.uniform_(-1, 1, generator=gen)
        b.step(act)
        store("resample", False)
        L.odk_set_debug_dump(1)
        for t in range(N_DUMPED):     # step_kernel_dbg
            act.uniform_(-1, 1, generator=gen)
            b.step(act)
            store(f"dumped{t}", True)
        ctrl = torch.tensor(np.asarray(model.a["key_ctrl"], np.float32).reshape(-1)[:nu][None].repeat(n, 0), device="cuda")
        for nsub in (1, 10):
            b.physics_step(ctrl, nsub)
            store(f"physics{nsub}", True)
    finally:
        L.odk_set_debug_dump(0)
        b.close()
    out = {k: np.stack(v) for k, v in stacks.items()}
    out["nan_words"] = np.array(nan_words, np.int64)
    out["launches"] = np.array(labels)
    return out, facts


def run_env(out, product, only=""):
    import torch
    from open_duck_playground_amd import engine
    for name, _, spec, lanes, standing in ENV_CASES:
        if not name.startswith(only):
            continue
        for config, stand in [(c, False) for c in ENV_CONFIGS] + ([("standing", True)] if standing else []):
            run = f"{name}/{config}"
            t0 = time.time()
            try:
                arrays, facts = _run_env(torch, engine, spec, lanes, stand, config)
            except engine.OdkError as e:
                out[f"{run}/refused"] = np.array(str(e))
                print(f"{run}: refused: {e}", flush=True)
                continue
            for k, v in arrays.items():
                out[f"{run}/{k}"] = v
            print(f"{run}: {len(arrays['launches'])} launches, NaN words of the dumped images {arrays['nan_words'][arrays['nan_words'] >= 0].tolist()}, "
                  f"{time.time() - t0:.2f} s", flush=True)
            if product:
                for k in FINITE:
                    if k in arrays:
                        assert np.isfinite(arrays[k]).all(), (run, k)
                if config == "everything":
                    assert facts["trunc"] > 0 and facts["done"] > 0 and facts["pushed"] > 0, (run, facts)


# ---- learner family ------------------------------------------------------------------------------------------------------------------

def gae_one_by_one():
    """odk_gae at (1, 1): one trajectory of one step, against gae_reference (float64) at the bounds of test_gae_kernel_matches_torch_reference;
    the advantage statistics of a single sample are mean = the sample, 1 / (0 + 1e-8)."""
    import torch
    from open_duck_playground_amd import engine
    from test_learner_sizes_host import gae_reference
    rew, val, boot = torch.tensor([[0.7]], device="cuda"), torch.tensor([[-0.4]], device="cuda"), torch.tensor([1.3], device="cuda")
    zero = torch.zeros(1, 1, device="cuda")
    stats = torch.zeros(2, device="cuda")
    vs, adv = engine.gae(zero, zero, rew, val, boot, 0.95, 0.97, stats=stats)
    r = gae_reference(zero.cpu(), zero.cpu(), rew.cpu(), val.cpu(), boot.cpu(), 0.95, 0.97)
    vs_ref, adv_ref = r[0], r[1]
    torch.testing.assert_close(vs.cpu().double(), vs_ref.reshape(1, 1).double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(adv.cpu().double(), adv_ref.reshape(1, 1).double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(stats[0].cpu().double(), adv_ref.double().mean(), rtol=1e-4, atol=1e-5)
    assert float(stats[1]) == float(np.float32(1.0) / np.float32(1e-8))


def colsum_width_30(n):
    """odk_silu_bwd_colsum / odk_colsum_partial / odk_colsum_finalize at width 30 (less than the 64-column block) with n rows (65, 130: a
    ragged second / third 64-row tile) against float64.  Bounds: dz = dh s (1 + x (1 - s)) with s from one __expf (argument |x| < 6: its
    exp2 argument carries |x| log2(e) 2^-24 < 6e-7, the result an ulp or two more), one division and five more float32 roundings, each
    below 6e-8 of its own result: against the sum of magnitudes M = |dh| s (1 + |x| (1 - s)) -- not against dz itself, which cancels to
    zero near x = -1.28 -- that is < 2e-6 M; asserted at 4e-6 M.  A column sum of n <= 130 float32 terms in a fixed tree is within
    n 2^-24 sum|terms| < 1e-5 sum|terms|."""
    import torch
    from open_duck_playground_amd import engine
    g = torch.Generator(device="cuda").manual_seed(n)
    w, tiles = 30, (n + 63) // 64
    dh, z, x = (torch.randn(n, w, device="cuda", generator=g) for _ in range(3))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    dz, p_dz, p_x, cs_dz, cs_x, cs_one = nan(n, w), nan(tiles * w), nan(tiles * w), nan(w), nan(w), nan(w)
    engine.silu_bwd_colsum(dh, z, dz, None, p_dz)
    engine.colsum_partial(x, p_x)
    engine.ColsumFinalize([(p_dz, cs_dz), (p_x, cs_x)], n)()
    engine.silu_bwd_colsum(dh, z, nan(n, w), cs_one, nan(tiles * w))      # the single-layer form folds in the same call
    sg = torch.sigmoid(z.double())
    ref = dh.double() * sg * (1 + z.double() * (1 - sg))
    mag = dh.double().abs() * sg * (1 + z.double().abs() * (1 - sg))
    assert bool(((dz.double() - ref).abs() <= 4e-6 * mag).all())
    for got, terms in ((cs_dz, ref), (cs_x, x.double()), (cs_one, ref)):
        assert bool(((got.double() - terms.sum(0)).abs() <= 1e-5 * terms.abs().sum(0)).all())


def moments(rows, w):
    """odk_col_moments + odk_moments_update at (rows, w), against float64 at the bounds of test_col_moments_kernel_matches_float64_torch."""
    import torch
    from open_duck_playground_amd import engine
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = (torch.randn(rows, w, device="cuda", generator=g) * 3 + 1.5).contiguous()
    s, s2 = engine.col_moments(x)
    xd = x.double()
    torch.testing.assert_close(s, xd.sum(0), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(s2, (xd * xd).sum(0), rtol=1e-12, atol=1e-9)
    count = torch.tensor(10.0, dtype=torch.float64, device="cuda")
    mean, sv, sd = torch.full((w,), 0.25, device="cuda"), torch.full((w,), 40.0, device="cuda"), torch.ones(w, device="cuda")
    engine.running_stats_update(x, count, mean, sv, sd, 1e-6, 1e6)
    nr, c1 = float(rows), 10.0 + rows
    m0 = torch.full((w,), 0.25, dtype=torch.float64, device="cuda")
    m1 = m0 + (xd.sum(0) / nr - m0) * (nr / c1)
    v1 = 40.0 + ((xd * xd).sum(0) - xd.sum(0) * (m0 + m1) + nr * m0 * m1)
    assert float(count) == c1
    torch.testing.assert_close(mean, m1.float(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(sv, v1.float(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(sd, torch.sqrt(v1 / c1).float().clamp(1e-6, 1e6), rtol=1e-6, atol=1e-7)


class Recorder:
    """Wraps every engine entry that launches a learner kernel with LDS: after the call, every CUDA tensor among its arguments, its result and
    what the op object keeps is stored (inputs too: they must agree as well)."""
    FUNCS = ("gae", "ppo_head", "adam_clip", "silu_bwd_colsum", "colsum_partial", "pack_weights", "adam_clip_packed", "col_moments",
             "running_stats_update")
    METHODS = (("ColsumFinalize", "__call__"), ("DwGemm", "__call__"), ("GaeHead", "__call__"), ("ColsumFold", "__call__"), ("FusedMLP", "forward"),
               ("FusedMLP", "backward"))

    def __init__(self, torch, engine, out):
        self.torch, self.out, self.case, self.calls = torch, out, "", 0
        for f in self.FUNCS:
            setattr(engine, f, self._wrap(getattr(engine, f), f))
        for cls, m in self.METHODS:
            setattr(getattr(engine, cls), m, self._wrap(getattr(getattr(engine, cls), m), f"{cls}.{m.strip('_')}"))

    def _tensors(self, obj, path, found, seen):
        torch = self.torch
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda and id(obj) not in seen:
                seen.add(id(obj)); found.append((path, obj))
        elif isinstance(obj, dict):
            for k, v in obj.items():
                self._tensors(v, f"{path}.{k}", found, seen)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                self._tensors(v, f"{path}.{i}", found, seen)
        elif hasattr(obj, "keep"):
            self._tensors(obj.keep, path + ".keep", found, seen)
            self._tensors(getattr(obj, "keep_finish", None), path + ".keep_finish", found, seen)

    def _wrap(self, fn, name):
        def wrapped(*a, **k):
            r = fn(*a, **k)
            self.torch.cuda.synchronize()
            found = []
            self._tensors([a, k, r], "", found, set())
            # loss sums that workgroups add with float atomics: the head launch's `losses`, the fused launch's when it has no partials buffer
            atomics = name == "ppo_head" or (name == "GaeHead.call" and a[0].keep[-1] is None)
            for path, t in found:
                tag = "@unordered" if atomics and t.numel() == 4 and t.dtype == self.torch.float32 else ""
                self.out[f"{self.case}/{self.calls:03d}.{name}{path}{tag}"] = t.detach().cpu().numpy().copy()
            self.calls += 1
            return r
        return wrapped


def run_learner(out, product, only=""):
    import pytest
    import torch
    from open_duck_playground_amd import engine
    from conftest import _PLOG
    # an element no kernel writes must not differ between the two children by what the allocator handed out
    torch.empty = lambda *a, **k: torch.zeros(*a, **k)
    torch.empty_like = lambda *a, **k: torch.zeros_like(*a, **k)
    rec = Recorder(torch, engine, out)
    for name, module, fn, args in LEARNER_CASES:
        if not name.startswith(only):
            continue
        f = getattr(sys.modules[__name__] if module == "lds_poison_driver" else __import__(module), fn)
        mp = pytest.MonkeyPatch()
        rec.case, rec.calls = name, 0
        t0 = time.time()
        try:
            f(*[_PLOG if a is PLOG else mp if a is MONKEY else a for a in args])
            verdict = "ok"
        except AssertionError as e:      # (under the poison library: stored, and the run goes on; the product library must pass)
            if product:
                raise
            verdict = "check failed: " + " ".join(str(e).split())[:300]
        finally:
            mp.undo()
        out[f"{name}/check"] = np.array(verdict)
        print(f"{name}: {rec.calls} recorded calls, {verdict}, {time.time() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=("env", "learner"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="run the cases whose name starts with this (when looking into a difference)")
    a = ap.parse_args()
    t0 = time.time()
    from open_duck_playground_amd import engine
    lib = os.path.realpath(engine.LIB_PATH)
    product = os.path.basename(lib) == "libodk.so"
    out = {"library": np.array(lib)}
    (run_env if a.family == "env" else run_learner)(out, product, a.only)
    np.savez(a.out, **out)
    print(f"{a.family}: {len(out)} arrays from {lib} in {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
