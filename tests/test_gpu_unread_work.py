"""The product env step against the step that fills the debug image, and the RNG stream across a change of noise_level.

The product step kernels leave out the stores that only the debug image reads, draw no observation noise while noise_level is 0, and
build the observation through the gather table made at model load.  None of that may change what a caller gets: both launches return the
same outputs bit for bit (noise and pushes on, both tasks, and a robot that is not the duck), and a run that starts with noise off and
turns it on later continues on the stream a run with noise on from the start is on (stored key and counter, and the noisy observations
themselves: the noise reaches no physics, so both runs are in the same state)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [("flat_terrain", False), ("flat_terrain", True), ("flat_terrain_backlash", False), ("tail_biped.xml", False)]
N_ENVS, N_STEPS = 64, 40


def _model(task):
    from open_duck_playground_amd.model import Model, load_task_model
    if task.endswith(".xml"):
        return Model.from_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", task), sim_dt=0.002)
    return load_task_model(task)


def _batch(task, standing, noise_level):
    from open_duck_playground_amd import engine
    cfg = engine.default_config(standing)
    if task.endswith(".xml"):
        cfg.use_imitation = 0
    cfg.noise_level = noise_level
    cfg.push_enable = 1.0
    cfg.push_interval_range[0] = 0.1; cfg.push_interval_range[1] = 0.3      # a push every 5 .. 15 env steps
    cfg.episode_length = 25                                                # truncation and auto-reset inside the run
    return engine.Batch(_model(task), N_ENVS, cfg), cfg


def _actions(torch, nu):
    g = torch.Generator(device="cuda:0").manual_seed(11)
    return [torch.empty(N_ENVS, nu, device="cuda:0").uniform_(-1, 1, generator=g) for _ in range(N_STEPS)]


def _outputs(b):
    qpos, qvel, warm = b.get_state()
    out = {k: getattr(b, k).cpu().numpy().copy() for k in ("obs", "priv", "reward", "done", "truncation", "metrics")}
    out.update(qpos=qpos.copy(), qvel=qvel.copy(), warm=warm.copy(), records=b.records().copy())
    return out


@pytest.mark.parametrize("task,standing", CASES)
def test_debug_launch_and_product_launch_return_the_same(task, standing):
    import torch
    from open_duck_playground_amd import engine
    L = engine.load_library()
    bd, _ = _batch(task, standing, 1.0)
    bp, _ = _batch(task, standing, 1.0)
    acts = _actions(torch, bd.model.nu)
    try:
        bd.reset(seed=21); bp.reset(seed=21)
        pushed = 0
        for t, a in enumerate(acts):
            L.odk_set_debug_dump(1)
            bd.step(a)
            L.odk_set_debug_dump(0)
            bp.step(a)
            torch.cuda.synchronize()
            od, op = _outputs(bd), _outputs(bp)
            for k in od:
                assert np.array_equal(od[k].view(np.uint32), op[k].view(np.uint32)), (task, standing, t, k)
            pushed += int((np.abs(bp.info()["push"]).sum(axis=1) > 0).sum())
        assert np.isfinite(op["obs"]).all() and pushed > 0      # the run did meet pushes
        # The debug launch filled its image, debug-only slots included.  S_MISC + 7 is the line search's gradient tolerance of the last substep,
        # a model constant times the norm of the search direction, which the image holds too: the ratio is one positive number for every env
        # (float32 sums of <= 32 squares: 1e-4 is far above their rounding, far below anything a slot not written by this launch would show).
        img = bd.lds_image()
        o_cd, o_misc, o_s, o_jar = (bd.lds_offset(k) for k in ("contact_dist", "misc", "search", "jar"))
        assert np.abs(img[:, o_cd: o_cd + 8]).sum() > 0
        assert set(np.unique(img[:, o_misc + 2])) <= {0.0, 1.0}      # warm start used
        gtol = img[:, o_misc + 7].astype(np.float64)
        assert np.isfinite(gtol).all() and (gtol > 0).all(), (task, standing)
        if "backlash" not in task:      # (the backlash model keeps the search direction on its reduced dofs)
            sn = np.sqrt((img[:, o_s: o_s + bd.model.nv].astype(np.float64) ** 2).sum(axis=1))
            ratio = gtol / sn
            print(f"gtol / |search| {task} standing={standing}: min {ratio.min():.9g} max {ratio.max():.9g}")
            assert ratio.max() / ratio.min() - 1.0 < 1e-4, (task, standing, ratio.min(), ratio.max())
        assert np.abs(img[:, o_jar: o_jar + 60]).sum() > 0      # Jaref of the contact rows: a debug-only store
    finally:
        L.odk_set_debug_dump(0)
        bd.close(); bp.close()


@pytest.mark.parametrize("task,standing", CASES)
def test_noise_switched_on_later_continues_the_same_stream(task, standing):
    import torch
    n_off = 12
    b_on, _ = _batch(task, standing, 1.0)         # noise on from the start
    b_sw, cfg = _batch(task, standing, 0.0)       # noise off for n_off steps, then on
    acts = _actions(torch, b_on.model.nu)
    try:
        b_on.reset(seed=33); b_sw.reset(seed=33)
        # Commands are resampled on the step that takes info["step"] past 500, from draws of the same block as the observation noise.  Some envs
        # start close to it, so that with noise still off some waves (two envs each at 32 lanes) have no resampling env, some one -- the first or the
        # second of the pair -- and some two: stored 500 resamples on the first step, 499 on the second, 498 on the third.
        preset = {0: 500, 3: 500, 4: 500, 5: 500, 8: 499, 11: 499, 12: 499, 13: 499, 17: 498, 62: 498}
        for b in (b_on, b_sw):
            I = b.info()
            I["step"][:] = np.arange(N_ENVS) % 7
            for e, v in preset.items():
                I["step"][e] = v
            b.set_records(I["_records"])
        resampled = set()
        cmd_before = b_sw.info()["command"].copy()
        nobs = b_on.nobs
        differed = False
        for t, a in enumerate(acts):
            if t == n_off:
                cfg.noise_level = 1.0
                b_sw.set_config(cfg)
            b_on.step(a); b_sw.step(a)
            torch.cuda.synchronize()
            i_on, i_sw = b_on.info(), b_sw.info()
            assert np.array_equal(i_on["rng"], i_sw["rng"]), (task, standing, t)      # stored key and counter
            for k in ("step", "command", "push", "push_step"):
                assert np.array_equal(i_on[k], i_sw[k]), (task, standing, t, k)
            for e, v in preset.items():
                if t == 500 - v:      # this env resampled on this step, with noise off: a fresh command, the one the noise-on batch drew
                    assert int(i_sw["step"][e]) == 0 and t < n_off, (task, standing, t, e)
                    resampled.add(e)
                    if not np.array_equal(i_sw["command"][e], cmd_before[e]):
                        resampled.add(("changed", e))
            cmd_before = i_sw["command"].copy()
            s_on, s_sw = b_on.get_state(), b_sw.get_state()
            assert all(np.array_equal(x, y) for x, y in zip(s_on, s_sw)), (task, standing, t)      # observation noise reaches no physics
            o_on, o_sw = b_on.obs.cpu().numpy(), b_sw.obs.cpu().numpy()
            p_on, p_sw = b_on.priv.cpu().numpy(), b_sw.priv.cpu().numpy()
            assert np.array_equal(p_on[:, nobs:], p_sw[:, nobs:]), (task, standing, t)              # the privileged tail carries no noise
            fresh = b_on.done.cpu().numpy() != 0      # an auto-reset row shows the reset's observation, drawn with the reset's noise_level
            if t >= n_off:
                assert np.array_equal(o_on[~fresh], o_sw[~fresh]), (task, standing, t)            # same draws, same noise
            else:
                differed |= bool((o_on[~fresh] != o_sw[~fresh]).any())
                assert np.array_equal(o_sw[~fresh][:, :3], p_sw[~fresh][:, nobs: nobs + 3]), (task, standing, t)   # noise off: the gyro as it is
        assert differed      # the noise was really off in the first part
        assert all(e in resampled for e in preset)
        assert sum(1 for x in resampled if isinstance(x, tuple)) >= len(preset) - 2      # (a resample may draw the zero command twice in a row)
    finally:
        b_on.close(); b_sw.close()
