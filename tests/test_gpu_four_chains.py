"""A biped with arms on the GPU (tests/assets/biped_arms.xml, ShapeE): four serial chains below the floating base (legs 6 / 6, arms 2 / 2),
the chain solve's fourth 8-lane group.  The physics kernels against the float64 oracle at the duck's bounds (one mjx.step, ten substeps,
feet pressed into each other), for both body orders (tests/assets/biped_arms_between.xml: the arms' dofs between the two legs), and the env
kernels (odk_reset / odk_step) against the oracle env."""
import numpy as np
import pytest

from test_gpu_env import (ENV_BOUNDS, RESET_BOUNDS, SET_ASIDE_BOX, _errs, _ill_resets, _mk, _new_W, _obs_err, _resync, _step_and_compare,
                          _xml_model)
from test_gpu_parity import FOOT_BOUNDS, STAGE_BOUNDS, _contact_tie, _contacts, _oracle_step, _rel, _robot_through_the_physics_kernels, torch_cuda  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

ARMS = ("biped_arms.xml", "biped_arms_between.xml")
DIMS, RED_DIMS = (23, 22, 16, 20, 17), (22, 165, 201)      # (nq, nv, nu, nbody, njnt), (reduced dofs, nM, nH)


@pytest.mark.parametrize("xml", ARMS)
def test_a_biped_with_arms_through_the_physics_kernels(torch_cuda, oracle_mod, parity_log, xml):
    """One mjx.step (every comparable stage) and ten substeps from random contact-rich states (test_gpu_parity's robot helper)."""
    _robot_through_the_physics_kernels(torch_cuda, oracle_mod, parity_log, xml, xml[:-4], dims=DIMS, red_dims=RED_DIMS)


@pytest.mark.parametrize("xml", ARMS)
def test_foot_foot_contacts_of_a_biped_with_arms(torch_cuda, oracle_mod, parity_log, xml):
    """Feet pressed into each other (hip rolls inwards, lifted off the floor, yaw / pitch crossings): the foot-foot manifold and the Hessian on
    the virtual tree (second leg below the first foot), whose dof order has the arms between the two legs in biped_arms_between.xml."""
    from open_duck_playground_amd import engine
    torch = torch_cuda
    model = _xml_model(xml)
    jq = lambda name: int(model.a["jnt_qposadr"][model.joint_id(name)])
    lroll, rroll, lyaw, ryaw, lpitch, rpitch = (jq(n) for n in ("left_hip_roll", "right_hip_roll", "left_hip_yaw", "right_hip_yaw",
                                                                "left_hip_pitch", "right_hip_pitch"))
    aq = np.asarray(model.a["jnt_qposadr"])[np.asarray(model.a["actuator_trnid"]).reshape(model.nu, -1)[:, 0]]
    rng = np.random.default_rng(5)
    # hip roll is about +x: a negative left roll / positive right roll swings the feet inwards (they touch from ~0.1 rad on)
    grid = [(l, r, y, pt) for (y, pt) in ((0.0, 0.0), (0.3, 0.0), (-0.25, 0.2)) for l in (-0.09, -0.11, -0.13, -0.15, -0.17, -0.19)
            for r in (0.09, 0.11, 0.13, 0.15, 0.17, 0.21)]
    n = len(grid)
    qpos = np.tile(np.asarray(model.a["key_qpos"], np.float64), (n, 1)); qvel = np.zeros((n, model.nv))
    for e, (l, r, y, pt) in enumerate(grid):
        qpos[e, 2] = 0.5
        qpos[e, lroll] = l + rng.uniform(-0.01, 0.01); qpos[e, rroll] = r + rng.uniform(-0.01, 0.01)
        qpos[e, lyaw] += y; qpos[e, ryaw] -= y; qpos[e, lpitch] += pt; qpos[e, rpitch] -= pt
        qvel[e, 6:] = rng.normal(0, 0.5, model.nv - 6)
    warm = np.zeros((n, model.nv))
    ctrl = np.stack([qpos[e, aq] for e in range(n)])
    b = engine.Batch(model, n)
    b.set_state(qpos, qvel, warm)
    b.physics_step(torch.tensor(ctrl, dtype=torch.float32, device="cuda"), 1)
    gq, gv, _ = b.get_state()
    img = b.lds_image()
    om = oracle_mod.OracleModel(model.blob())
    o = {k: b.lds_offset(k) for k in ("contact_dist", "qacc")}
    nv, nq = model.nv, model.nq
    n_pen = n_flip = n_tie = 0
    prng = np.random.default_rng(97)
    worst = dict(dist=0.0, qacc=0.0, qpos=0.0, qvel=0.0)
    for e in range(n):
        d = oracle_mod.OracleData(om)
        d["qpos"][:nq] = qpos[e]; d["qvel"][:nv] = qvel[e]; d["ctrl"][: model.nu] = ctrl[e]
        d.forward()
        cd_o = np.array(d["contact_dist"][8:12]); cd_g = img[e][o["contact_dist"] + 8: o["contact_dist"] + 12]
        n_pen += int((cd_o < 0).any())
        if _contact_tie(oracle_mod, om, qpos[e], qvel[e], ctrl[e], prng, _contacts(d)):
            n_tie += 1
            continue
        if set(np.flatnonzero(cd_o < 0)) != set(np.flatnonzero(cd_g < 0)):
            n_flip += 1
            continue
        pen = cd_o < 0
        if pen.any():
            worst["dist"] = max(worst["dist"], np.abs(cd_g[pen] - cd_o[pen]).max())
        worst["qacc"] = max(worst["qacc"], _rel(img[e][o["qacc"]: o["qacc"] + nv], d["qacc"][:nv], 5.0).max())
        ds = _oracle_step(oracle_mod, om, qpos[e], qvel[e], warm[e], ctrl[e], 1)
        worst["qpos"] = max(worst["qpos"], _rel(gq[e], ds["qpos"][:nq], 1e-2).max())
        worst["qvel"] = max(worst["qvel"], _rel(gv[e], ds["qvel"][:nv], 1.0).max())
    b.close()
    print(xml, dict(n=n, penetrating=n_pen, flips=n_flip, ties=n_tie, **{k: float(f"{v:.3g}") for k, v in worst.items()}))
    assert n_pen >= 30, "the grid must contain penetrating poses"
    # box feet pressed sole to side tie in the manifold's arg-max steps by construction (SET_ASIDE_BOX in test_gpu_env.py; measured 30 of 108 poses,
    # against the duck's hull <= 5 %), and their deep face contacts put qacc at the one-step stage bound rather than the duck's foot-foot one (measured 3.0e-4)
    assert n_flip == 0 and n_tie <= n // 3
    parity_log.check(f"foot_foot/{xml}", dict(FOOT_BOUNDS, qacc=STAGE_BOUNDS["qacc"]), **worst)


def test_env_steps_of_a_biped_with_arms(oracle_mod, parity_log):
    """odk_reset and 60 odk_step of biped_arms.xml against the oracle env: observation noise, pushes, truncation, auto-reset and domain
    randomisation (randomize.py's per-env model fields) on; physics re-synchronised before every step, the carried info running free."""
    from open_duck_playground_amd import randomize
    xml, nu, nobs, npriv = "biped_arms.xml", 16, 113, 230
    n = 32
    fields, _ = randomize.domain_randomize(_xml_model(xml), np.random.default_rng(17), n)

    def edit(cfg):
        cfg.episode_length = 25
    torch, model, b, envs, keep = _mk(oracle_mod, xml, n, edit, dr_fields=fields)
    assert model.nu == nu and (b.nobs, b.npriv) == (nobs, npriv) == (envs[0].nobs, envs[0].npriv) and b.lanes_per_env == 32
    b.reset(seed=9)
    obs = b.obs.cpu().numpy(); priv = b.priv.cpu().numpy()
    for i, e in enumerate(envs):
        e.reset(9, i)
    ill = _ill_resets(envs, model, nobs)
    WR = dict(obs=0.0, acc=0.0)
    for i, e in enumerate(envs):
        o, a = _obs_err(obs[i], priv[i], e, nobs, npriv)
        WR["obs"] = max(WR["obs"], o); WR["acc"] = max(WR["acc"], 0.0 if i in ill else a)
    rng = np.random.default_rng(0)
    W = _new_W()
    W["reset_ill"] = ill
    for t in range(60):
        _resync(b, envs, model)
        act = rng.uniform(-1, 1, (n, nu)).astype(np.float32)
        _step_and_compare(torch, b, envs, act, nobs, npriv, t, W)
    assert W["n_trunc"] > 0, "sequence must cross truncations"
    I = b.info()
    for i, e in enumerate(envs):
        np.testing.assert_allclose(I["last_act"][i], e["last_act"][:nu], atol=1e-6)
        np.testing.assert_allclose(I["action_history"][i], e["action_history"][:3 * nu], atol=1e-6)
        assert int(I["rng"][i, 2]) == int(e.ints("rng_ctr")[0])
    b.close()
    errs = _errs(W)
    print(xml, "reset", WR, "steps", errs)
    parity_log.check(f"robot_env/{xml}/dr/reset", dict(obs=RESET_BOUNDS["obs"], acc=RESET_BOUNDS["acc"]), **WR)
    parity_log.check(f"robot_env/{xml}/dr/env_step", {**ENV_BOUNDS, **SET_ASIDE_BOX}, **errs)
