"""Cases of the neighbour-independence tests (tests/test_gpu_neighbours.py on the GPU, tests/test_neighbours_host.py without one).

At 32 lanes per env two envs share a wave and an LDS allocation, and the env kernels let them interact on purpose (ballot-guarded branches,
the height-field pair loop, foot_foot_sat, the wave-wide Hessian switch, the dead slot of an odd batch).  The property: the same env with
the same inputs stores the same BITS whoever shares its wave and whichever slot it sits in -- with one exception, the wave-wide switch to the
virtual tree (csrc/odk_kernels.h `any_ffa`), which the tests model as a group and do not tolerate (profiles/neighbours/NOTES.md).

Not collected by pytest.  CPU only: the state pools come from the float64 oracle, the batches are laid out here; nothing in this file
touches a GPU.  The kernel sets, their models and the two configurations are tests/lds_poison_driver.py's (ENV_CASES, _model, _config)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lds_poison_driver import ENV_CASES, ENV_CONFIGS, _config, _model  # noqa: E402,F401

N_ORD, N_FF = 16, 4      # subjects per case: ordinary states, foot-foot states (where the case has a pool)
FF_MIN_DUCK = 5          # pressed-feet states of make_states(task, 64, 0) with a negative foot-foot distance on the oracle: at least this many ...
FF_MIN = {"B-32-hfield-prim": 4}      # ... but four with sphere / capsule feet (measured: 4 of 8; hulls: 7 of 8, 5 of 8 with backlash joints)
ORD_MARGIN = 1e-4        # an ordinary state's foot-foot distance on the oracle (m): far above float32 rounding of a distance (~1e-7)
# the neighbour kinds of a subject s, each placed once with s in slot 0 and once in slot 1 (the twin: one wave holds both; the dead slot: slot 0 only)
KINDS = ("twin", "ordinary", "footfoot", "nan_qpos", "nan_qvel", "overflow", "far", "upside_down", "dead_slot")
PLANTED = ("nan_qpos", "nan_qvel", "overflow", "far", "upside_down")      # neighbours only, never subjects
# models whose Hessian is ALWAYS factored on the virtual tree (DevModel::eqp_cross: a connect between the two foot chains, odk_model_load.hip)
ALWAYS_VIRTUAL = ("C-32-loop",)
ELLIPTIC = ("AE-32", "BE-32-plane", "BE-32-hfield")

CASE_NAMES = [c[0] for c in ENV_CASES]
CASES_32 = [c[0] for c in ENV_CASES if c[3] == 32]
CASES_64 = [c[0] for c in ENV_CASES if c[3] == 64]


def case(name):
    return next(c for c in ENV_CASES if c[0] == name)


def is_robot(spec):
    return isinstance(spec, str) and spec.endswith(".xml")


def duck_task_variant(spec):
    """an ENV_CASES model spec in tools/gpu_fuzz_parity.make_states' terms"""
    if isinstance(spec, str):
        return spec, None
    return spec[1], ("elliptic" if spec[0] == "cone" else "-".join(spec[2]))


def footfoot_dist(O, om, qpos):
    """min(contact_dist[8:12]) of the float64 oracle at qpos: a function of qpos alone"""
    d = O.OracleData(om)
    d["qpos"][: om.nq] = qpos
    d.forward()
    return float(np.min(np.asarray(d["contact_dist"][8:12])))


def _pressed_feet_robot(O, model, om, n, rng):
    """Foot-foot pool of a robot: the key pose with both hip-roll joints turned by the same angle towards each other, the angle found by
    bisection on the oracle so that the feet overlap by 0.3 ... 4 mm; every other state airborne, the others settled on the floor.  None when the
    joint limits do not let the feet meet."""
    from test_gpu_parity import _settle_on_terrain
    names = [str(s) for s in model.a["names_jnt"]]
    if "left_hip_roll" not in names or "right_hip_roll" not in names:
        return None
    jl, jr = names.index("left_hip_roll"), names.index("right_hip_roll")
    al, ar = int(model.a["jnt_qposadr"][jl]), int(model.a["jnt_qposadr"][jr])
    hi = min(float(model.a["jnt_range"][jl][1]), float(model.a["jnt_range"][jr][1]), -float(model.a["jnt_range"][jl][0]), -float(model.a["jnt_range"][jr][0]))
    key = np.asarray(model.a["key_qpos"], np.float64)

    def pose(sign, th):
        q = key.copy(); q[2] += 0.2; q[al] += sign * th; q[ar] -= sign * th
        return q
    # the first angle (steps of 0.01 rad from the key pose, either way) at which the feet overlap by 4 mm: past it the legs cross and the feet part again,
    # so the bisection below stays between the key pose and this angle, where the overlap grows with the angle
    sign, reach = None, None
    for th in np.arange(0.01, hi + 1e-9, 0.01):
        for s in (1.0, -1.0):
            if sign is None and footfoot_dist(O, om, pose(s, th)) < -4e-3:
                sign, reach = s, float(th)
    if sign is None:
        return None
    out = []
    for k in range(n):
        target = -rng.uniform(3e-4, 4e-3)
        lo_t, hi_t = 0.0, reach      # dist(lo_t) >= 0 > target >= dist(hi_t)
        for _ in range(40):
            mid = 0.5 * (lo_t + hi_t)
            if footfoot_dist(O, om, pose(sign, mid)) > target:
                lo_t = mid
            else:
                hi_t = mid
        q = pose(sign, hi_t)
        q[0:2] += rng.uniform(-0.05, 0.05, 2)
        out.append(q)
    qpos = np.array(out)
    air = np.arange(n) % 2 == 0
    for e in range(n):
        if not air[e]:
            qpos[e, 2] = key[2]
    return _settle_on_terrain(O, om, qpos, rng, air)


_POOLS = {}


def pools(O, name):
    """-> dict(model, om, qpos, qvel, warm, ctrl [rows of the pool], ord [pool rows of the ordinary states], ff [pool rows of the foot-foot states],
    ff_dist [oracle foot-foot distance per row]).  Ducks: make_states(task, 64, 0); robots: the generator of _robot_through_the_physics_kernels plus
    bisected pressed-feet poses."""
    if name in _POOLS:
        return _POOLS[name]
    _, _, spec, lanes, _ = case(name)
    if is_robot(spec):
        from test_gpu_parity import _robot_states
        model = _model(spec)
        om = O.OracleModel(model.blob())
        rng, qpos, qvel, warm, ctrl = _robot_states(O, model, om, 64)
        rng = np.random.default_rng(97)
        pressed = _pressed_feet_robot(O, model, om, 8, rng)
        n0 = len(qpos)
        if pressed is not None:
            k = len(pressed)
            qpos = np.concatenate([qpos, pressed])
            qvel = np.concatenate([qvel, rng.normal(0, 0.5, (k, model.nv))])
            warm = np.concatenate([warm, rng.normal(0, 5.0, (k, model.nv))])
            ctrl = np.concatenate([ctrl, np.asarray(model.a["key_ctrl"])[None] + rng.uniform(-0.4, 0.4, (k, model.nu))])
        ffd = np.array([footfoot_dist(O, om, q) for q in qpos])
        ord_rows = [e for e in range(n0) if ffd[e] > ORD_MARGIN]
        ff_rows = [e for e in range(n0, len(qpos)) if ffd[e] < 0]
    else:
        import gpu_fuzz_parity as fz
        task, variant = duck_task_variant(spec)
        model, om, _, qpos, qvel, warm, ctrl = fz.make_states(task, 64, 0, variant)
        ffd = np.array([footfoot_dist(O, om, q) for q in qpos])
        pressed = [e for e in range(64) if e % 16 in (7, 15)]
        ord_rows = [e for e in range(64) if e not in pressed]
        ff_rows = [e for e in pressed if ffd[e] < 0]
    P = dict(name=name, model=model, om=om, qpos=np.asarray(qpos, np.float64), qvel=np.asarray(qvel, np.float64), warm=np.asarray(warm, np.float64),
             ctrl=np.asarray(ctrl, np.float64), ord=ord_rows, ff=ff_rows, ff_dist=ffd, lanes=lanes)
    _POOLS[name] = P
    return P


def _plant(kind, q, v):
    """a neighbour that is never a subject, made from an ordinary state"""
    q, v = q.copy(), v.copy()
    if kind == "nan_qpos":
        q[9] = np.nan
    elif kind == "nan_qvel":
        v[7] = np.nan
    elif kind == "overflow":
        v[8] = 3e38      # a joint velocity that overflows inside the pass
    elif kind == "far":
        q[0], q[1] = 1e5, -1e5      # off the grid of a height field
    elif kind == "upside_down":
        q[2] = 0.3; q[3:7] = [0.0, 1.0, 0.0, 0.0]      # terminates (the up vector points down)
    else:
        raise KeyError(kind)
    return q, v


def arrangement(P, leave_out=()):
    """One batch per case.  -> dict(qpos, qvel, warm [nenv, ...] float64; src [nenv]: the pool row whose per-env inputs (ctrl / action, DR row, command,
    push, delay, record) the env carries; sid [nenv]: the subject (= its pool row) the env is an occurrence of, -1 for a planted neighbour;
    kind [nenv]: the neighbour kind of the env's wave; role [nenv]: 1 = the wave's subject, 0 = its neighbour; subjects; nenv (odd: the last env has the dead slot as partner))."""
    subjects = P["ord"][:N_ORD] + P["ff"][:N_FF]
    envs = []      # (pool row, planted kind or None, kind of the wave, the wave's subject (1) or its neighbour (0))
    for i, s in enumerate(subjects):
        is_ff = s in P["ff"]
        other = P["ord"][(P["ord"].index(s) + 1) % len(P["ord"])] if not is_ff else P["ord"][i % len(P["ord"])]
        for kind in KINDS:
            if kind in leave_out or kind == "dead_slot":
                continue
            if kind == "twin":
                envs += [(s, None, kind, 1), (s, None, kind, 1)]
                continue
            if kind == "ordinary":
                nb = (other, None)
            elif kind == "footfoot":
                if not P["ff"]:
                    continue
                pool = [f for f in P["ff"] if f != s]
                nb = (pool[i % len(pool)], None)
            else:
                nb = (other, kind)
            envs += [(s, None, kind, 1), (nb[0], nb[1], kind, 0)]      # s in slot 0
            envs += [(nb[0], nb[1], kind, 0), (s, None, kind, 1)]      # s in slot 1
    envs.append((subjects[0], None, "dead_slot" if "dead_slot" not in leave_out else "twin", 1))
    if "dead_slot" in leave_out:
        envs.append((subjects[0], None, "twin", 1))
    n = len(envs)
    qpos = np.zeros((n, P["qpos"].shape[1])); qvel = np.zeros((n, P["qvel"].shape[1])); warm = np.zeros((n, P["warm"].shape[1]))
    src = np.zeros(n, np.int64); sid = np.full(n, -1, np.int64); kinds = []
    role = np.array([r for _, _, _, r in envs], np.int64)
    for e, (row, planted, kind, _) in enumerate(envs):
        q, v = P["qpos"][row], P["qvel"][row]
        if planted:
            q, v = _plant(planted, q, v)
        qpos[e], qvel[e], warm[e] = q, v, P["warm"][row]
        src[e] = row
        sid[e] = -1 if planted else row      # (an unplanted neighbour is a pool state like any other: its results are held to the rule too)
        kinds.append(kind)
    return dict(qpos=qpos, qvel=qvel, warm=warm, src=src, sid=sid, kind=np.array(kinds), role=role, subjects=subjects, nenv=n)


def partner(e, nenv, lanes):
    """the env that shares env e's wave (32 lanes per env: envs 2w and 2w + 1; the dead slot re-runs the last env itself); None at 64 lanes"""
    if lanes != 32:
        return None
    p = e ^ 1
    return p if p < nenv else e


def everything_inputs(P, rng_seed=3):
    """Per POOL ROW inputs of the "everything" configuration (an env takes the rows of its `src`): DR fields, commands, pushes of two steps,
    action delays (0, 1, 2 and -1 = the sampled one), actions."""
    from open_duck_playground_amd import randomize
    model = P["model"]
    n = len(P["qpos"])
    fields, _ = randomize.domain_randomize(model, np.random.default_rng(17), n)
    rng = np.random.default_rng(rng_seed)
    cmd = np.zeros((n, 7), np.float32)
    cmd[:, :3] = rng.uniform(-0.2, 0.2, (n, 3)); cmd[:, 3:] = rng.uniform(-0.5, 0.5, (n, 4)); cmd[::7] = 0.0
    push = rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32); push[::5] = 0.0
    delay = rng.integers(-1, 3, n).astype(np.int32)
    action = rng.uniform(-1, 1, (n, model.nu)).astype(np.float32)
    return dict(fields=fields, cmd=cmd, push=push, delay=delay, action=action)


def bits(a):
    """an array's words (float32 / int32 as uint32: NaN payloads and the sign of zero count)"""
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint32) if a.ndim > 1 else a.reshape(-1, 1).view(np.uint32)


def env_flag(cd, D_ff, jar_ff, cone=None):
    """Whether one env turns its wave's Hessian to the virtual tree in a forward pass, from that pass's debug image: "yes", "no" or "unknown".
    The kernel's test (odk_kernels.h ff_active): min(contact_dist[8:12]) < 0 (fminf: a NaN entry is passed over) and a non-zero diagonal of the
    foot-foot block K_X, the sum of the sixteen foot-foot rows' Hessian terms.  Pyramidal cones: `some foot-foot row has D > 0 and Jaref < 0`.
    Elliptic cones (cone = (mu, impratio) of the foot-foot pair): `some foot-foot contact with D_n > 0 is not in its cone's top zone`, the zone test of
    cone_ev restated in float32 on the contact's three Jaref.  With a non-finite entry the image does not decide it: "unknown"."""
    with np.errstate(invalid="ignore", over="ignore"):
        if not np.fmin.reduce(cd[8:12]) < 0:
            return "no"
        if not (np.isfinite(cd[8:12]).all() and np.isfinite(D_ff).all() and np.isfinite(jar_ff).all()):
            return "unknown"
        if cone is None:
            return "yes" if ((D_ff > 0) & (jar_ff < 0)).any() else "no"
        f32 = np.float32
        mu = f32(cone[0]); mur = f32(mu * f32(1.0 / np.sqrt(f32(cone[1]))))
        x = np.asarray(jar_ff, f32).reshape(4, 4); Dn = np.asarray(D_ff, f32).reshape(4, 4)[:, 0]
        U1, U2, N = mu * x[:, 1], mu * x[:, 2], mur * x[:, 0]
        T = np.sqrt(U1 * U1 + U2 * U2, dtype=f32)
        top = (N >= mur * T) | ((T <= 0) & (N >= 0)) | ~(Dn > 0)
        return "no" if top.all() else "yes"


def wave_keys(flags, nenv, lanes, always_virtual, src):
    """Per env the group of this pass: "P" (plain: no env of its wave has an active foot-foot row), "V" (virtual), or ("U", partner's pool row) where
    the image does not decide it (held to its mirror arrangement only).  64 lanes: one env per wave, the env's own flag."""
    out = []
    for e in range(nenv):
        p = partner(e, nenv, lanes)
        fl = {flags[e]} | ({flags[p]} if p is not None else set())
        if always_virtual or "yes" in fl:
            out.append("V")
        elif "unknown" in fl:
            out.append(("U", int(src[p if p is not None else e]), str(flags[e]), str(flags[p if p is not None else e])))
        else:
            out.append("P")
    return out


def mismatches(A, keys, arrays, what=""):
    """The rule itself: the occurrences of one subject (envs with the same `sid`) that share a group key hold the same bits in every array.
    -> messages, one per (subject, group, array) that differs, naming both envs, their partners' kinds and the first differing word."""
    bad = []
    occ = {}
    for e in range(A["nenv"]):
        if A["sid"][e] >= 0:
            occ.setdefault((int(A["sid"][e]), keys[e]), []).append(e)
    for (s, key), envs in sorted(occ.items(), key=lambda kv: str(kv[0])):
        for name, a in arrays.items():
            w = bits(a)
            ref = w[envs[0]]
            for e in envs[1:]:
                if not np.array_equal(ref, w[e]):
                    i = int(np.flatnonzero(ref != w[e])[0])
                    bad.append(f"{what}{name}: subject {s} group {key}: env {envs[0]} (slot {envs[0] & 1}, beside {A['kind'][envs[0]]}) != env {e} (slot {e & 1}, beside "
                               f"{A['kind'][e]}): {int((ref != w[e]).sum())} of {ref.size} words, first [{i}] {int(ref[i]):#010x} != {int(w[e][i]):#010x}")
    return bad


def group_sizes(A, keys):
    """occurrences of subjects per group of ONE pass (wave_keys' output): (plain, virtual, undecided)"""
    k = [keys[e] for e in range(A["nenv"]) if A["sid"][e] >= 0]
    return sum(x == "P" for x in k), sum(x == "V" for x in k), sum(isinstance(x, tuple) for x in k)
