"""CPU side of the neighbour-independence tests: the state pools (from the float64 oracle), the batch layout, the group rule and the
comparison itself, so that tests/test_gpu_neighbours.py spends its GPU time on launches and a mistake in the machinery shows here.
Cases and helpers: tests/neighbours_cases.py."""
import numpy as np
import pytest

import neighbours_cases as NC


def test_the_cases_are_the_compiled_kernel_sets():
    """all twelve 32-lane instantiations and the two 64-lane controls, taken from the poison driver's table"""
    from lds_poison_driver import ENV_CASES, ENV_CONFIGS
    assert len(NC.CASES_32) == 12 and len(NC.CASES_64) == 2 and NC.CASE_NAMES == [c[0] for c in ENV_CASES]
    assert {NC.case(n)[1] for n in NC.CASES_32} == {c[1] for c in ENV_CASES if c[1][1] == 32}
    assert ENV_CONFIGS == ("defaults", "everything")
    assert set(NC.ALWAYS_VIRTUAL) | set(NC.ELLIPTIC) <= set(NC.CASE_NAMES)


@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_state_pools(oracle_mod, name):
    """At least 16 ordinary subjects, none with a negative foot-foot distance on the oracle; a foot-foot pool of at least 5 states for the duck
    models (4 with sphere / capsule feet) and of at least 4 for the robots, every one with a negative foot-foot distance; the ducks' model is the
    one the poison driver builds for the case."""
    P = NC.pools(oracle_mod, name)
    spec = NC.case(name)[2]
    assert P["model"].blob() == NC._model(spec).blob()
    assert len(P["ord"]) >= NC.N_ORD + 1 and all(P["ff_dist"][e] >= 0 for e in P["ord"]), (name, len(P["ord"]))
    if NC.is_robot(spec):
        assert all(P["ff_dist"][e] > NC.ORD_MARGIN for e in P["ord"])
        assert len(P["ff"]) >= NC.N_FF, (name, len(P["ff"]))      # (no robot of the suite is held apart by its joint limits: every set has the virtual group)
    else:
        pressed = [e for e in range(64) if e % 16 in (7, 15)]
        assert min(P["ff_dist"][e] for e in P["ord"]) > 1e-3      # (the nearest non-touching state: 1.3 mm)
        assert len(P["ff"]) >= NC.FF_MIN.get(name, NC.FF_MIN_DUCK) and set(P["ff"]) <= set(pressed), (name, P["ff"])
    assert all(P["ff_dist"][e] < 0 for e in P["ff"])
    depth = [-P["ff_dist"][e] for e in P["ff"]]
    print(name, "ordinary", len(P["ord"]), "foot-foot", len(P["ff"]), "overlap mm", [round(1e3 * d, 2) for d in depth])
    for k in ("qpos", "qvel", "warm", "ctrl"):
        assert np.isfinite(P[k]).all()


@pytest.mark.parametrize("name", ["A-32", "B-32-hfield-hull", "D-32", "A-64"])
def test_arrangement(oracle_mod, name):
    """Every subject meets every neighbour kind once in slot 0 and once in slot 1 of a wave; planted neighbours are never subjects; every env's
    per-env inputs are its pool row's; the batch is odd and its last env (a subject) has the dead slot."""
    P = NC.pools(oracle_mod, name)
    A = NC.arrangement(P)
    n = A["nenv"]
    assert n % 2 == 1 and A["kind"][-1] == "dead_slot" and A["sid"][-1] == A["subjects"][0] and NC.partner(n - 1, n, 32) == n - 1
    assert len(A["subjects"]) == NC.N_ORD + NC.N_FF and len(set(A["subjects"])) == len(A["subjects"])
    assert NC.partner(4, n, 32) == 5 and NC.partner(5, n, 32) == 4 and NC.partner(4, n, 64) is None
    for s in A["subjects"]:
        seen = {}
        for e in range(n - 1):
            if A["sid"][e] == s and A["role"][e] == 1:      # (s as the wave's subject; as another subject's neighbour it is held to the rule all the same)
                p = e ^ 1
                assert A["kind"][p] == A["kind"][e] and (A["role"][p] == 0 or A["kind"][e] == "twin")
                planted = A["sid"][p] < 0
                if A["kind"][e] in NC.PLANTED:
                    assert planted
                    q, v = A["qpos"][p], A["qvel"][p]
                    assert not (np.isfinite(q).all() and np.isfinite(v).all() and np.abs(v).max() < 1e38 and np.abs(q[:2]).max() < 1e4 and q[3] != 0.0)
                elif A["kind"][e] == "twin":
                    assert A["sid"][p] == s
                elif A["kind"][e] == "footfoot":
                    assert A["sid"][p] in P["ff"] and A["sid"][p] != s
                elif A["kind"][e] == "ordinary" and s in P["ord"]:
                    assert A["sid"][p] in P["ord"] and A["sid"][p] != s
                seen.setdefault(str(A["kind"][e]), set()).add(e & 1)
        assert set(seen) == set(NC.KINDS) - {"dead_slot"}, (s, seen)
        assert all(v == {0, 1} for v in seen.values()), (s, seen)
    for e in range(n):      # rows follow the env; an unplanted env IS its pool row
        r = A["src"][e]
        assert np.array_equal(A["warm"][e], P["warm"][r])
        if A["sid"][e] >= 0:
            assert A["sid"][e] == r and np.array_equal(A["qpos"][e], P["qpos"][r]) and np.array_equal(A["qvel"][e], P["qvel"][r])
    # a kind left out (profiles/neighbours/NOTES.md: where termination could not be shown) leaves the batch odd and the rest in place
    B = NC.arrangement(P, leave_out=("nan_qpos", "nan_qvel", "overflow"))
    assert B["nenv"] % 2 == 1 and not set(B["kind"]) & {"nan_qpos", "nan_qvel", "overflow"} and np.isnan(A["qpos"]).any() and not np.isnan(B["qpos"]).any()


def test_bits_see_the_sign_of_zero_and_nan_payloads():
    a = np.array([[0.0, 1.0], [-0.0, 1.0]], np.float32)
    assert not np.array_equal(NC.bits(a)[0], NC.bits(a)[1]) and np.array_equal(a[0], a[1])
    n = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    assert NC.bits(n)[0, 0] != NC.bits(n)[1, 0]
    assert NC.bits(np.array([3, 4], np.int32)).shape == (2, 1)


def test_the_group_rule():
    """env_flag / wave_keys: the switch needs a negative foot-foot distance AND an active foot-foot row; NaN entries of the distance are passed
    over like fminf does; a non-finite image is undecided, not plain."""
    cd = np.ones(12, np.float32); D = np.zeros(16, np.float32); jar = np.zeros(16, np.float32)
    assert NC.env_flag(cd, D, jar) == "no"
    cd[9] = -1e-3
    assert NC.env_flag(cd, D, jar) == "no" and NC.env_flag(cd, D, jar, (1.0, 1.0)) == "no"      # (a negative distance alone is not enough)
    Dn = np.zeros(16, np.float32); x = np.zeros(16, np.float32); Dn[4] = 3.0      # elliptic: contact 1 = rows 4 .. 6 (normal, two tangents)
    x[4:7] = [0.5, 0.3, 0.3]
    assert NC.env_flag(cd, Dn, x, (1.0, 1.0)) == "no"      # top zone (x_n >= |x_t|: separating): no force, no Hessian
    x[4:7] = [0.2, 0.3, 0.3]
    assert NC.env_flag(cd, Dn, x, (1.0, 1.0)) == "yes"     # middle zone
    x[4:7] = [-0.9, 0.3, 0.3]
    assert NC.env_flag(cd, Dn, x, (1.0, 1.0)) == "yes"     # bottom zone
    assert NC.env_flag(cd, Dn, x, (1.0, 100.0)) == "yes" and NC.env_flag(cd, np.zeros(16, np.float32), x, (1.0, 1.0)) == "no"
    D[4] = 2.0; jar[4] = 0.5
    assert NC.env_flag(cd, D, jar) == "no"      # (a separating row: D > 0, Jaref >= 0)
    jar[4] = -0.5
    assert NC.env_flag(cd, D, jar) == "yes"
    cd[8] = np.nan
    assert NC.env_flag(cd, D, jar) == "unknown"
    assert NC.env_flag(np.full(12, np.nan, np.float32), D, jar) == "no"      # (every distance NaN: `NaN < 0` is false in the kernel too)
    src = np.arange(5)
    keys = NC.wave_keys(["no", "yes", "no", "unknown", "no"], 5, 32, False, src)
    assert keys[0] == "V" and keys[1] == "V" and keys[2][0] == "U" and keys[2][1] == 3 and keys[3][0] == "U" and keys[4] == "P"
    assert NC.wave_keys(["no", "yes", "no", "no", "yes"], 5, 32, False, src)[4] == "V"      # (the dead slot re-runs the last env: its own flag)
    assert NC.wave_keys(["no", "yes", "no"], 3, 64, False, src) == ["P", "V", "P"]
    assert NC.wave_keys(["no"] * 3, 3, 32, True, src) == ["V"] * 3


def test_the_comparison_finds_a_planted_leak(oracle_mod):
    """mismatches(): silent on equal bits, loud on ONE flipped sign of zero in one occurrence of one subject, and it does not compare across
    groups"""
    P = NC.pools(oracle_mod, "A-32")
    A = NC.arrangement(P)
    n = A["nenv"]
    val = np.zeros((n, 3), np.float32)
    for e in range(n):
        val[e] = A["src"][e]      # a function of the env's inputs alone
    keys = ["P"] * n
    assert NC.mismatches(A, keys, dict(x=val)) == []
    e = int(np.flatnonzero(A["sid"] == A["subjects"][3])[5])
    leak = val.copy(); leak[e, 1] = -leak[e, 1] if leak[e, 1] != 0 else -0.0
    leak[e, 2] = np.float32(leak[e, 2]) * np.float32(1 + 2 ** -23)
    bad = NC.mismatches(A, keys, dict(x=leak))
    assert len(bad) == 1 and f"env {e} " in bad[0] and f"subject {A['subjects'][3]} " in bad[0], bad
    keys2 = list(keys); keys2[e] = "V"
    assert NC.mismatches(A, keys2, dict(x=leak)) == []      # (between the groups nothing is judged)
    assert NC.group_sizes(A, keys2)[:2] == (int((A["sid"] >= 0).sum()) - 1, 1)
