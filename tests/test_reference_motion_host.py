"""Reference-motion loader (open_duck_playground_amd/reference_motion.py) against the reference's PolyReferenceMotion semantics
(poly_reference_motion.py:74-168), the imitation joint maps (custom_rewards.py:80-88) and the command-line plumbing; no GPU."""
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN
from open_duck_playground_amd import reference_motion as RM

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")


def _entry(coeffs_lowest_first, period=0.54, fps=50):
    """One value of the reference's dict: `dim_k` lists of np.float64, lowest order first."""
    return dict(period=period, fps=fps, coefficients={f"dim_{k}": [np.float64(c) for c in row] for k, row in enumerate(coeffs_lowest_first)},
                frame_offsets={}, startend_double_support_ratio=1.0, start_offset=50, nb_steps_in_period=int(period * fps))


def _shipped_pickle(prm_arrays):
    t64 = prm_arrays["table64"]
    data = {}
    for ix, dx in enumerate(prm_arrays["dxs"]):
        for iy, dy in enumerate(prm_arrays["dys"]):
            for it, dth in enumerate(prm_arrays["dthetas"]):
                data[f"{dx}_{dy}_{dth}"] = _entry(t64[ix, iy, it][:, ::-1])
    return pickle.dumps(data)


def _synthetic(J=3, K=4, grid=((0.1, 0.2), (0.0,), (0.0,)), period=0.4, fps=50, seed=0):
    rng = np.random.default_rng(seed)
    return {f"{dx}_{dy}_{dth}": _entry(rng.uniform(-1, 1, (2 * J + 8, K)), period, fps)
            for dx in grid[0] for dy in grid[1] for dth in grid[2]}


def _load(data):
    return RM.ReferenceMotion.from_bytes(pickle.dumps(data))


def _midpoint_tie(m, q):
    for v, grid, rng in ((q[0], m.dxs, m.dx_range), (q[1], m.dys, m.dy_range), (q[2], m.dthetas, m.dtheta_range)):
        d = np.sort(np.abs(grid - np.clip(v, rng[0], rng[1])))
        if len(d) > 1 and d[1] - d[0] < 1e-6:
            return True
    return False


def test_round_trip_of_the_shipped_table(prm_arrays, tmp_path):
    p = tmp_path / "polynomial_coefficients.pkl"
    p.write_bytes(_shipped_pickle(prm_arrays))
    m = RM.ReferenceMotion.from_pickle(str(p))
    prm = m.prm()
    assert prm["table"].dtype == np.float32 and np.array_equal(prm["table"].view(np.int32), prm_arrays["table"].view(np.int32))
    for k in ("dxs", "dys", "dthetas", "dx_range", "dy_range", "dtheta_range"):
        np.testing.assert_array_equal(prm[k], prm_arrays[k])
    assert m.nb_steps_in_period == int(prm["nb_steps_in_period"][0]) == 27 and (m.n_joints, m.n_dims, m.n_coeffs) == (16, 40, 16)
    import hashlib
    assert m.sha256 == hashlib.sha256(p.read_bytes()).hexdigest()
    g = np.load(os.path.join(GOLDEN, "reference_motion.npz"))
    n = 0
    for q, exp in zip(g["query"], g["expected"]):
        if _midpoint_tie(m, q):
            continue
        np.testing.assert_allclose(m.evaluate(q[0], q[1], q[2], int(q[3])), exp, rtol=1e-9, atol=1e-9)
        n += 1
    assert n > 50
    shipped = RM.ReferenceMotion.from_npz()
    assert np.array_equal(shipped.table, prm_arrays["table"]) and shipped.nb_steps_in_period == 27


def test_ranges_are_anchored_at_zero():
    m = _load(_synthetic(grid=((0.1, 0.2), (-0.3, -0.1), (0.5,))))
    assert list(m.dx_range) == [0.0, 0.2] and list(m.dy_range) == [-0.3, 0.0] and list(m.dtheta_range) == [0.0, 0.5]
    # a command below the positive-only dx grid clips at 0, then picks the nearest point (0.1)
    assert m.index(-1.0, 0.0, 0.0) == (0, 1, 0)


def test_steps_in_period_truncate_in_float64():
    assert _load(_synthetic(period=0.58, fps=50)).nb_steps_in_period == 28     # 0.58 * 50 = 28.999999999999996
    assert _load(_synthetic(period=0.54, fps=50)).nb_steps_in_period == 27


def test_first_entry_period_wins():
    d = _synthetic(grid=((0.1, 0.2), (0.0,), (0.0,)))
    k0, k1 = list(d)
    d[k0]["period"], d[k1]["period"] = 0.4, 0.8
    assert _load(d).nb_steps_in_period == 20
    d2 = {k1: d[k1], k0: d[k0]}
    m2 = _load(d2)
    assert m2.nb_steps_in_period == 40 and list(m2.dxs) == [0.1, 0.2]     # grids sorted whatever the key order


def test_ties_go_to_the_first_index():
    m = _load(_synthetic(grid=((0.0, 0.5), (0.0,), (0.0,))))
    assert m.index(0.25, 0.0, 0.0) == (0, 0, 0)
    assert m.index(0.2500001, 0.0, 0.0) == (1, 0, 0)


def test_low_degree_table_pads_with_leading_zeros():
    J, K = 4, 8
    m = _load(_synthetic(J=J, K=K, grid=((0.1,), (0.0,), (0.0,)), seed=3))
    t32 = m.prm()["table"][0, 0, 0]
    assert np.all(t32[:, :16 - K] == 0)
    used = [RM.canonical_row(f, J) for f in range(m.n_dims)]
    assert np.all(t32[[r for r in range(40) if r not in used]] == 0)
    n = m.nb_steps_in_period
    for i in range(n):
        t = np.float32((i % n) / n)
        # 16-coefficient float32 fma Horner on the padded row == the same Horner over the K source coefficients
        for f, r in enumerate(used):
            y16 = np.float32(t32[r, 0])
            for q in range(1, 16):
                y16 = np.float32(np.float64(y16) * np.float64(t) + np.float64(t32[r, q]))
            yk = np.float32(t32[r, 16 - K])
            for q in range(16 - K + 1, 16):
                yk = np.float32(np.float64(yk) * np.float64(t) + np.float64(t32[r, q]))
            assert y16 == yk
        np.testing.assert_allclose(m.evaluate(0.1, 0.0, 0.0, i)[:J], [np.polyval(m.table64[0, 0, 0, f], (i % n) / n) for f in range(J)], rtol=1e-12)


@pytest.mark.parametrize("case, match", [
    ("J17", "J = 17"),
    ("odd", "even"),
    ("small", "even number >= 10"),
    ("K17", "17 coefficients"),
    ("grid17", "17 dx grid points"),
    ("missing", "has no entry"),
    ("mixed_dims", "first entry"),
    ("mixed_coeffs", "first entry"),
    ("mixed_within", "mixes polynomials"),
    ("badkey", "is not '<dx>_<dy>_<dtheta>'"),
])
def test_refusals(case, match):
    if case == "J17":
        d = _synthetic(J=17, grid=((0.1,), (0.0,), (0.0,)))
    elif case == "odd":
        d = {"0.1_0_0": _entry(np.zeros((13, 4)))}
    elif case == "small":
        d = {"0.1_0_0": _entry(np.zeros((8, 4)))}
    elif case == "K17":
        d = _synthetic(J=2, K=17, grid=((0.1,), (0.0,), (0.0,)))
    elif case == "grid17":
        d = _synthetic(J=2, grid=(tuple(0.01 * i for i in range(17)), (0.0,), (0.0,)))
    elif case == "missing":
        d = _synthetic(J=2, grid=((0.1, 0.2), (0.0, 0.1), (0.0,)))
        d.pop(next(iter(d)))
    elif case == "mixed_dims":
        d = {"0.1_0_0": _entry(np.zeros((12, 4))), "0.2_0_0": _entry(np.zeros((14, 4)))}
    elif case == "mixed_coeffs":
        d = {"0.1_0_0": _entry(np.zeros((12, 4))), "0.2_0_0": _entry(np.zeros((12, 5)))}
    elif case == "mixed_within":
        e = _entry(np.zeros((12, 4)))
        e["coefficients"]["dim_3"] = [np.float64(0.0)] * 5
        d = {"0.1_0_0": e}
    else:
        d = {"0.1_0": _entry(np.zeros((12, 4)))}
    with pytest.raises(ValueError, match=match):
        _load(d)


class _Trap:
    called = []


def _trap(*a):
    _Trap.called.append(a)
    return 0


def test_a_pickle_naming_another_global_is_refused_without_calling_it():
    # protocol 0 text: builtins.eval('...') -- the loader must refuse the global before anything is called
    raw = b"cbuiltins\neval\n(V_Trap_should_not_run\ntR."
    with pytest.raises(pickle.UnpicklingError, match="builtins.eval"):
        RM.safe_load(raw)
    global_call = pickle.dumps(_trap_obj())
    with pytest.raises(pickle.UnpicklingError, match="_trap"):
        RM.ReferenceMotion.from_bytes(global_call)
    assert _Trap.called == []
    # numpy arrays and scalars (both module spellings through numpy's own pickling) are accepted
    arr = RM.safe_load(pickle.dumps({"a": np.arange(3.0), "s": np.float64(1.5), "dt": np.dtype("float32")}))
    assert np.array_equal(arr["a"], np.arange(3.0)) and arr["s"] == 1.5


class _trap_obj:
    def __reduce__(self):
        return (_trap, ("called",))


def _duck():
    from open_duck_playground_amd.model import load_task_model
    return load_task_model("flat_terrain")


def _robot(name):
    from open_duck_playground_amd.model import Model
    return Model.from_xml(os.path.join(ASSETS, name))


def test_duck_default_map_is_the_reference_slices(prm_arrays):
    m = RM.ReferenceMotion.from_npz()
    assert RM.imitation_joint_map(_duck(), m) == [0, 1, 2, 3, 4, -1, -1, -1, -1, 11, 12, 13, 14, 15]
    # explicit names: the same map; leaving out a leg joint drops it
    assert RM.imitation_joint_map(_duck(), m, list(RM.DUCK_FRAME_JOINTS), list(RM.DUCK_UNDRIVEN)) == [0, 1, 2, 3, 4, -1, -1, -1, -1, 11, 12, 13, 14, 15]
    assert RM.imitation_joint_map(_duck(), m, ignore=["left_antenna", "right_antenna", "left_knee"])[3] == -1
    with pytest.raises(ValueError, match="left_antenna"):
        RM.imitation_joint_map(_duck(), m, list(RM.DUCK_FRAME_JOINTS))      # antennas named, not ignored (the duck's models have none)


def test_robot_default_maps():
    b12 = _robot("biped12.xml")
    m12 = _load(_synthetic(J=12, grid=((0.1,), (0.0,), (0.0,))))
    assert RM.imitation_joint_map(b12, m12) == list(range(12))
    tb = _robot("tail_biped.xml")
    m15 = _load(_synthetic(J=15, grid=((0.1,), (0.0,), (0.0,))))
    act = RM.actuated_joint_names(tb)
    mp = RM.imitation_joint_map(tb, m15)
    for u, n in enumerate(act):
        assert mp[u] == (-1 if n.startswith("tail") else u)
    assert sum(v >= 0 for v in mp) == 10


def test_map_errors():
    b12 = _robot("biped12.xml")
    m12 = _load(_synthetic(J=12, grid=((0.1,), (0.0,), (0.0,))))
    m10 = _load(_synthetic(J=10, grid=((0.1,), (0.0,), (0.0,))))
    with pytest.raises(ValueError, match="J = 10.*nu = 12"):
        RM.imitation_joint_map(b12, m10)
    names = RM.actuated_joint_names(b12)
    with pytest.raises(ValueError, match="not a joint of the model"):
        RM.imitation_joint_map(b12, m12, names[:-1] + ["no_such_joint"])
    tb = _robot("tail_biped.xml")
    free = [str(n) for n in tb.a["names_jnt"] if str(n) not in RM.actuated_joint_names(tb)]
    if free:     # a joint of the model that no actuator drives
        m15 = _load(_synthetic(J=15, grid=((0.1,), (0.0,), (0.0,))))
        with pytest.raises(ValueError, match="driven by no actuator"):
            RM.imitation_joint_map(tb, m15, RM.actuated_joint_names(tb)[:-1] + [free[0]])
    with pytest.raises(ValueError, match="not one of the frame's joints"):
        RM.imitation_joint_map(b12, m12, ignore=["no_such_joint"])
    with pytest.raises(ValueError, match="given twice"):
        RM.imitation_joint_map(b12, m12, names[:-1] + [names[0]])
    with pytest.raises(ValueError, match="11 names"):
        RM.imitation_joint_map(b12, m12, names[:-1])
    # a 10-joint frame of the legs without the ankle rolls: explicit names
    legs = [n for n in names if "ankle_roll" not in n]
    mp = RM.imitation_joint_map(b12, m10, legs)
    assert [mp[names.index(n)] for n in legs] == list(range(10)) and sum(v < 0 for v in mp) == 2


def test_runner_and_track_flags_reach_config_overrides():
    from open_duck_playground_amd import runner, track
    a = runner.build_parser().parse_args(["--reference_motion", "m.pkl", "--imitation_joints", "a, b,c", "--imitation_ignore", "c"])
    ov = runner.config_overrides(a)
    assert ov["reference_motion"] == "m.pkl" and ov["imitation_joints"] == ["a", "b", "c"] and ov["imitation_ignore"] == ["c"]
    assert runner.config_overrides(runner.build_parser().parse_args([])) is None
    t = track.build_parser().parse_args(["--checkpoint", "x.pt", "--reference_motion", "m.pkl", "--imitation_joints", "a,b"])
    ov = track.config_overrides(t)
    assert ov["reference_motion"] == "m.pkl" and ov["imitation_joints"] == ["a", "b"] and "imitation_ignore" not in ov
    assert "reference_motion" not in track.config_overrides(track.build_parser().parse_args(["--checkpoint", "x.pt"]))


def test_standing_refuses_a_reference_motion():
    from open_duck_playground_amd import standing
    with pytest.raises(ValueError, match="Standing"):
        standing.Standing(config_overrides={"reference_motion": "m.pkl"}, num_envs=8)


def test_library_exports_set_imitation_joints():
    from open_duck_playground_amd import engine
    assert "odk_batch_set_imitation_joints" in engine.EXPORTED_SYMBOLS
    L = engine.load_library()
    assert hasattr(L, "odk_batch_set_imitation_joints")
    hdr = open(os.path.join(os.path.dirname(ASSETS), "..", "include", "odk.h")).read()
    assert "int odk_batch_set_imitation_joints(odk_batch* b, const int32_t* frame_joint, int nu);" in hdr
