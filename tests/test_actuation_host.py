"""CPU checks of the actuation-fault stage of `track --actuation` / `--actuation_grid`: the C-ABI export and the slot names, the parsers
with every refusal by its flag, the filter coefficient against the reference's own numbers, the per-env fault rows, the numpy restatement
of `odk_action_apply` on its own (the all-nominal identity, the filter's step response, packet loss, freeze, the hash's statistics) and
`track`'s refusals next to another cell axis."""
import ctypes
import os
import re

import numpy as np
import pytest

from open_duck_playground_amd import actuation      # (fails at import before the stage exists)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU = 14
NAMES = [f"joint_{i}" for i in range(NU)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_libodk_exports_the_launch_and_engine_mirrors_every_slot():
    from open_duck_playground_amd import engine
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(lib, "odk_action_apply") and "odk_action_apply" in engine.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    assert re.search(r"\bint odk_action_apply\(const odk_batch\* b, const float\* act_dev", text)
    names = {k[4:]: v for k, v in engine.header_constants().items() if k.startswith("ACT_")}
    assert set(names) == set(re.findall(r"\bODK_ACT_([A-Z_]+)\b", text)), "a name the header mentions has no value here"
    assert len(names) == 19 and names["NPRM"] == 48 and names["NSTATE"] == 48
    for name, v in names.items():
        assert getattr(engine, "ACT_" + name) == v, name
    assert sorted(n for n in vars(engine) if n.startswith("ACT_")) == sorted("ACT_" + n for n in names)
    widths = dict(GAIN=1, NOISE=1, LIMIT=1, ALPHA=1, QUANT=1, DROP_P=1, DROP_LEN=1, SEED=1, OFFSET=16, FREEZE_AT=16)
    used = sorted(names[k] + i for k, w in widths.items() for i in range(w))
    assert len(set(used)) == len(used) and used[-1] == names["NPRM"] - 1
    widths = dict(HEAD=1, EPISODE=1, HOLD=1, CALLS=1, DROPS=1, FILT=16, PREV=16)
    used = sorted(names[k] + i for k, w in widths.items() for i in range(w))
    assert len(set(used)) == len(used) and used[-1] == names["NSTATE"] - 1
    rows = engine.Batch.action_fault_rows(3)
    assert rows.dtype == np.float32 and rows.shape == (3, 48)
    want = np.zeros(48, np.float32)
    want[[names["GAIN"], names["DROP_LEN"]]] = 1.0
    want[names["FREEZE_AT"]:names["FREEZE_AT"] + 16] = -1.0
    assert all(np.array_equal(bits(r), bits(want)) for r in rows)


def test_the_parsers():
    from open_duck_playground_amd import track
    s = actuation.parse_actuation("cutoff=37.5, drop=0.05,drop_len=3,freeze=joint_2,freeze_at=100")
    assert tuple(s) == actuation.ACTUATION_KEYS and track.actuations_from_args is actuation.actuations_from_args
    want = actuation.nominal_actuation()
    want.update(cutoff=37.5, drop=0.05, drop_len=3, freeze="joint_2", freeze_at=100)
    assert s == want and isinstance(s["drop_len"], int) and isinstance(s["freeze_at"], int)
    assert actuation.nominal_actuation() == dict(gain=1.0, offset=0.0, noise=0.0, limit=0.0, cutoff=0.0, quant=0.0, drop=0.0, drop_len=1,
                                                  freeze="none", freeze_at=0)
    grid = actuation.parse_actuation_grid("cutoff=5:40:3,drop=0:0.2:2")
    assert [(g["cutoff"], g["drop"]) for g in grid] == [(5.0, 0.0), (5.0, 0.2), (22.5, 0.0), (22.5, 0.2), (40.0, 0.0), (40.0, 0.2)]
    assert all(g["gain"] == 1.0 and g["freeze"] == "none" for g in grid)
    assert [g["drop_len"] for g in actuation.parse_actuation_grid("drop_len=1:4:4")] == [1, 2, 3, 4]
    for spec, message in (("slew=1", "--actuation: unknown key 'slew'"), ("gain=1,gain=2", "--actuation: key 'gain' given twice"),
                          ("drop=1.5", "--actuation: drop=1.5 is outside 0 .. 1"), ("drop=-0.1", "--actuation: drop=-0.1 is outside 0 .. 1"),
                          ("drop_len=1.5", "--actuation: drop_len=1.5 is not a whole number of control steps"),
                          ("drop_len=0", "--actuation: drop_len=0 is below 1"), ("freeze_at=-1", "--actuation: freeze_at=-1 is below 0"),
                          ("cutoff=-3", "--actuation: cutoff=-3 is negative"), ("quant=-0.1", "--actuation: quant=-0.1 is negative"),
                          ("gain=nan", "--actuation: gain=nan is not finite"), ("noise=loud", "--actuation: noise='loud' is not a number"),
                          ("limit", "--actuation: 'limit' is not KEY=VALUE"), ("", "--actuation: no key given")):
        with pytest.raises(ValueError, match=re.escape(message)):
            actuation.parse_actuation(spec)
    for spec, message in (("slew=0:1:2", "--actuation_grid: unknown key 'slew'"), ("drop=0:2:3", "--actuation_grid: drop=2.0 is outside 0 .. 1"),
                          ("drop_len=1:2:3", "--actuation_grid: drop_len=1.5 is not a whole number"),
                          ("cutoff=-5:5:2", "--actuation_grid: cutoff=-5.0 is negative"),
                          ("freeze=0:1:2", "--actuation_grid: freeze takes an actuator's name, not a range: give one --actuation freeze=NAME per joint"),
                          ("cutoff=5:40:3,cutoff=1:2:2", "--actuation_grid: key 'cutoff' given twice")):
        with pytest.raises(ValueError, match=re.escape(message)):
            actuation.parse_actuation_grid(spec)
    with pytest.raises(ValueError, match=re.escape("--actuation: freeze='elbow' is not one of the robot's actuators (joint_0, joint_1")):
        actuation.actuation_blocks(1, [actuation.parse_actuation("freeze=elbow")], 2, 0, 0.25, 0.02, NAMES)


def test_filter_alpha_is_the_references():
    assert actuation.filter_alpha(37.5, 0.02) == np.float32(4.0 / 7.0)      # the reference's own numbers: (1 / 37.5) / (1 / 50 + 1 / 37.5)
    assert actuation.filter_alpha(37.5, 0.02) == np.float32((1.0 / 37.5) / (1.0 / 50.0 + 1.0 / 37.5))
    assert actuation.filter_alpha(0, 0.02) == 0 and actuation.filter_alpha(0.0, 0.005) == 0
    assert bits(actuation.filter_alpha(0, 0.02)) == 0 and actuation.filter_alpha(30.0, 0.02).dtype == np.float32
    assert actuation.filter_alpha(50.0, 0.02) == np.float32(0.5)


def test_fault_rows_of_cells():
    from open_duck_playground_amd import engine
    scale, dt = 0.25, 0.02
    cells = [actuation.nominal_actuation(), actuation.parse_actuation("cutoff=37.5,quant=0.0015,drop=0.1,drop_len=3,freeze=joint_2,freeze_at=7,limit=0.9"),
             actuation.parse_actuation("offset=0.05,gain=1.1,noise=0.02")]
    rows = actuation.actuation_blocks(2, cells, 4, 7, scale, dt, NAMES)
    assert rows.dtype == np.float32 and rows.shape == (2 * 3 * 4, engine.ACT_NPRM)
    # the layout is cell_rows': per cell a marker through cell_rows lands where the rows' own settings are
    from open_duck_playground_amd.sweeps import cell_rows
    marker = cell_rows(np.float32([1.0, 1.0, 1.1]), 2, 4)
    assert np.array_equal(rows[:, engine.ACT_GAIN], marker)
    nominal = engine.action_fault_rows(1)[0]
    seeds = rows[:, engine.ACT_SEED]
    assert (seeds == np.floor(seeds)).all() and seeds.min() >= 0 and seeds.max() < 2 ** 24 and len(np.unique(seeds)) == seeds.size
    assert np.array_equal(seeds, actuation.env_seeds(7, 24)) and not np.array_equal(seeds, actuation.env_seeds(8, 24))
    unit = np.random.default_rng(7).uniform(-1.0, 1.0, (24, 16))      # drawn for every env, used by the cells with an offset
    for c in range(2):
        blk = rows[c * 12:(c + 1) * 12].copy()
        blk[:, engine.ACT_SEED] = 0
        assert all(np.array_equal(bits(r), bits(nominal)) for r in blk[0:4])      # bit for bit nominal: no -0.0 from a zero bound
        for r in blk[4:8]:
            assert r[engine.ACT_ALPHA] == np.float32(4 / 7) and r[engine.ACT_QUANT] == np.float32(0.0015 / scale) and r[engine.ACT_LIMIT] == np.float32(0.9)
            assert r[engine.ACT_DROP_P] == np.float32(0.1) and r[engine.ACT_DROP_LEN] == 3 and r[engine.ACT_GAIN] == 1 and r[engine.ACT_NOISE] == 0
            fz = r[engine.ACT_FREEZE_AT:engine.ACT_FREEZE_AT + 16]
            assert fz[2] == 7 and (np.delete(fz, 2) == -1).all() and not r[engine.ACT_OFFSET:engine.ACT_OFFSET + 16].any()
        off = blk[8:12, engine.ACT_OFFSET:engine.ACT_OFFSET + 16]
        assert (np.abs(off) <= 0.05 / scale).all() and len(np.unique(off)) == off.size and np.abs(off).max() > 0.04 / scale
        assert np.array_equal(off, (unit[c * 12 + 8:c * 12 + 12] * (0.05 / scale)).astype(np.float32))      # radians over action_scale
        assert (blk[8:12, engine.ACT_GAIN] == np.float32(1.1)).all() and (blk[8:12, engine.ACT_NOISE] == np.float32(0.02)).all()
    np.testing.assert_array_equal(rows[8], actuation.fault_row(cells[2], scale, dt, NAMES, unit[8], seeds[8]))
    assert np.array_equal(actuation.fault_row(cells[1], 0.5, dt, NAMES)[engine.ACT_QUANT], np.float32(0.0015 / 0.5))
    links = actuation.reduce_link(np.tile(np.float32([0, 0, 0, 8, 2] + [0] * 43), (6, 1)), 3, 2)
    assert links == [dict(dropped_share=0.25)] * 3 and actuation.reduce_link(np.zeros((2, 48), np.float32), 1, 2) == [dict(dropped_share=0.0)]


def _run(acts, fault, done=None, nu=NU):
    state = np.zeros((acts[0].shape[0], actuation.ACT_NSTATE), np.float32)
    return [actuation.action_apply_reference(a, None if done is None else done[t], fault, state, nu) for t, a in enumerate(acts)], state


def test_restatement_all_nominal_returns_every_bit():
    from open_duck_playground_amd import engine
    rng = np.random.default_rng(0)
    n, T = 9, 12
    odd = np.concatenate([np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0]), np.frombuffer(np.uint32(0xFFC12345).tobytes(), np.float32)])
    acts = [rng.standard_normal((n, NU)).astype(np.float32) for _ in range(T)]
    for a in acts:
        plant = rng.random(a.shape) < 0.3
        a[plant] = odd[rng.integers(0, 6, int(plant.sum()))]
    done = (rng.random((T, n)) < 0.2).astype(np.float32)
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_SEED] = actuation.env_seeds(3, n)
    for d in (done, None):
        out, state = _run(acts, fault, d)
        assert all(np.array_equal(bits(o), bits(a)) for o, a in zip(out, acts))
        assert (state[:, engine.ACT_CALLS] == T).all() and not state[:, engine.ACT_DROPS].any() and not state[:, engine.ACT_FILT:engine.ACT_PREV].any()
        assert np.array_equal(bits(state[:, engine.ACT_PREV:engine.ACT_PREV + NU]), bits(acts[-1]))
    assert (state[:, engine.ACT_HEAD] == T).all() and (state[:, engine.ACT_EPISODE] == 1).all()      # (done = None: one episode)


def test_restatement_filter_follows_the_step_response():
    from open_duck_playground_amd import engine
    alpha = actuation.filter_alpha(37.5, 0.02)
    fault = engine.action_fault_rows(1)
    fault[:, engine.ACT_ALPHA] = alpha
    T = 40
    out, state = _run([np.ones((1, NU), np.float32)] * T, fault)
    a64 = float(alpha)
    for k, o in enumerate(out):      # y_k = 1 - alpha^(k + 1) from y_-1 = 0; each step rounds a product twice and a sum once
        want = 1.0 - a64 ** (k + 1)
        assert np.abs(o.astype(np.float64) - want).max() <= 4 * (k + 1) * np.spacing(np.float32(want)), k
    assert np.array_equal(state[0, engine.ACT_FILT:engine.ACT_FILT + NU], out[-1][0]) and not state[0, engine.ACT_FILT + NU:engine.ACT_PREV].any()


def test_restatement_drop_one_delivers_zeros_for_every_episode():
    from open_duck_playground_amd import engine
    rng = np.random.default_rng(1)
    n, T = 4, 20
    acts = [rng.standard_normal((n, NU)).astype(np.float32) + 3 for _ in range(T)]
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_DROP_P] = 1.0
    done = np.zeros((T, n), np.float32)
    done[9, :2] = 1.0
    out, state = _run(acts, fault, done)
    assert not np.stack(out).any(), "every packet lost: the servos keep the episode's first target, action 0"
    assert (state[:, engine.ACT_DROPS] == T).all() and (state[:, engine.ACT_CALLS] == T).all()
    assert list(state[:, engine.ACT_EPISODE]) == [2, 2, 1, 1] and list(state[:, engine.ACT_HEAD]) == [T - 9, T - 9, T, T]
    # and a loss that ends: with drop back at 0 the next packet arrives
    fault[:, engine.ACT_DROP_P] = 0.0
    nxt = actuation.action_apply_reference(acts[0], None, fault, state, NU)
    assert np.array_equal(bits(nxt), bits(acts[0]))


def test_restatement_freeze_holds_the_value_before():
    from open_duck_playground_amd import engine
    rng = np.random.default_rng(2)
    n, T = 3, 12
    acts = [rng.standard_normal((n, NU)).astype(np.float32) for _ in range(T)]
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_FREEZE_AT + 3] = 5.0
    fault[1, engine.ACT_FREEZE_AT + 0] = 0.0      # frozen from the first step: the default pose
    out, _ = _run(acts, fault)
    for t in range(T):
        want = acts[t].copy()
        if t >= 5:
            want[:, 3] = acts[4][:, 3]            # call 4's value
        want[1, 0] = 0.0
        assert np.array_equal(bits(out[t]), bits(want)), t
    done = np.zeros((T, n), np.float32)
    done[8] = 1.0                                  # a new episode: the servo works again until its step 5
    out, _ = _run(acts, fault, done)
    assert np.array_equal(out[7][:, 3], acts[4][:, 3]) and np.array_equal(out[8][:, 3], acts[8][:, 3]) and np.array_equal(out[11][:, 3], acts[11][:, 3])


def _lost(out, acts):
    return np.stack([~(o == a).all(axis=1) for o, a in zip(out, acts)])      # [T, n]: the delivered row is not the asked one


def test_restatement_losses_come_in_runs_of_drop_len():
    from open_duck_playground_amd import engine
    n, T = 16, 200
    acts = [np.full((n, NU), t + 1, np.float32) for t in range(T)]      # every call its own value: a held row shows
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_DROP_P], fault[:, engine.ACT_DROP_LEN], fault[:, engine.ACT_SEED] = 0.1, 3, actuation.env_seeds(5, n)
    out, state = _run(acts, fault)
    lost = _lost(out, acts)
    assert np.array_equal(lost.sum(axis=0), state[:, engine.ACT_DROPS]) and lost.any()
    for e in range(n):
        runs = [len(r) for r in "".join("x" if v else "." for v in lost[:, e]).split(".") if r]
        runs = runs[:-1] if lost[-1, e] else runs      # (a run the end of the calls may have cut short is left out)
        assert runs and all(r % 3 == 0 for r in runs), (e, runs)      # runs of three; two draws in a row make six
        t0 = int(np.argmax(lost[:, e]))
        assert (np.stack(out)[t0:t0 + 3, e] == float(t0)).all()      # the value delivered before the loss, three times


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_restatement_loss_share_and_noise_correlation(seed):
    from open_duck_playground_amd import engine
    n, T, p = 64, 256, 0.25
    acts = [np.full((n, NU), t + 1, np.float32) for t in range(T)]
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_DROP_P], fault[:, engine.ACT_SEED] = p, seed      # (one seed for every env: the env index alone tells them apart)
    out, state = _run(acts, fault)
    share = state[:, engine.ACT_DROPS].sum() / state[:, engine.ACT_CALLS].sum()
    N = n * T
    assert state[:, engine.ACT_CALLS].sum() == N and abs(share - p) <= 5 * np.sqrt(p * (1 - p) / N), share      # 0.0169
    # the noise: zero actions, amplitude 1 -> the delivered action is the draw itself, uniform in -1 .. 1, adjacent lanes uncorrelated
    fault = engine.action_fault_rows(n)
    fault[:, engine.ACT_NOISE], fault[:, engine.ACT_SEED] = 1.0, seed
    out, _ = _run([np.zeros((n, NU), np.float32)] * T, fault)
    x = np.stack(out).astype(np.float64)      # [T, n, NU]
    assert x.min() >= -1 and x.max() < 1 and abs(x.mean()) < 5 / np.sqrt(3 * x.size) and abs(x.var() - 1 / 3) < 0.01
    for shifted, axis in ((x[:, :, 1:], 2), (x[1:], 0), (x[:, 1:], 1)):      # adjacent lanes, steps, envs
        base = x[:, :, :-1] if axis == 2 else (x[:-1] if axis == 0 else x[:, :-1])
        r = np.corrcoef(base.ravel(), shifted.ravel())[0, 1]
        assert abs(r) < 5 / np.sqrt(base.size), (axis, r)


REFUSALS = [
    (["--actuation", "slew=1"], "--actuation: unknown key 'slew'"),
    (["--actuation_grid", "freeze=0:1:2"], "--actuation_grid: freeze takes an actuator's name, not a range"),
    (["--actuation", "drop=2"], "--actuation: drop=2 is outside 0 .. 1"),
    (["--actuation", "cutoff=10", "--push_grid", "magnitude=0:1:2"], "--actuation / --actuation_grid do not combine with --push / --push_grid.*third cell axis"),
    (["--actuation_grid", "drop=0:0.2:2", "--push", "1", "0"], "--actuation / --actuation_grid do not combine with --push / --push_grid.*third cell axis"),
    (["--actuation", "cutoff=10", "--plant", "kp=0.6"], "--actuation / --actuation_grid do not combine with --plant / --plant_grid.*third cell axis"),
    (["--actuation_grid", "drop=0:0.2:2", "--sensor", "gyro_bias_y=0.2"], "--actuation / --actuation_grid do not combine with --sensor / --sensor_grid.*third cell axis"),
]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_come_before_any_batch_work(flags, message):
    """Each as `run` raises it through `main`: SystemExit before any batch is made (no GPU here, so getting that far would be another error)."""
    from open_duck_playground_amd import track
    argv = ["--checkpoint", "c.pt", "--command", "0", "0", "0", "--episode_length", "100"] + flags
    with pytest.raises(SystemExit, match=message):
        track.actuations_from_args(track.build_parser().parse_args(argv))
    with pytest.raises(SystemExit, match=message):
        track.main(argv)
    plain = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0"])
    assert track.actuations_from_args(plain) == [] and plain.actuation is None and plain.actuation_grid is None


def test_robustness_lines_run_around_each_keys_nominal():
    """hand-made cells: `off` (0) ends the cutoff line above the largest cutoff, so the drop line is taken at the mildest filter"""
    from open_duck_playground_amd import track
    assert [actuation.actuation_order("cutoff", v) for v in (5.0, 40.0, 0.0)] == [-0.2, -0.025, 0.0]
    assert actuation.actuation_order("drop", 0.2) == 0.2 and actuation.actuation_order("freeze", "none") == 0 and actuation.actuation_order("freeze", "x") == 1
    cells = []
    for cutoff, drop, fall in ((5.0, 0.0, 0.5), (5.0, 0.2, 0.9), (20.0, 0.0, 0.04), (20.0, 0.2, 0.3), (40.0, 0.0, 0.0), (40.0, 0.2, 0.02)):
        cells.append(dict(actuation=dict(actuation.nominal_actuation(), cutoff=cutoff, drop=drop), fall_rate=fall, rms_error_vx=0.0, rms_error_vy=0.0,
                          rms_error_wz=0.0, mean_episode_reward=0.0))
    rb = track.reduce_robustness(cells, 0.05, "actuation", actuation.nominal_actuation(), actuation.actuation_order)
    assert set(rb) == {"robust_fall_rate", "cutoff", "drop", "survived_range"}
    assert [p["value"] for p in rb["cutoff"]] == [5.0, 20.0, 40.0] and [p["fall_rate"] for p in rb["cutoff"]] == [0.5, 0.04, 0.0]      # at drop = 0
    assert [p["value"] for p in rb["drop"]] == [0.0, 0.2] and [p["fall_rate"] for p in rb["drop"]] == [0.0, 0.02]      # at cutoff = 40
    assert rb["survived_range"] == {"cutoff": [20.0, 40.0], "drop": [0.0, 0.2]}
