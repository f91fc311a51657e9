"""Host-side checks (no GPU) of caller-given action delays and the plant sweep of `python -m open_duck_playground_amd.track`: the exported
symbol, what `check_action_delays` refuses, `--plant` / `--plant_grid` parsing, the (command, plant) block layout, the set_param arrays
as nominal times scale, the refusal next to pushes before any device call, and `survived_range` / `reduce_robustness` on hand-made rows."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_libodk_exports_the_delay_binding():
    from open_duck_playground_amd import engine
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(lib, "odk_batch_bind_action_delays"), "libodk.so does not export odk_batch_bind_action_delays"
    assert "odk_batch_bind_action_delays" in engine.EXPORTED_SYMBOLS
    L = engine.load_library()
    assert L.odk_batch_bind_action_delays.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    assert "int odk_batch_bind_action_delays(odk_batch* b, const int32_t* delay_dev, int row_stride);" in text
    # a null batch is refused by the C ABI itself (no device needed)
    assert L.odk_batch_bind_action_delays(None, None, 0) == -1


def test_the_poison_build_carries_the_binding():
    from open_duck_playground_amd import engine
    if not os.path.exists(engine.POISON_LIB_PATH):
        engine.build_library(poison=True)
    assert hasattr(ctypes.CDLL(engine.POISON_LIB_PATH), "odk_batch_bind_action_delays")


def test_check_action_delays_refuses_with_value_errors():
    import torch
    from open_duck_playground_amd import engine
    n = 8
    bad = [
        (np.zeros(n, np.int32), "torch tensor"),
        (torch.zeros(n), "int32"),
        (torch.zeros(n, dtype=torch.int64), "int32"),
        (torch.zeros(n, dtype=torch.int32), "cuda:0"),            # a CPU tensor
        (torch.zeros(n, 1, dtype=torch.int32), "cuda:0"),
    ]
    for t, word in bad:
        with pytest.raises(ValueError, match=word) as err:
            engine.check_action_delays(t, n, 0)
        assert isinstance(err.value, engine.OdkError)              # `except OdkError` call sites keep catching it
    # shape and stride are judged before anything touches a device: a meta tensor "on" cuda:0 carries them without one
    meta = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="meta")

    class OnDevice:
        """a tensor's metadata with the device check satisfied"""
        def __init__(self, t):
            self.t = t
            self.dtype, self.shape = t.dtype, t.shape
            self.device = torch.device("cuda", 0)
        def dim(self): return self.t.dim()
        def stride(self, k): return self.t.stride(k)

    import unittest.mock as mock
    with mock.patch.object(torch, "is_tensor", lambda x: True):
        engine.check_action_delays(OnDevice(meta(n)), n, 0)
        engine.check_action_delays(OnDevice(meta(n + 5)), n, 0)                      # more rows than envs: legal
        engine.check_action_delays(OnDevice(meta(n, 4)), n, 0)                       # a wider row: the stride is the tensor's
        engine.check_action_delays(OnDevice(meta(2 * n)[::2]), n, 0)                 # a strided view: stride 2
        for t, word in ((meta(n - 1), "shape"), (meta(n, 0), "shape"), (meta(n, 2, 2), "shape"), (meta(1).expand(n), "stride")):
            with pytest.raises(ValueError, match=word):
                engine.check_action_delays(OnDevice(t), n, 0)


def test_plant_parsing():
    from open_duck_playground_amd import track
    assert track.nominal_plant() == dict(kp=1.0, mass=1.0, frictionloss=1.0, armature=1.0, delay="random")
    assert track.parse_plant("kp=0.6,delay=2") == dict(kp=0.6, mass=1.0, frictionloss=1.0, armature=1.0, delay=2)
    assert track.parse_plant(" mass=1.2 , frictionloss=2, armature=0.5, delay=random") == dict(kp=1.0, mass=1.2, frictionloss=2.0, armature=0.5,
                                                                                              delay="random")
    assert track.parse_plant("delay=1.0")["delay"] == 1 and isinstance(track.parse_plant("delay=1.0")["delay"], int)
    for spec, word in (("stiffness=2", "unknown axis"), ("kp=0.5,kp=0.6", "twice"), ("delay=1.5", "whole number"), ("delay=3", "outside"),
                       ("delay=-1", "outside"), ("delay=soon", "not 0, 1, 2"), ("kp=0", "scale > 0"), ("mass=-1", "scale > 0"), ("kp=nan", "scale > 0"),
                       ("kp=big", "not a number"), ("kp", "KEY=VALUE"), ("", "no axis")):
        with pytest.raises(ValueError, match=word):
            track.parse_plant(spec)
    g = track.parse_plant_grid("kp=0.5:1.0:2,delay=0:2:3")
    assert [(p["kp"], p["delay"]) for p in g] == [(0.5, 0), (0.5, 1), (0.5, 2), (1.0, 0), (1.0, 1), (1.0, 2)]      # the last axis varies fastest
    assert all(p["mass"] == p["frictionloss"] == p["armature"] == 1.0 for p in g)
    assert len(track.parse_plant_grid("kp=0.7:1.3:4,mass=0.9:1.2:3,delay=0:2:3")) == 36
    assert [p["delay"] for p in track.parse_plant_grid("delay=1:1:1")] == [1]
    for spec, word in (("stiffness=0:1:2", "unknown axis"), ("kp=0.5:1:2,kp=1:2:2", "twice"), ("delay=0:2:2,kp=1:1:1", None), ("delay=0:2:4", "whole number"),
                       ("delay=0:3:4", "outside"), ("delay=-1:1:3", "outside"), ("kp=0.5:1", "start:stop:count"), ("kp=0.5:1:0", "count >= 1"),
                       ("kp=0:1:3", "scale > 0"), ("kp=a:b:c", "start:stop:count"), ("", "no axis")):
        if word is None:
            assert [p["delay"] for p in track.parse_plant_grid(spec)] == [0, 2]
            continue
        with pytest.raises(ValueError, match=word):
            track.parse_plant_grid(spec)


def test_plant_block_layout():
    from open_duck_playground_amd import track
    commands = [track.command_row([0, 0, 0]), track.command_row([0.1, 0, 0.5])]
    plants = [track.parse_plant("kp=0.6,delay=2"), track.parse_plant("kp=1.0"), track.parse_plant("mass=1.2,delay=0")]
    E = 4
    cmd, scales, delays = track.plant_blocks(commands, plants, E)
    n = 2 * 3 * E
    assert cmd.shape == (n, 7) and cmd.dtype == np.float32 and delays.shape == (n,) and delays.dtype == np.int32
    assert set(scales) == set(track.PLANT_SCALE_AXES) and all(v.shape == (n,) and v.dtype == np.float64 for v in scales.values())
    for c in range(2):
        for p in range(3):
            blk = slice((c * 3 + p) * E, (c * 3 + p + 1) * E)          # command blocks outermost: `cell_blocks`' layout
            np.testing.assert_array_equal(cmd[blk], np.tile(np.asarray(commands[c], np.float32), (E, 1)))
            for axis in track.PLANT_SCALE_AXES:
                np.testing.assert_array_equal(scales[axis][blk], plants[p][axis])
            np.testing.assert_array_equal(delays[blk], {"random": -1}.get(plants[p]["delay"], plants[p]["delay"]))
    np.testing.assert_array_equal(cmd, track.cell_blocks(commands, [track.push_entry(0, 0)] * 3, E)[0])


def test_set_param_arrays_are_nominal_times_scale(model_a):
    """what `randomize.apply` hands odk_batch_set_param per block: the model's value times the cell's scale on the named axes, the model's
    value untouched everywhere else; an all-ones plant is the nominal model in float32, bit for bit"""
    from open_duck_playground_amd import engine, randomize, track
    a = model_a.a
    plants = [track.parse_plant("kp=0.6,delay=2"), track.nominal_plant(), track.parse_plant("mass=1.25,frictionloss=2,armature=0.5")]
    E = 3
    _, scales, _ = track.plant_blocks([track.command_row([0, 0, 0])], plants, E)
    fields = track.plant_fields(model_a, scales)
    act_jnt = np.asarray(a["actuator_trnid"]).reshape(model_a.nu, -1)[:, 0]
    dofs, qadr = np.asarray(a["jnt_dofadr"])[act_jnt], np.asarray(a["jnt_qposadr"])[act_jnt]
    nominal = dict(body_mass=np.asarray(a["body_mass"], np.float64), actuator_gainprm=np.asarray(a["actuator_gainprm0"], np.float64),
                   dof_frictionloss=np.asarray(a["dof_frictionloss"], np.float64)[dofs], dof_armature=np.asarray(a["dof_armature"], np.float64)[dofs],
                   qpos0=np.asarray(a["qpos0"], np.float64)[qadr], body_ipos=np.asarray(a["body_ipos"], np.float64)[randomize.TORSO_BODY_ID])
    scale_of = dict(body_mass="mass", actuator_gainprm="kp", dof_frictionloss="frictionloss", dof_armature="armature")
    for name, nom in nominal.items():
        assert fields[name].shape == (3 * E,) + nom.shape, name
        for p, plant in enumerate(plants):
            want = nom * plant[scale_of[name]] if name in scale_of else nom
            for e in range(p * E, (p + 1) * E):
                np.testing.assert_array_equal(fields[name][e], want, err_msg=f"{name} plant {p}")
        one = fields[name][E].astype(np.float32)                        # the all-ones plant
        np.testing.assert_array_equal(one.view(np.int32), nom.astype(np.float32).view(np.int32), err_msg=name)
    np.testing.assert_array_equal(fields["actuator_biasprm"], -fields["actuator_gainprm"])      # the bias follows the gain
    assert float(nominal["dof_frictionloss"].min()) > 0 and float(nominal["dof_armature"].min()) > 0 and nominal["body_mass"].max() > 0
    # the six arrays reach set_param with the per-env widths odk_batch_set_param expects, in randomize.apply's order
    calls = []

    class FakeBatch:
        def set_param(self, param, values):
            calls.append((param, np.asarray(values).shape))
    randomize.apply(FakeBatch(), fields)
    nb, nu = model_a.nbody, model_a.nu
    assert calls == [(engine.PARAM_BODY_MASS, (9, nb)), (engine.PARAM_BODY_IPOS_TORSO, (9, 3)), (engine.PARAM_DOF_FRICTIONLOSS, (9, nu)),
                     (engine.PARAM_DOF_ARMATURE, (9, nu)), (engine.PARAM_QPOS0, (9, nu)), (engine.PARAM_KP, (9, nu))]
    # a domain_randomize draw is multiplied, not replaced
    draw = randomize.domain_randomize(model_a, np.random.default_rng(0), 3 * E)[0]
    both = track.plant_fields(model_a, scales, draw)
    np.testing.assert_array_equal(both["actuator_gainprm"][:E], draw["actuator_gainprm"][:E] * 0.6)
    np.testing.assert_array_equal(both["body_mass"][2 * E:], draw["body_mass"][2 * E:] * 1.25)
    np.testing.assert_array_equal(both["qpos0"], draw["qpos0"])
    with pytest.raises(ValueError, match="unknown plant scale"):
        randomize.scale_fields(draw, {"delay": np.ones(3 * E)})


def test_plants_next_to_pushes_are_refused_before_any_device_call(monkeypatch):
    from open_duck_playground_amd import track
    called = []
    monkeypatch.setattr(track, "make_env", lambda *a, **k: called.append("make_env"))
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: called.append("set_device"))
    base = ["--checkpoint", "none.pt", "--command", "0", "0", "0"]
    for extra in (["--plant", "kp=0.6", "--push", "0.5", "0"], ["--plant_grid", "delay=0:2:3", "--push_grid", "magnitude=0:1:2"],
                  ["--plant", "kp=0.6", "--push_grid", "magnitude=0:1:2"]):
        with pytest.raises(SystemExit, match="third cell axis"):
            track.run(track.build_parser().parse_args(base + extra))
    for extra, word in ((["--plant", "delay=1.5"], "whole number"), (["--plant_grid", "delay=0:2:4"], "whole number"), (["--plant", "gain=2"], "unknown axis"),
                        (["--plant", "kp=0.5,kp=0.6"], "twice"), (["--plant", "kp=0.8", "--robust_fall_rate", "1.5"], "--robust_fall_rate")):
        with pytest.raises(SystemExit, match=word):
            track.run(track.build_parser().parse_args(base + extra))
    assert called == []


def test_plant_command_line_switches():
    from open_duck_playground_amd import track
    a = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0"])
    assert a.plant is None and a.plant_grid is None and a.randomize is False and a.noise_level is None
    assert a.robust_fall_rate == track.DEFAULT_ROBUST_FALL_RATE == 0.05
    assert track.plants_from_args(a) == []
    assert "noise_config.level" not in track.config_overrides(a)
    a = track.build_parser().parse_args(["--checkpoint", "c.pt", "--command", "0", "0", "0", "--plant", "kp=0.6,delay=2", "--plant", "kp=1.0",
                                         "--plant_grid", "mass=0.9:1.1:2", "--robust_fall_rate", "0.1", "--randomize", "--noise_level", "0"])
    plants = track.plants_from_args(a)
    assert [(p["kp"], p["mass"], p["delay"]) for p in plants] == [(0.6, 1.0, 2), (1.0, 1.0, "random"), (1.0, 0.9, "random"), (1.0, 1.1, "random")]
    assert a.randomize is True and a.robust_fall_rate == 0.1 and track.config_overrides(a)["noise_config.level"] == 0.0
    text = track.build_parser().format_help()
    assert "inertias are NOT rescaled" in " ".join(text.split())


def _cells(spec, fall_rates):
    from open_duck_playground_amd import track
    plants = track.parse_plant_grid(spec) if ":" in spec else [track.parse_plant(s) for s in spec.split(";")]
    assert len(plants) == len(fall_rates)
    return [dict(plant=p, fall_rate=f, rms_error_vx=0.1 * i, rms_error_vy=0.0, rms_error_wz=0.0, mean_episode_reward=10.0 - i)
            for i, (p, f) in enumerate(zip(plants, fall_rates))]


def test_survived_range_on_hand_made_rows():
    from open_duck_playground_amd.track import survived_range
    v = [0.6, 0.8, 1.0, 1.2, 1.4]
    assert survived_range(v, [0.5, 0.0, 0.0, 0.05, 0.3], 0.05) == [0.8, 1.2]            # at most the threshold counts as survived
    assert survived_range(v, [0.5, 0.0, 0.0, 0.05, 0.3], 0.04) == [0.8, 1.0]
    assert survived_range(v, [0.0] * 5, 0.05) == [0.6, 1.4]
    # a gap in the middle ends the run there, whatever passes beyond it
    assert survived_range(v, [0.0, 0.2, 0.0, 0.0, 0.0], 0.05) == [1.0, 1.4]
    assert survived_range(v, [0.0, 0.0, 0.0, 0.2, 0.0], 0.05) == [0.6, 1.0]
    # nominal not in the grid: the run starts at the nearest value, the smaller of two equally near
    assert survived_range([0.7, 0.9, 1.1, 1.3], [0.0, 0.0, 0.2, 0.0], 0.05) == [0.7, 0.9]
    assert survived_range([0.7, 0.9, 1.1, 1.3], [0.0, 0.2, 0.0, 0.0], 0.05) is None      # 0.9 is "nominal" here, and it fails
    assert survived_range([1.2, 1.4], [0.0, 0.0], 0.05) == [1.2, 1.4]
    assert survived_range([1.2, 1.4], [0.3, 0.0], 0.05) is None
    # all cells failing; no cells
    assert survived_range(v, [0.2] * 5, 0.05) is None
    assert survived_range([], [], 0.05) is None
    # the order given does not matter
    assert survived_range([1.4, 0.6, 1.0, 1.2, 0.8], [0.3, 0.5, 0.0, 0.05, 0.0], 0.05) == [0.8, 1.2]
    # the delay line: nominal is the smallest fixed delay
    assert survived_range([0, 1, 2], [0.0, 0.0, 0.4], 0.05, nominal=0) == [0.0, 1.0]
    assert survived_range([0, 1, 2], [0.1, 0.0, 0.0], 0.05, nominal=0) is None


def test_robustness_lines_hold_the_other_axes_nearest_nominal():
    from open_duck_playground_amd import track
    # kp 0.5 | 1.0 x delay 0 | 1 | 2: the kp line runs at delay 0 (no `random` in the grid: the smallest), the delay line at kp 1.0
    cells = _cells("kp=0.5:1.0:2,delay=0:2:3", [0.5, 0.6, 0.9, 0.0, 0.02, 0.3])
    r = track.reduce_robustness(cells, 0.05)
    assert set(r) == {"robust_fall_rate", "kp", "delay", "survived_range"} and r["robust_fall_rate"] == 0.05
    assert [(p["value"], p["fall_rate"]) for p in r["kp"]] == [(0.5, 0.5), (1.0, 0.0)]
    assert [(p["value"], p["fall_rate"]) for p in r["delay"]] == [(0, 0.0), (1, 0.02), (2, 0.3)]
    assert all(tuple(p) == track.ROBUSTNESS_POINT_KEYS for p in r["kp"] + r["delay"])
    assert r["delay"][1]["mean_episode_reward"] == 10.0 - 4 and r["delay"][1]["rms_error_vx"] == pytest.approx(0.4)
    assert r["survived_range"] == {"kp": [1.0, 1.0], "delay": [0.0, 1.0]}
    # --plant lists: `random` is the delay's nominal when present, listed first, and no point of the survived line
    cells = _cells("delay=2;delay=random;delay=0;kp=0.7,delay=0", [0.4, 0.0, 0.0, 0.9])
    r = track.reduce_robustness(cells, 0.05)
    assert [p["value"] for p in r["delay"]] == ["random", 0, 2]
    assert [p["value"] for p in r["kp"]] == [1.0]          # kp is swept (0.7, 1.0), but no cell pairs 0.7 with the nominal delay
    assert r["survived_range"] == {"kp": [1.0, 1.0], "delay": [0.0, 0.0]}
    # one plant: nothing is swept
    r = track.reduce_robustness(_cells("kp=0.8", [0.0]), 0.05)
    assert r == {"robust_fall_rate": 0.05, "survived_range": {}}
    # every cell failing
    r = track.reduce_robustness(_cells("mass=0.8:1.2:3", [0.5, 0.5, 0.5]), 0.05)
    assert r["survived_range"] == {"mass": None} and len(r["mass"]) == 3
