"""CPU checks of command schedules and the step-response report of `track --sequence` / `--then`: the C-ABI exports and the slot names,
the schedule parser, table and env map (padding, the `--then` cross product, the block order, every refusal by its message), the report's
reduction of a hand-written response accumulator (a segment nobody entered, one nobody responded to, a fall, a segment without tail
samples, an axis whose command did not change), the command-line flags with their refusals next to pushes and `--posture`, and the tensor
checks of `Batch.command_schedule_apply` / `Batch.response_accumulate`."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLOTS = dict(ENTERED=0, SAMPLES=1, FELL=2, STEPS_TO_FALL=3, FIRST_IN=4, LAST_OFF=5, PEAK_LIN_ERR=6, PEAK_ANG_ERR=7, SUM=8, SQERR=11, OVERSHOOT=14,
             TAIL_SAMPLES=17, TAIL_SUM=18)
TRIPLES = ("SUM", "SQERR", "OVERSHOOT", "TAIL_SUM")
STRIDE, MAX_SEGMENTS, NACC = 24, 8, 192


def test_libodk_exports_the_schedule_and_response_kernels_and_the_header_names_their_slots():
    from open_duck_playground_amd import engine, track
    engine.build_library()
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ("odk_command_schedule_apply", "odk_response_accumulate"):
        assert hasattr(lib, name), name
        assert name in engine.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    header = engine.header_constants()
    assert header["SCHED_MAX_SEGMENTS"] == MAX_SEGMENTS and header["SCHED_SEG_FLOATS"] == 8
    assert header["RESP_STRIDE"] == STRIDE and header["RESP_NACC"] == NACC
    assert re.search(r"#define ODK_RESP_NACC \(ODK_SCHED_MAX_SEGMENTS \* ODK_RESP_STRIDE\)", text)
    assert re.search(r"#define ODK_SCHED_NEVER [0-9.e+]+f\b", text) and header["SCHED_NEVER"] == engine.SCHED_NEVER == 1.0e9
    assert np.float32(engine.SCHED_NEVER) > 2.0 ** 24          # above every step count a float32 counter can reach
    assert engine.SCHED_MAX_SEGMENTS == track.SCHED_MAX_SEGMENTS == MAX_SEGMENTS and engine.SCHED_SEG_FLOATS == 8
    assert engine.RESP_STRIDE == track.RESP_STRIDE == STRIDE and engine.RESP_NACC == track.RESP_NACC == NACC
    names = {k[5:]: v for k, v in header.items() if k.startswith("RESP_") and k not in ("RESP_STRIDE", "RESP_NACC")}
    assert names == SLOTS                # the header names these slots and no others
    for name, slot in SLOTS.items():
        assert getattr(engine, "RESP_" + name) == slot, name
    # no two slots overlap, and a block fits its stride
    used = sorted(s + i for name, s in SLOTS.items() for i in range(3 if name in TRIPLES else 1))
    assert len(set(used)) == len(used) and used[-1] < STRIDE


def test_parse_sequence_pads_commands_and_keeps_the_order():
    from open_duck_playground_amd import track
    s = track.parse_sequence("0: 0 0 0 | 150: 0.15 0 0 | 400: 0 0 0.5 0.1|700:0 0 0 0 0 0 -0.25")
    assert [seg["start_step"] for seg in s] == [0, 150, 400, 700]
    assert s[1]["command"] == [0.15, 0, 0, 0, 0, 0, 0] and s[2]["command"] == [0, 0, 0.5, 0.1, 0, 0, 0] and s[3]["command"][6] == -0.25
    assert all(len(seg["command"]) == 7 for seg in s)
    track.check_schedule(s, 1000)
    assert track.parse_sequence("0: 0.1 0 0") == [dict(start_step=0, command=[0.1, 0, 0, 0, 0, 0, 0])]
    for bad, why in (("0 0 0 0", "is not `start_step"), ("0: 0 0", "3 to 7 numbers"), ("0: 0 0 0 | x: 0 0 0", "is not a number"),
                     ("0: 0 0 0 | 1.5: 0 0 0", "whole number"), ("0: 0 0 0 |", "is not `start_step"), ("0: 0 0 0 0 0 0 0 0", "3 to 7 numbers")):
        with pytest.raises(ValueError, match=why):
            track.parse_sequence(bad)


def test_schedule_table_pads_with_never_and_blocks_map_envs():
    from open_duck_playground_amd import engine, track
    a = track.parse_sequence("0: 0.1 0 0")
    b = track.parse_sequence("0: 0 0 0 | 20: 0.1 0.05 0 | 40: 0 0 0.5 0.1 0.2 0.3 0.4")
    tab = track.schedule_table([a, b])
    assert tab.dtype == np.float32 and tab.shape == (2, 3, 8)
    np.testing.assert_array_equal(tab[0, 0], np.float32([0, 0.1, 0, 0, 0, 0, 0, 0]))
    np.testing.assert_array_equal(tab[0, 1:, 0], np.float32(engine.SCHED_NEVER))
    np.testing.assert_array_equal(tab[0, 1:, 1:], 0.0)
    np.testing.assert_array_equal(tab[1, :, 0], [0, 20, 40])
    np.testing.assert_array_equal(tab[1, 2, 1:], np.float32([0, 0, 0.5, 0.1, 0.2, 0.3, 0.4]))
    full = [dict(start_step=10 * k, command=[0.01 * k] * 7) for k in range(8)]
    assert track.schedule_table([full]).shape == (1, 8, 8)
    m = track.schedule_blocks(3, 4)
    assert m.dtype == np.int32
    np.testing.assert_array_equal(m, [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2])
    with pytest.raises(ValueError, match="no schedule"):
        track.schedule_table([])


def test_then_crosses_every_command_with_every_target_from_commands_outermost():
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt"]
    args = track.build_parser().parse_args(base + ["--command", "0.1", "0", "0", "--grid", "wz=-1:1:2", "--then", "0", "0", "0", "--then", "0", "0.05", "0",
                                                   "0.2", "--switch_at", "30", "--episode_length", "60"])
    s = track.schedules_from_args(args)
    froms = [[0.1, 0, 0, 0, 0, 0, 0], [0, 0, -1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0]]
    thens = [[0, 0, 0, 0, 0, 0, 0], [0, 0.05, 0, 0.2, 0, 0, 0]]
    assert len(s) == 6
    for c, f in enumerate(froms):
        for k, t in enumerate(thens):
            assert s[c * 2 + k] == [dict(start_step=0, command=f), dict(start_step=30, command=t)], (c, k)
    assert s == track.then_schedules(froms, thens, 30)
    # the issue's own command line: nine from-commands, one target, the default switch
    args = track.build_parser().parse_args(base + ["--grid", "vx=-0.15:0.15:3,wz=-1:1:3", "--then", "0", "0", "0"])
    s = track.schedules_from_args(args)
    assert len(s) == 9 and all(x[1] == dict(start_step=300, command=[0.0] * 7) for x in s) and args.switch_at == track.DEFAULT_SWITCH_AT == 300
    assert [x[0]["command"][:3] for x in s][:4] == [[-0.15, 0, -1], [-0.15, 0, 0], [-0.15, 0, 1], [0, 0, -1]]
    # no schedule flag: None, and nothing is asked of the other flags
    assert track.schedules_from_args(track.build_parser().parse_args(base + ["--command", "0", "0", "0", "--posture", "--push", "1", "0"])) is None


REFUSALS = [
    (["--sequence", "5: 0 0 0 | 20: 0.1 0 0"], "first segment of a schedule starts at step 0.*not at 5"),
    (["--sequence", "0: 0 0 0 | 20: 0.1 0 0 | 20: 0 0 0"], "start steps of a schedule increase: segment 2 starts at 20, segment 1 at 20"),
    (["--sequence", "0: 0 0 0 | 30: 0.1 0 0 | 10: 0 0 0"], "start steps of a schedule increase"),
    (["--sequence", " | ".join(f"{10 * k}: 0 0 0" for k in range(9))], "a schedule has 1 to 8 segments, this one has 9"),
    (["--sequence", "0: 0 0 0 | 100: 0.1 0 0"], "segment 1 starts at step 100, at or beyond the episode's 100 steps"),
    (["--sequence", "0: 0 0 0 | 250: 0.1 0 0"], "at or beyond the episode's 100 steps"),
    (["--sequence", "0: 0 0 0 | 20: 0.1 nan 0"], "command of segment 1 is not 7 finite values"),
    (["--sequence", "0: inf 0 0"], "command of segment 0 is not 7 finite values"),
    (["--sequence", "0: 1e39 0 0"], "not 7 finite values"),                                   # finite as a double, not as the float32 the table holds
    (["--sequence", "0: 0 0 0", "--sequence", "0: 0 0 0 | 0: 0.1 0 0"], "schedule 1: .*increase"),
    (["--then", "0", "0", "0"], "--then switches away from a command: give the from-commands with --command or --grid"),
    (["--sequence", "0: 0 0 0", "--command", "0", "0", "0"], "--sequence is a whole schedule of its own.*--command, --grid or --then"),
    (["--sequence", "0: 0 0 0", "--grid", "vx=0:0.1:2"], "--sequence is a whole schedule of its own"),
    (["--sequence", "0: 0 0 0", "--then", "0", "0", "0"], "--sequence is a whole schedule of its own"),
    (["--command", "0", "0", "0", "--then", "0.1", "0", "0", "--switch_at", "100"], "segment 1 starts at step 100, at or beyond"),
    (["--command", "0", "0", "0", "--then", "0.1", "0", "0", "--switch_at", "0"], "start steps of a schedule increase"),
    (["--command", "0", "0", "0", "--then", "0.1", "0"], "3 to 7 numbers"),
    (["--sequence", "0: 0 0 0", "--push", "1", "0"], "do not combine with --push / --push_grid.*one command per episode"),
    (["--command", "0", "0", "0", "--then", "0.1", "0", "0", "--switch_at", "10", "--push_grid", "magnitude=0:1:2"], "do not combine with --push / --push_grid"),
    (["--sequence", "0: 0 0 0", "--posture"], "do not combine with --posture.*one command per episode"),
    (["--sequence", "0: 0 0 0", "--response_tolerance", "-0.1", "0.2"], "--response_tolerance LIN ANG: two finite errors >= 0"),
    (["--sequence", "0: 0 0 0", "--response_tolerance", "0.1", "nan"], "--response_tolerance LIN ANG"),
    (["--sequence", "0: 0 0 0", "--response_tail_after", "-1"], "--response_tail_after is a number of steps: >= 0"),
    (["--sequence", "0 0 0"], "is not `start_step: vx vy wz"),
]


@pytest.mark.parametrize("flags,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_say_what_is_wrong(flags, message):
    """Each as `run` raises it: SystemExit before any batch is made (no GPU here, so getting that far would be another error)."""
    from open_duck_playground_amd import track
    args = track.build_parser().parse_args(["--checkpoint", "c.pt", "--episode_length", "100"] + flags)
    with pytest.raises(SystemExit, match=message):
        track.schedules_from_args(args)
    with pytest.raises(SystemExit, match=message):
        track.run(args)


def test_response_command_line_flags():
    from open_duck_playground_amd import track
    base = ["--checkpoint", "c.pt"]
    args = track.build_parser().parse_args(base + ["--command", "0", "0", "0"])
    assert args.sequence is None and args.then is None and args.switch_at == 300
    assert tuple(args.response_tolerance) == track.DEFAULT_PUSH_TOLERANCE and args.response_tail_after == track.DEFAULT_RESPONSE_TAIL_AFTER == 100
    args = track.build_parser().parse_args(base + ["--sequence", "0: 0 0 0 | 150: 0.15 0 0 | 400: 0 0 0.5 | 700: 0 0 0", "--sequence", "0: 0.1 0 0",
                                                   "--response_tolerance", "0.02", "0.1", "--response_tail_after", "50"])
    assert len(args.sequence) == 2 and args.response_tolerance == [0.02, 0.1] and args.response_tail_after == 50
    s = track.schedules_from_args(args)
    assert [len(x) for x in s] == [4, 1] and track.response_tolerance(args) == (0.02, 0.1)
    # --gait and --imitation_report combine with schedules
    args = track.build_parser().parse_args(base + ["--sequence", "0: 0.1 0 0", "--gait", "--imitation_report"])
    assert len(track.schedules_from_args(args)) == 1
    help_text = " ".join(track.build_parser().format_help().split())
    for word in ("--sequence", "--then", "--switch_at", "--response_tolerance", "--response_tail_after", "from-commands outermost", "steady-state error"):
        assert word in help_text, word


def _env(**segments):
    """one accumulator row: per segment index a dict of slots by name (three values for SUM, SQERR, OVERSHOOT, TAIL_SUM)"""
    r = np.zeros(NACC, np.float32)
    for k, slots in segments.items():
        for name, v in slots.items():
            n = 3 if name in TRIPLES else 1
            r[int(k[1:]) * STRIDE + SLOTS[name]:int(k[1:]) * STRIDE + SLOTS[name] + n] = np.float32(v)
    return r


def test_response_report_reduction():
    """One schedule of four segments, three envs, dt 0.02, every figure at its closed form.  Segment 0 (command 0 0 0, 20 steps): everybody
    inside at once, vx and wz unchanged from rest.  Segment 1 (vx 0.1, vy -0.05: vy changed downwards, wz did not change): env 0 responds
    after 5 samples and settles after 8, env 1 responds after 9 and is outside again at its last sample (not settled), env 2 falls at its
    4th step without ever responding.  Segment 2: only env 0 and env 1 enter; nobody responds; fewer samples than the tail needs.  Segment 3:
    nobody entered."""
    from open_duck_playground_amd import track
    dt = 0.02
    sched = track.parse_sequence("0: 0 0 0 | 20: 0.1 -0.05 0 | 60: 0 0 0.5 | 90: 0 0 0")
    s0 = dict(ENTERED=1, SAMPLES=20, FIRST_IN=1, LAST_OFF=0, PEAK_LIN_ERR=0.01, PEAK_ANG_ERR=0.05, SUM=(0.2, 0, -0.4), SQERR=(0.002, 0, 0.008),
              TAIL_SAMPLES=10, TAIL_SUM=(0.1, 0, -0.2))
    acc = np.stack([
        _env(s0=s0,
             s1=dict(ENTERED=1, SAMPLES=40, FIRST_IN=5, LAST_OFF=8, PEAK_LIN_ERR=0.04, PEAK_ANG_ERR=0.1, SUM=(3.6, -1.8, 0.4), SQERR=(0.04, 0.01, 0.16),
                     OVERSHOOT=(0.02, 0.01, 0), TAIL_SAMPLES=30, TAIL_SUM=(3.0, -1.5, 0.3)),
             s2=dict(ENTERED=1, SAMPLES=8, LAST_OFF=8, SUM=(0.4, 0, 1.6), SQERR=(0.02, 0, 0.72), OVERSHOOT=(0, 0, 0))),
        _env(s0=s0,
             s1=dict(ENTERED=1, SAMPLES=40, FIRST_IN=9, LAST_OFF=40, PEAK_LIN_ERR=0.08, PEAK_ANG_ERR=0.3, SUM=(4.4, -2.2, 0.4), SQERR=(0.08, 0.03, 0.16),
                     OVERSHOOT=(0.04, 0.03, 0), TAIL_SAMPLES=30, TAIL_SUM=(3.3, -1.8, 0.3)),
             s2=dict(ENTERED=1, SAMPLES=8, LAST_OFF=8, SUM=(0.4, 0, 2.4), SQERR=(0.02, 0, 0.32), OVERSHOOT=(0, 0, 0.125))),
        _env(s0=s0,
             s1=dict(ENTERED=1, SAMPLES=3, FELL=1, STEPS_TO_FALL=4, LAST_OFF=3, SUM=(0.0, 0.0, 0.9), SQERR=(0.03, 0.0075, 0.27), OVERSHOOT=(0, 0, 0))),
    ])
    (segs,) = track.reduce_response(acc, [sched], 3, dt)
    assert len(segs) == 4 and json.loads(json.dumps(segs)) == segs
    assert all(tuple(g) == track.SEGMENT_KEYS for g in segs)
    ap = pytest.approx
    g = segs[0]
    assert g["start_step"] == 0 and g["command"] == [0.0] * 7 and g["envs_entered"] == 3 and g["velocity_samples"] == 60
    assert g["mean_vx"] == ap(0.6 / 60) and g["mean_wz"] == ap(-1.2 / 60) and g["rms_error_wz"] == ap(np.sqrt(0.024 / 60))
    assert g["fall_rate"] == 0.0 and g["mean_steps_to_fall"] is None
    assert g["responded_fraction"] == 1.0 and g["response_time_s"] == ap(1 * dt) and g["settled_fraction"] == 1.0 and g["settle_time_s"] == 0.0
    assert g["peak_lin_error"] == ap(0.01) and g["peak_ang_error"] == ap(0.05)
    assert g["overshoot_vx"] == g["overshoot_vy"] == g["overshoot_wz"] == 0.0      # nothing changed from rest: every axis keeps 0
    assert g["steady_state_error_vx"] == ap(0.3 / 30) and g["steady_state_error_wz"] == ap(-0.6 / 30)

    g = segs[1]
    assert g["start_step"] == 20 and g["command"][:3] == [0.1, -0.05, 0.0] and g["envs_entered"] == 3 and g["velocity_samples"] == 83
    assert g["mean_vx"] == ap(8.0 / 83) and g["mean_vy"] == ap(-4.0 / 83) and g["rms_error_vy"] == ap(np.sqrt(0.0475 / 83))
    assert g["fall_rate"] == ap(1 / 3) and g["mean_steps_to_fall"] == 4.0
    assert g["responded_fraction"] == ap(2 / 3) and g["response_time_s"] == ap((5 + 9) / 2 * dt)
    assert g["settled_fraction"] == ap(1 / 3) and g["settle_time_s"] == ap(8 * dt)      # env 1 and the env that fell were outside at their last sample
    assert g["peak_lin_error"] == ap(0.08) and g["peak_ang_error"] == ap(0.3)           # over the envs that responded
    assert g["overshoot_vx"] == ap(0.06 / 3) and g["overshoot_vy"] == ap(0.04 / 3)
    assert g["overshoot_wz"] == 0.0                                                     # the axis whose command did not change
    assert g["steady_state_error_vx"] == ap(6.3 / 60 - 0.1) and g["steady_state_error_vy"] == ap(-3.3 / 60 + 0.05)
    assert g["steady_state_error_wz"] == ap(0.6 / 60)

    g = segs[2]      # nobody responded, no tail samples
    assert g["envs_entered"] == 2 and g["velocity_samples"] == 16 and g["fall_rate"] == 0.0
    assert g["responded_fraction"] == 0.0 and g["response_time_s"] is None and g["peak_lin_error"] is None and g["peak_ang_error"] is None
    assert g["settled_fraction"] == 0.0 and g["settle_time_s"] is None
    assert g["mean_wz"] == ap(4.0 / 16) and g["overshoot_wz"] == ap(0.125 / 2)
    assert g["steady_state_error_vx"] is None and g["steady_state_error_vy"] is None and g["steady_state_error_wz"] is None

    g = segs[3]      # nobody entered: the segment as given, counts of 0, nothing to average
    assert g["start_step"] == 90 and g["command"] == [0.0] * 7 and g["envs_entered"] == 0 and g["velocity_samples"] == 0
    assert all(g[k] is None for k in track.SEGMENT_KEYS[4:])

    # two schedules of different lengths: blocks in schedule order, a shorter schedule reports its own segments only
    short = track.parse_sequence("0: 0.1 0 0")
    both = track.reduce_response(np.concatenate([acc, acc[:3]]), [sched, short], 3, dt)
    assert [len(x) for x in both] == [4, 1] and both[0] == segs and both[1][0]["envs_entered"] == 3 and both[1][0]["command"][0] == 0.1


def test_the_batch_methods_reject_bad_tensors(monkeypatch):
    """The tensor checks run before the library is touched, so a stand-in batch (no GPU) reaches them through the real methods."""
    import torch
    from open_duck_playground_amd import engine
    n = 8
    stub = types.SimpleNamespace(nenv=n, device=0, model=types.SimpleNamespace(nu=14))
    R, T = engine.RESP_NACC, engine.TRACK_NACC
    sched, smap, tacc, acc = torch.zeros(2, 3, 8), torch.zeros(n, dtype=torch.int32), torch.zeros(n, T), torch.zeros(n, R)
    bad_sched = [
        (np.zeros((2, 3, 8), np.float32), "sched: expected a torch tensor"),
        (torch.zeros(2, 3, 7), "sched: shape"),
        (torch.zeros(2, 9, 8), "sched: shape"),
        (torch.zeros(0, 3, 8), "sched: shape"),
        (torch.zeros(2, 0, 8), "sched: shape"),
        (torch.zeros(6, 8), "sched: shape"),
        (torch.zeros(2, 3, 8, dtype=torch.float64), "sched: dtype"),
        (torch.zeros(2, 8, 3).transpose(1, 2), "sched: the tensor must be contiguous"),
        (sched, "sched: the tensor must live on cuda:0"),            # a host tensor: the kernel reads device memory
    ]
    for t, what in bad_sched:
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.command_schedule_apply(stub, t, smap, tacc)
        assert "command_schedule_apply" in str(ei.value)
    # the accumulator of the response launch
    for t, what in ((np.zeros((n, R), np.float32), "torch tensor"), (torch.zeros(n, R - 1), "shape"), (torch.zeros(n + 1, R), "shape"),
                    (torch.zeros(n, R, dtype=torch.float64), "dtype"), (torch.zeros(R, n).t(), "contiguous"), (acc, "cuda:0")):
        with pytest.raises(engine.OdkError, match=what) as ei:
            engine.Batch.response_accumulate(stub, t, tacc, sched, smap, 0.05, 0.2, 10)
        assert "response_accumulate: acc" in str(ei.value)
    # the map's own checks come after the table's, so they need a table that passes: only a device tensor does, and there is none here;
    # check_schedule is the function both methods call
    dev = types.SimpleNamespace(type="cuda", index=0)

    class OnDevice:
        """a tensor's face as check_schedule reads it, claiming cuda:0"""
        def __init__(self, t):
            self.t = t
        shape = property(lambda self: self.t.shape)
        dtype = property(lambda self: self.t.dtype)
        device = dev
        dim = lambda self: self.t.dim()
        is_contiguous = lambda self: self.t.is_contiguous()

    real = torch.is_tensor
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, OnDevice) or real(x))
    assert engine.check_schedule("x", OnDevice(sched), OnDevice(smap), n, 0) == (2, 3)
    for m, what in ((torch.zeros(n + 1, dtype=torch.int32), "sched_of_env: shape"), (torch.zeros(n, 1, dtype=torch.int32), "sched_of_env: shape"),
                    (torch.zeros(n, dtype=torch.int64), "sched_of_env: dtype"), (torch.zeros(n, dtype=torch.float32), "sched_of_env: dtype"),
                    (torch.zeros(2 * n, dtype=torch.int32)[::2], "sched_of_env: the tensor must be contiguous")):
        with pytest.raises(engine.OdkError, match=what):
            engine.check_schedule("x", OnDevice(sched), OnDevice(m), n, 0)
    with pytest.raises(engine.OdkError, match="sched_of_env: the tensor must live on cuda:0"):
        engine.check_schedule("x", OnDevice(sched), smap, n, 0)
    with pytest.raises(engine.OdkError, match="sched_of_env: expected a torch tensor"):
        engine.check_schedule("x", OnDevice(sched), [0] * n, n, 0)
