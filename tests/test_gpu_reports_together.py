"""The reports of track.Tracker do not see each other, and a replayed graph launches all of them: every accumulator of a Tracker that carries
all reports equals, bit for bit, the one of a Tracker that carries that report alone, captured and eager.  The duck on flat terrain, a
random-weight policy, 6 envs -- the second wave of the 16-lane kernels is half empty, and their rows e >= nenv exist -- and 24 steps."""
import numpy as np
import pytest

import report_cases as RC

pytestmark = pytest.mark.gpu

N, T, SEED = 6, 24, 5
PUSH_AT = 2
# One world-frame kick per env at step PUSH_AT, after test_gpu_pushes' (0.2 .. 3 m/s there, over 300 steps), from none to ones that end the
# episode within the 21 steps left.  Picked on the GPU: envs 1, 3, 4, 5 fell (after 24, 21, 12, 12 steps), envs 0 and 2 did not.
KICKS = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, -1.0], [4.0, 0.0], [0.0, 6.0], [-6.0, -6.0]], np.float32)
ACCS = ("acc", "push_acc", "gait_acc", "posture_acc", "imitation_acc", "response_acc", "fall_acc")


def _accumulators(ckpt, use_graph=True, **reports):
    """a Tracker with `reports` (Tracker's own switches) over N fresh envs, reset and stepped T times: its accumulators as int32 arrays"""
    import torch
    from open_duck_playground_amd import track
    args = track.build_parser().parse_args(["--checkpoint", ckpt, "--command", "0", "0", "0"])      # the default episode length: no truncation in T steps
    env = track.make_env(args, N, 0)
    net = track.load_networks(ckpt, env, torch.device("cuda", 0))
    commands = [track.command_row([0, 0, 0]), track.command_row([0.1, 0, 0])]
    env.set_commands(torch.from_numpy(track.command_blocks(commands, N // 2)).to("cuda"))
    tr = track.Tracker(env, net, use_graph=use_graph, **reports)
    with torch.no_grad():
        tr.reset(SEED)
        for _ in range(T):
            tr.step()
        out = {name: getattr(tr, name).cpu().numpy().view(np.int32) for name in ACCS if getattr(tr, name) is not None}
    assert (tr.graph is not None) == use_graph
    env.set_commands(None)
    env.set_pushes(None)
    env.batch.close()
    return out


def _same(a, b, names):
    for name in names:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), name


def test_pushes_gait_posture_imitation_and_falls_together_are_each_alone(tmp_path):
    """The kicks are part of the episode -- a Tracker without them steps another trajectory -- so every Tracker binds them: `alone` is the push
    report by itself, and each other report next to it alone."""
    import torch
    from open_duck_playground_amd import engine
    ckpt = RC.fresh_checkpoint(tmp_path)
    pushes = dict(kicks=torch.from_numpy(KICKS), push_at=PUSH_AT)
    each = dict(gait=dict(gait=True), posture=dict(posture=True, posture_tolerance=0.05), imitation=dict(imitation=True),
                fall=dict(falls=dict(ring=8, tilt_tol=0.3)))
    everything = {k: v for switches in each.values() for k, v in switches.items()}
    together = _accumulators(ckpt, **pushes, **everything)
    assert sorted(together) == sorted(set(ACCS) - {"response_acc"})
    ended = together["acc"].view(np.float32)[:, engine.TRACK_ENDED] != 0
    print("first episodes ended:", ended.astype(int), "pushed:", together["push_acc"].view(np.float32)[:, engine.PUSH_PUSHED])
    assert 0 < ended.sum() < N                                 # some episodes end inside the run (their rows freeze), some run on
    assert together["fall_acc"].view(np.float32)[:, engine.FALL_FELL].sum() > 0
    _same(together, _accumulators(ckpt, **pushes), ("acc", "push_acc"))
    for name, switches in each.items():
        _same(together, _accumulators(ckpt, **pushes, **switches), ("acc", "push_acc", name + "_acc"))
    eager = _accumulators(ckpt, use_graph=False, **pushes, **everything)
    _same(together, eager, sorted(together))


def test_schedule_response_and_falls_together_are_each_alone(tmp_path):
    """Schedules exclude pushes.  The schedule is part of the episode, so every Tracker carries it (and with it the response report): the
    response report is compared alone; falls next to it IS the together run, so here falls is held only captured against eager."""
    from open_duck_playground_amd import track
    ckpt = RC.fresh_checkpoint(tmp_path)
    schedules = track.then_schedules([track.command_row([0, 0, 0]), track.command_row([0.1, 0, 0])], [track.command_row([0, 0, 1.0])], 8)
    schedule = dict(table=track.schedule_table(schedules), map=track.schedule_blocks(len(schedules), N // 2), tolerance=(0.05, 0.2), tail_after=4)
    falls = dict(ring=8, tilt_tol=0.3)
    together = _accumulators(ckpt, schedule=schedule, falls=falls)
    assert sorted(together) == ["acc", "fall_acc", "response_acc"]
    _same(together, _accumulators(ckpt, schedule=schedule), ("acc", "response_acc"))
    _same(together, _accumulators(ckpt, use_graph=False, schedule=schedule, falls=falls), sorted(together))
