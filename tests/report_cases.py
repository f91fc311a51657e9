"""What the GPU tests of the `track` reports share: the robots and a fresh checkpoint, `track.run` with its Tracker caught, the synthetic
first episodes, the guarded accumulator driven step by step, and the two judgements -- a row that is no sample keeps its bits; float32
running sums lie within their bound of a float64 restatement.  A plain module without fixtures; torch and the package are imported where
they are used, so it imports on a machine without a GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "assets")


class _Header:
    """include/odk.h's constants as engine carries them (engine.GAIT_SAMPLES, ...), looked up at first use: a test file aliases this at its
    top (`G = RC.HEADER`) and still imports the package only inside its tests."""
    def __getattr__(self, name):
        from open_duck_playground_amd import engine
        return getattr(engine, name)


HEADER = _Header()


def robot_sizes(robot):
    """(nobs, npriv, nu, nq, key_ctrl [nu] float32) of a Joystick batch of `robot` (as `robot_env` names it), from its model alone: no GPU."""
    from open_duck_playground_amd import constants, engine
    from open_duck_playground_amd.model import Model
    model = Model.from_xml(os.path.join(ASSETS, robot)) if robot.endswith(".xml") else constants.task_to_model("flat_terrain" if robot == "duck" else robot)
    return (*engine.model_obs_sizes(model), int(model.nu), int(model.nq), home_pose(model, int(model.nu)))


def home_pose(model, nu):
    return np.asarray(model.a["key_ctrl"], np.float64).reshape(-1)[:nu].astype(np.float32)


def robot_env(robot, n, **kw):
    """A Joystick env of n envs: "duck" or a task name is the shipped task, an .xml name the robot under tests/assets."""
    from open_duck_playground_amd import joystick
    if robot.endswith(".xml"):
        return joystick.Joystick(xml_path=os.path.join(ASSETS, robot), num_envs=n, **kw)
    return joystick.Joystick(task="flat_terrain" if robot == "duck" else robot, num_envs=n, **kw)


def fresh_checkpoint(tmp_path, sizes=(101, 212, 14), name="fresh.pt"):
    """A randomly initialised policy (seed 0) of the duck's Joystick sizes, or of `sizes`, saved under tmp_path."""
    import torch
    from open_duck_playground_amd.ppo.networks import PPONetworks
    from open_duck_playground_amd.ppo.train import save_checkpoint
    torch.manual_seed(0)
    ckpt = str(tmp_path / name)
    save_checkpoint(ckpt, PPONetworks(*sizes))
    return ckpt


def step_outputs(tracker, before=None):
    """`run_track`'s default recording: the privileged rows and the done and truncation flags the step left."""
    b = tracker.env.batch
    return b.priv.cpu().numpy(), b.done.cpu().numpy(), b.truncation.cpu().numpy()


def run_track_with_ended(track, monkeypatch, argv, eager=False):
    """`run_track` recording (priv, done, ended) per step: ended is the tracking accumulator's ENDED column as the step's launches saw it,
    read before this step's tracking launch sets it."""
    return run_track(track, monkeypatch, argv, eager, before_step=lambda tr: tr.acc[:, HEADER.TRACK_ENDED].cpu().numpy(),
                     after_step=lambda tr, ended: step_outputs(tr)[:2] + (ended,))


def run_track(track, monkeypatch, argv, eager=False, before_step=None, after_step=step_outputs, after_reset=None):
    """track.run with its Tracker caught.  eager: no graph, and a recording -- what `after_reset(tracker)` returns after the reset and what
    `after_step(tracker, before)` returns after every step, `before` being what `before_step(tracker)` returned ahead of it (None without
    one).  Returns (report, tracker, recording)."""
    real = track.Tracker
    caught, hist = [], []

    class Caught(real):
        def __init__(self, *a, **k):
            if eager:
                k["use_graph"] = False
            super().__init__(*a, **k)
            caught.append(self)

        def reset(self, seed):
            super().reset(seed)
            if eager and after_reset is not None:
                hist.append(after_reset(self))

        def step(self):
            before = before_step(self) if eager and before_step is not None else None
            super().step()
            if eager:
                hist.append(after_step(self, before))

    monkeypatch.setattr(track, "Tracker", Caught)
    try:
        rep = track.run(track.build_parser().parse_args(argv))
    finally:
        monkeypatch.setattr(track, "Tracker", real)
    assert len(caught) == 1
    return rep, caught[0], hist


def planar32(x, y):
    """the kernels' hypot: float64 squares (exact for float32 inputs) and root, one rounding to float32"""
    x, y = np.float64(x), np.float64(y)
    return np.float32(np.sqrt(x * x + y * y))


def first_episodes(rng, T, n, ends, truncated):
    """Synthetic first episodes of n envs over T steps: env e ends at step ends[e % len(ends)] (T + 1: never), by truncation where that
    residue is in `truncated`.  One draw from rng, uniform(size=(T, n)): stray done flags after the end, which must not matter; none
    before it.  Returns end_at [n], done and trunc [T, n] float32, and ended [T, n] float32, the tracking accumulator's ENDED column as
    the launch of step t sees it."""
    end_at = np.array([ends[e % len(ends)] for e in range(n)])
    with_trunc = np.array([e % len(ends) in truncated for e in range(n)])
    done = (rng.uniform(size=(T, n)) < 0.1).astype(np.float32)
    for e in range(n):
        done[:min(end_at[e], T), e] = 0.0
        if end_at[e] < T:
            done[end_at[e], e] = 1.0
    trunc = (done * with_trunc[None]).astype(np.float32)
    ended = (np.arange(T)[:, None] > end_at[None]).astype(np.float32)
    return end_at, done, trunc, ended


def drive_rows(b, launch, nacc, priv, done, trunc, ended):
    """T launches over rows written straight into batch b's outputs -- no odk_step: per step priv / done / trunc [t] go into b.priv, b.done
    and b.truncation, ended[t] into the tracking accumulator's ENDED column, as odk_tracking_accumulate would have left it, and
    `launch(acc, tacc)` runs.  The accumulator is the first n rows of one three rows longer and filled with 7.0: the last wave's idle rows
    must not touch those.  Returns (acc [n, nacc], the three rows past it, acc after every step [T, n, nacc])."""
    import torch
    from open_duck_playground_amd import engine
    T, n = done.shape
    guard = torch.full((n + 3, nacc), 7.0, device="cuda")
    acc = guard[:n]
    acc.zero_()
    tacc = torch.zeros(n, engine.TRACK_NACC, device="cuda")
    priv_d, done_d, trunc_d, ended_d = (torch.tensor(x, device="cuda") for x in (priv, done, trunc, ended))
    snaps = []
    for t in range(T):
        b.priv.copy_(priv_d[t]); b.done.copy_(done_d[t]); b.truncation.copy_(trunc_d[t])
        tacc[:, engine.TRACK_ENDED] = ended_d[t]
        launch(acc, tacc)
        snaps.append(acc.clone())
    torch.cuda.synchronize()
    return acc.cpu().numpy(), guard[n:].cpu().numpy(), torch.stack(snaps).cpu().numpy()


def assert_frozen_after_end(snaps, end_at):
    """Rows of envs past their first episode, and of the done step that ends it, keep their bits: what step end_at - 1 left (zeros when
    the episode ended at step 0) is what every later step leaves.  snaps [T, n, nacc] float32; returns the (env, step) pairs compared."""
    snaps = snaps.view(np.int32)
    T, n, nacc = snaps.shape
    checked = 0
    for e in range(n):
        if end_at[e] >= T:
            continue
        frozen = snaps[end_at[e] - 1, e] if end_at[e] > 0 else np.zeros(nacc, np.int32)
        for t in range(end_at[e], T):
            np.testing.assert_array_equal(snaps[t, e], frozen, err_msg=f"env {e} step {t}")
            checked += 1
    return checked


def compare_sums(got, want, samples_col, scales, label):
    """An accumulator `got` [n, nacc] float32 against its float64 restatement `want`.  `scales` maps each column that is a float32 running
    sum to the per-env scale of its bound: want[:, c] itself for a sum of non-negative terms, the sum of the terms' magnitudes for a signed
    one.  Every other column -- counts, peaks, ranges, bookkeeping -- is exact.

    The bound: |got - want| <= (N + 4) * 2^-23 * scale, N the env's sample count (want[:, samples_col]).  The kernel adds N terms one
    after the other in float32, each addition rounding by at most 2^-24 of a partial sum that is no larger than the scale; the terms
    themselves carry at most a few roundings of their own -- a product, a root, a 16-lane tree sum -- under 4 * 2^-23 together.  An env
    without a sample has scale 0 and is exact."""
    got = got.astype(np.float64)
    N = want[:, samples_col]
    bounds = {c: (N + 4) * 2.0 ** -23 * s for c, s in scales.items()}
    worst = max(float(np.max(np.abs(got[:, c] - want[:, c]) / np.maximum(b, 1e-300))) for c, b in bounds.items())
    print(f"{label}: float32 sums, worst error / bound {worst:.3f}")
    for c in range(want.shape[1]):
        if c not in bounds:
            np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=f"{label}: slot {c}")
    for c, b in bounds.items():
        err = np.abs(got[:, c] - want[:, c])
        assert np.all(err <= b), (label, c, float(err.max()), float(b[np.argmax(err - b)]))
