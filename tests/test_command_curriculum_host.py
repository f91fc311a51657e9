"""Host checks of the command curriculum (open_duck_playground_amd/command_curriculum.py): the flags' parser and its refusals, the start
region, the numpy restatements of `odk_curriculum_step` (the draw's distribution) and `odk_curriculum_update` (how levels spread), and the
runner's flags.  No GPU, no libodk.so."""
import json

import numpy as np
import pytest

from open_duck_playground_amd import command_curriculum as CC, engine as E

HEAD = [(-0.34, 1.1), (-0.78, 0.78), (-1.5, 1.5), (-0.5, 0.5)]
NOBS, NPRIV = 101, 212


def spec(grid="vx=-0.15:0.222:8,vy=-0.2:0.2:4,wz=-1.2:1.2:8", start=None, **kw):
    return CC.curriculum_spec(grid, start, **kw)


# ---- the parser
@pytest.mark.parametrize("grid, start, message", [
    ("vz=0:1:2", None, "--command_curriculum: unknown axis 'vz'"),
    ("vx=0:1:2,vx=0:1:3", None, "--command_curriculum: axis 'vx' given twice"),
    ("vx=0:1:17", None, r"--command_curriculum: vx has 17 bins \(1 .. 16 per axis\)"),
    ("vx=0:1:0", None, r"--command_curriculum: vx has 0 bins"),
    ("vx=0:1:16,vy=0:1:16,wz=0:1:16", None, None),                                     # 4096: the most
    ("vx=-0.15:0.222:8", "vx=0.3:0.4", "--curriculum_start: vx=0.3:0.4 lies outside the grid's -0.15 .. 0.222"),
    ("vx=-0.15:0.222:8", "vx=-0.2:0.1", "--curriculum_start: vx=-0.2:0.1 lies outside the grid"),
    ("vx=-0.15:0.222:8", "vx=0.0:0.001", "--curriculum_start: the start is empty: no bin's centre lies inside vx=0:0.001"),
    ("vx=-0.15:0.222:8", "vq=0:1", "--curriculum_start: unknown axis 'vq'"),
    ("vx=0.2:0.1:4", None, "--command_curriculum: vx=0.2:0.1:4 needs finite LO <= HI"),
    ("vx=0.1:0.2", None, "--command_curriculum: 'vx=0.1:0.2' is not AXIS=LO:HI:BINS"),
    ("", None, "--command_curriculum: no axis given"),
])
def test_the_parser_refuses_by_name(grid, start, message):
    if message is None:
        assert CC.curriculum_nbins(CC.curriculum_struct(spec(grid, "vx=0:1,vy=0:1,wz=0:1"), HEAD)) == 4096
        return
    with pytest.raises(ValueError, match=message):
        spec(grid, start)


def test_more_than_4096_bins_cannot_be_written_and_the_struct_check_names_it():
    """16 bins per axis on three axes is 4096: the flag cannot ask for more, so the bound is held where a struct can (engine.curriculum_nbins,
    what both Batch methods call first)."""
    cur = CC.curriculum_struct(spec("vx=0:1:16,vy=0:1:16,wz=0:1:16", "vx=0:1,vy=0:1,wz=0:1"), HEAD)
    cur.n[0] = 17
    with pytest.raises(E.OdkError, match=r"n\[0\] = 17"):
        E.curriculum_nbins(cur)
    cur.n[0] = 16
    assert E.curriculum_nbins(cur) == E.CURR_MAX_BINS == 4096


def test_the_start_region_opens_exactly_the_bins_whose_centre_lies_inside():
    s = spec()      # the default start: the env config's ranges
    assert s["start"] == dict(vx=[-0.15, 0.15], vy=[-0.2, 0.2], wz=[-1.0, 1.0]) and s["grid"]["vy"] == [-0.2, 0.2, 4]
    levels = CC.initial_levels(s).reshape(8, 4, 8)
    edges = CC.bin_edges(s)
    for a, (x, lo, hi) in enumerate((("vx", -0.15, 0.15), ("vy", -0.2, 0.2), ("wz", -1.0, 1.0))):
        e = np.asarray(edges[x])
        assert len(e) == s["grid"][x][2] + 1 and e[0] == s["grid"][x][0] and e[-1] == s["grid"][x][1]
    cx, cw = 0.5 * (np.asarray(edges["vx"])[:-1] + np.asarray(edges["vx"])[1:]), 0.5 * (np.asarray(edges["wz"])[:-1] + np.asarray(edges["wz"])[1:])
    want = ((cx >= -0.15) & (cx <= 0.15))[:, None, None] & np.ones(4, bool)[None, :, None] & ((cw >= -1.0) & (cw <= 1.0))[None, None, :]
    assert np.array_equal(levels == E.CURR_LMAX, want) and np.array_equal(levels == 0, ~want)
    assert want.sum() == 6 * 4 * 6 and not want[6:].any() and not want[:, :, 0].any() and not want[:, :, 7].any()
    # an axis the grid does not name: the env's range, one bin; a start over the whole grid: every bin open (uniform wide sampling)
    s = spec("vx=-0.15:0.222:8,wz=-1.2:1.2:8", "vx=-0.15:0.222,wz=-1.2:1.2")
    assert s["grid"]["vy"] == [-0.2, 0.2, 1] and (CC.initial_levels(s) == E.CURR_LMAX).all()
    assert json.loads(json.dumps(s)) == s


def test_a_grid_wider_than_the_reference_motion_table_is_refused_by_axis():
    table = dict(vx=(-0.2, 0.222), vy=(-0.3, 0.3), wz=(-1.222, 1.222))
    assert spec("vx=-0.15:0.222:8,wz=-1.2:1.2:8", table_ranges=table)["grid"]["vx"] == [-0.15, 0.222, 8]
    with pytest.raises(ValueError, match=r"wz=-1.2:1.3 is wider than the reference-motion table, whose wz range is -1.222 .. 1.222"):
        spec("vx=-0.15:0.222:8,wz=-1.2:1.3:8", table_ranges=table)
    with pytest.warns(UserWarning, match="wz range is -1.222 .. 1.222"):
        s = spec("vx=-0.15:0.222:8,wz=-1.2:1.3:8", table_ranges=table, allow_clipped_reference=True)
    assert s["grid"]["wz"] == [-1.2, 1.3, 8]
    assert spec("wz=-1.2:1.3:8", table_ranges=None)["grid"]["wz"][1] == 1.3      # the imitation reward off: no table to leave


def test_the_shipped_table_holds_the_issues_grid():
    from open_duck_playground_amd.reference_motion import ReferenceMotion
    m = ReferenceMotion.from_npz()
    table = {x: tuple(float(v) for v in getattr(m, k)) for x, k in zip(CC.AXES, CC.TABLE_KEYS)}
    assert table == dict(vx=(-0.148, 0.222), vy=(-0.111, 0.111), wz=(-1.111, 1.222))
    spec("vx=-0.15:0.222:8,vy=-0.2:0.2:4,wz=-1.1:1.222:8", table_ranges=table)      # (vx = -0.15 and vy = +-0.2 are the env's own range: not refused)
    with pytest.raises(ValueError, match="vx=-0.15:0.3 is wider than the reference-motion table, whose vx range is -0.148 .. 0.222"):
        spec("vx=-0.15:0.3:8", table_ranges=table)
    with pytest.raises(ValueError, match="wz=-1.2:1.2 is wider than the reference-motion table, whose wz range is -1.111 .. 1.222"):
        spec("wz=-1.2:1.2:8", table_ranges=table)


def test_settings_and_the_struct():
    s = spec(period=8, skip=2, min_samples=4, tol_lin=0.05)
    assert (s["period"], s["skip"], s["min_samples"], s["min_tries"], s["promote_rate"], s["p_zero"]) == (8, 2, 4, 16, 0.75, 0.1)
    assert CC.SETTINGS["period"] == 500 and CC.SETTINGS["skip"] == 25 and CC.SETTINGS["min_samples"] == 50 and E.CURR_LMAX == 5
    c = CC.curriculum_struct(s, HEAD, seed=7, env_id_offset=4096)
    assert list(c.n) == [8, 4, 8] and c.period == 8 and c.seed == 7 and c.env_id_offset == 4096 and c.tol_lin == np.float32(0.05)
    assert [np.float32(w) for w in c.width] == [(np.float32(0.222) - np.float32(-0.15)) / np.float32(8), (np.float32(0.2) - np.float32(-0.2)) / np.float32(4),
                                                 (np.float32(1.2) - np.float32(-1.2)) / np.float32(8)]
    assert [tuple(np.float32(v) for v in (c.head_lo[j], c.head_hi[j])) for j in range(4)] == [tuple(np.float32(v) for v in r) for r in HEAD]
    for bad, message in ((dict(period=0), "--curriculum_period"), (dict(min_tries=0), "--curriculum_min_tries"), (dict(skip=-1), "--curriculum_skip"),
                         (dict(promote_rate=1.5), "--curriculum_promote_rate"), (dict(tol_yaw=-1.0), "--curriculum_tol_yaw"),
                         (dict(p_zero=2.0), "--curriculum_p_zero"), (dict(pace=1), "unknown setting 'pace'")):
        with pytest.raises(ValueError, match=message):
            spec(**bad)


# ---- the step restatement: what the draws are
LEVELS = np.array([5, 0, 1, 2, 5, 0, 0, 0, 3, 1, 1, 1], np.int32)      # a 4 x 1 x 3 grid


def test_the_draws_follow_the_levels():
    """20 000 first-call draws of the restatement (seed 11): the share of every bin against level / total, of the zero command against
    p_zero, each within four binomial standard deviations; no command in a closed bin; every command inside its bin."""
    n = 20000
    s = spec("vx=-0.15:0.222:4,wz=-1.2:1.2:3")
    cur = CC.curriculum_struct(s, HEAD, seed=11, env_id_offset=3)
    cdf = np.cumsum(LEVELS).astype(np.int32)
    counts, state = np.zeros((12, 2), np.int32), np.zeros((n, E.CURR_NSTATE), np.float32)
    cmd, priv, obs = np.full((n, 7), 9.0, np.float32), np.full((n, NPRIV), 9.0, np.float32), np.full((n, NOBS), 9.0, np.float32)
    drew = CC.curriculum_step_reference(cur, NOBS, priv, None, None, cdf, counts, state, cmd, obs)
    assert drew.all() and not counts.any() and (state[:, E.CURR_HEAD] == 1).all() and (state[:, E.CURR_EPISODE] == 1).all()
    assert (state[:, E.CURR_STINT] == 1).all() and not state[:, [E.CURR_STEP, E.CURR_SAMPLES, E.CURR_SQLIN, E.CURR_SQYAW]].any()
    assert np.array_equal(obs[:, 6:13], cmd) and np.array_equal(priv[:, 6:13], cmd) and (obs[:, :6] == 9).all() and (priv[:, 13:] == 9).all()
    b = state[:, E.CURR_BIN].astype(int)
    zero = b < 0
    sd = lambda p, m: np.sqrt(p * (1 - p) / m)
    assert abs(zero.mean() - 0.1) <= 4 * sd(0.1, n), zero.mean()
    assert not cmd[zero].any()
    m, total = int((~zero).sum()), int(LEVELS.sum())
    share = np.bincount(b[~zero], minlength=12) / m
    for k in range(12):
        p = LEVELS[k] / total
        assert abs(share[k] - p) <= 4 * sd(p, m), (k, share[k], p)
        assert LEVELS[k] > 0 or share[k] == 0
    ex, ew = np.asarray(CC.bin_edges(s)["vx"], np.float64), np.asarray(CC.bin_edges(s)["wz"], np.float64)
    ix, iz = b[~zero] // 3, b[~zero] % 3
    c = cmd[~zero].astype(np.float64)
    eps = 1e-6      # the edges are float64 linspace, the commands float32 sums: an ulp of 0.2 is 1.5e-8
    assert (c[:, 0] >= ex[ix] - eps).all() and (c[:, 0] <= ex[ix + 1] + eps).all() and (c[:, 0] <= float(np.float32(0.222))).all()
    assert (c[:, 2] >= ew[iz] - eps).all() and (c[:, 2] <= ew[iz + 1] + eps).all()
    assert (c[:, 1] >= -0.2 - eps).all() and (c[:, 1] <= 0.2 + eps).all() and c[:, 1].std() > 0.1      # the unnamed axis: one bin, the env's range
    for j, (lo, hi) in enumerate(HEAD):
        assert (c[:, 3 + j] >= lo - eps).all() and (c[:, 3 + j] <= hi + eps).all() and c[:, 3 + j].std() > 0.2 * (hi - lo)
    # total == 0: the zero command everywhere
    state[:] = 0
    CC.curriculum_step_reference(cur, NOBS, priv, None, None, np.zeros(12, np.int32), counts, state, cmd, obs)
    assert not cmd.any() and (state[:, E.CURR_BIN] == -1).all()


def test_a_stint_is_sampled_judged_and_redrawn():
    """One env by hand: period 4, skip 1, min_samples 2; tolerances 0.1 / 0.2."""
    s = spec("vx=0:0.2:1", period=4, skip=1, min_samples=2, tol_lin=0.1, tol_yaw=0.2, p_zero=0.0)
    cur = CC.curriculum_struct(s, HEAD, seed=1)
    cdf, counts = np.array([5], np.int32), np.zeros((1, 2), np.int32)
    state, cmd, priv = np.zeros((1, 8), np.float32), np.zeros((1, 7), np.float32), np.zeros((1, NPRIV), np.float32)
    z = np.zeros(1, np.float32)
    CC.curriculum_step_reference(cur, NOBS, priv, z, z, cdf, counts, state, cmd)
    first = cmd.copy()
    assert state[0, E.CURR_BIN] == 0 and 0 <= first[0, 0] <= 0.2
    priv[0, NOBS + 9], priv[0, NOBS + 10], priv[0, NOBS + 2] = first[0, 0] + np.float32(0.05), first[0, 1], first[0, 2]
    for k in range(3):
        assert not CC.curriculum_step_reference(cur, NOBS, priv, z, z, cdf, counts, state, cmd).any()
    assert state[0, E.CURR_STEP] == 3 and state[0, E.CURR_SAMPLES] == 2 and np.array_equal(cmd, first)      # step 0 of the stint is skipped
    assert CC.curriculum_step_reference(cur, NOBS, priv, z, z, cdf, counts, state, cmd).all()                   # STEP reaches the period
    assert counts.tolist() == [[1, 1]] and state[0, E.CURR_EPISODE] == 1 and state[0, E.CURR_STINT] == 2 and not np.array_equal(cmd, first)
    # a fall: a try, no success, a new episode
    one = np.ones(1, np.float32)
    CC.curriculum_step_reference(cur, NOBS, priv, one, z, cdf, counts, state, cmd)
    assert counts.tolist() == [[2, 1]] and state[0, E.CURR_EPISODE] == 2 and state[0, E.CURR_STINT] == 1
    # a truncation with too few samples: not counted
    CC.curriculum_step_reference(cur, NOBS, priv, one, one, cdf, counts, state, cmd)
    assert counts.tolist() == [[2, 1]] and state[0, E.CURR_EPISODE] == 3


# ---- the update restatement
def ring_spec(n=(5, 1, 4), **kw):
    return spec(f"vx=0:1:{n[0]},vy=0:1:{n[1]},wz=0:1:{n[2]}", "vx=0:1,vy=0:1,wz=0:1", **kw)


def test_levels_spread_one_ring_per_update():
    s = ring_spec()
    cur = CC.curriculum_struct(s, HEAD)
    shape, at = (5, 1, 4), (1, 0, 2)
    levels = np.zeros(shape, np.int32)
    levels[at] = E.CURR_LMAX
    levels, cdf, stats = levels.reshape(-1), np.zeros(20, np.int32), np.zeros(4, np.int32)
    ix, iy, iz = np.indices(shape)
    dist = (abs(ix - at[0]) + abs(iy - at[1]) + abs(iz - at[2])).reshape(-1)
    open_at = np.full(20, -1)
    open_at[dist == 0] = 0
    diameter, saturated = int(dist.max()), None
    for update in range(1, diameter + 6):
        # the policy tracks perfectly wherever a command can be drawn: only open bins gather tries
        counts = np.where((levels > 0)[:, None], np.int32(cur.min_tries), np.int32(0)).astype(np.int32) * np.ones((1, 2), np.int32)
        CC.curriculum_update_reference(cur, levels, cdf, counts, stats)
        open_at[(levels > 0) & (open_at < 0)] = update
        assert np.array_equal(cdf, np.cumsum(levels)) and not counts.any()
        if saturated is None and (levels == E.CURR_LMAX).all():
            saturated = update
    assert np.array_equal(open_at, dist), "a bin at Manhattan distance d opens at update d"
    # the farthest bin opens at update `diameter` with level >= 1 and gains at least 1 (itself) per update after it
    assert saturated is not None and diameter < saturated <= diameter + E.CURR_LMAX - 1, (saturated, diameter)
    assert stats[E.CURR_STAT_UPDATES] == diameter + 5 and stats[E.CURR_STAT_JUDGED] == stats[E.CURR_STAT_PROMOTED] > 20


def test_with_every_bin_tried_the_grid_saturates_in_its_diameter():
    """Every bin at min_tries tries, all successes: a bin with f neighbours gains 1 + f >= 2 per update, so from one LMAX bin every level
    is LMAX after ceil(LMAX / 2) = 3 updates at the most -- and the 1 x 1 x 1 grid's one bin, with no neighbour, needs LMAX from 0."""
    s = ring_spec()
    cur = CC.curriculum_struct(s, HEAD)
    levels, cdf, stats = np.zeros(20, np.int32), np.zeros(20, np.int32), np.zeros(4, np.int32)
    levels[6] = E.CURR_LMAX
    for update in range(3):
        counts = np.full((20, 2), cur.min_tries, np.int32)
        CC.curriculum_update_reference(cur, levels, cdf, counts, stats)
    assert (levels == E.CURR_LMAX).all() and cdf[-1] == 100 and stats.tolist() == [3, 60, 60, 60 * cur.min_tries]
    cur = CC.curriculum_struct(ring_spec((1, 1, 1)), HEAD)
    levels, cdf = np.zeros(1, np.int32), np.zeros(1, np.int32)
    for update in range(E.CURR_LMAX):
        assert levels[0] == update
        CC.curriculum_update_reference(cur, levels, cdf, np.full((1, 2), 16, np.int32), stats)
    assert levels[0] == cdf[0] == E.CURR_LMAX


def test_failures_promote_nothing_and_a_bin_short_of_tries_keeps_its_counters():
    s = ring_spec()
    cur = CC.curriculum_struct(s, HEAD)
    levels = np.array([0, 1, 2, 3, 4, 5] * 3 + [0, 5], np.int32)
    before, cdf, stats = levels.copy(), np.zeros(20, np.int32), np.zeros(4, np.int32)
    counts = np.zeros((20, 2), np.int32)
    counts[:, 0] = cur.min_tries
    counts[3] = (cur.min_tries - 1, cur.min_tries - 1)      # all successes, one try short
    counts[7] = (cur.min_tries, 11)                         # 11 / 16 < 0.75
    counts[8] = (cur.min_tries + 4, 15)                     # 15 / 20 = 0.75: promoted (>=)
    CC.curriculum_update_reference(cur, levels, cdf, counts, stats)
    want = before.copy()
    for k in (8, 8 - 4, 8 + 4, 8 - 1, 8 + 1):                # (5 x 1 x 4: strides 4 and 1; bin 8 is (2, 0, 0): no bin below it on wz)
        if k == 7:
            continue
        want[k] = min(E.CURR_LMAX, want[k] + 1)
    assert np.array_equal(levels, want) and np.array_equal(cdf, np.cumsum(want))
    assert counts[3].tolist() == [15, 15] and not np.delete(counts, 3, 0).any()
    assert stats.tolist() == [1, 19, 1, 16 * 18 + 20]
    levels2 = before.copy()
    counts = np.zeros((20, 2), np.int32)
    counts[:, 0] = cur.min_tries
    CC.curriculum_update_reference(cur, levels2, cdf, counts, stats)
    assert np.array_equal(levels2, before) and not counts.any() and np.array_equal(cdf, np.cumsum(before))


# ---- the runner's flags
def test_the_runner_takes_the_flags_and_standing_refuses_them(capsys):
    from open_duck_playground_amd import runner
    parser = runner.build_parser()
    args = parser.parse_args(["--command_curriculum", "vx=-0.15:0.222:8,wz=-1.2:1.2:8", "--curriculum_start", "vx=-0.15:0.222,wz=-1.2:1.2",
                              "--curriculum_period", "250", "--curriculum_tol_lin", "0.07", "--train_sensor", "imu_delay=0:3"])
    runner.check_env_flags(parser, args)
    s = CC.spec_from_args(args)
    assert s["period"] == 250 and s["tol_lin"] == 0.07 and s["skip"] == 25 and (CC.initial_levels(s) == 5).all()
    assert CC.spec_from_args(parser.parse_args([])) is None
    for argv, message in ((["--env", "standing", "--command_curriculum", "vx=0:0.1:2"], "--command_curriculum belongs to --env joystick"),
                          (["--curriculum_period", "10"], "--curriculum_* flags need --command_curriculum"),
                          (["--command_curriculum", "vx=0:1:99"], "--command_curriculum: vx has 99 bins")):
        with pytest.raises(SystemExit):
            runner.check_env_flags(parser, parser.parse_args(argv))
        assert message in capsys.readouterr().err, message


def test_the_checkpoint_round_trips_the_curriculum(tmp_path):
    import torch
    from open_duck_playground_amd import track
    from open_duck_playground_amd.ppo import train as T
    from open_duck_playground_amd.ppo.networks import PPONetworks
    net = PPONetworks(101, 212, 14)
    described = dict(spec=spec(), levels=CC.initial_levels(spec()).reshape(8, 4, 8).tolist(), coverage=0.5625)
    with_, without = str(tmp_path / "with.pt"), str(tmp_path / "without.pt")
    T.save_checkpoint(with_, net, command_curriculum=described)
    T.save_checkpoint(without, net)
    assert track.trained_with_curriculum(with_) == described and track.trained_with_curriculum(without) is None
    assert "command_curriculum" not in torch.load(without, map_location="cpu") and track.trained_under(with_) is None
