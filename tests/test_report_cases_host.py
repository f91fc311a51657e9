"""tests/report_cases.py, the scaffold of the report GPU tests, judged on the CPU: its comparer and its frozen-row check can fail, its
synthetic first episodes are what they claim, and the synthetic inputs of the gait, posture, imitation and fall tests are, bit for bit,
the inputs those tests had before they shared a scaffold."""
import hashlib

import numpy as np
import pytest

import report_cases as RC
import test_gpu_falls as falls
import test_gpu_gait as gait
import test_gpu_imitation_report as imitation
import test_gpu_posture as posture

# ---- compare_sums: three envs with N = 4, 12 and 0 samples; column 0 the sample count, 1 a sum of non-negative terms, 2 a signed sum
# whose terms' magnitudes add up to 2 (and to 0 in the env without a sample), 3 an exact column.  Powers of two, so that the bound,
# (N + 4) * 2^-23 * scale, and the sums with it are exact in float64.
WANT = np.array([[4.0, 1.0, -0.5, 3.0], [12.0, 2.0, 0.25, 5.0], [0.0, 0.0, 0.0, 0.0]])
SIGNED_SCALE = np.array([2.0, 2.0, 0.0])
BOUND = ((WANT[:, 0] + 4) * 2.0 ** -23)[:, None] * np.stack([WANT[:, 1], SIGNED_SCALE], 1)      # [env, column - 1]


def _compare(got):
    RC.compare_sums(got, WANT, 0, {1: WANT[:, 1], 2: SIGNED_SCALE}, "host")


def test_compare_sums_accepts_an_error_exactly_at_the_bound(capsys):
    got = WANT.copy()
    got[:2, 1] += BOUND[:2, 0]
    got[:2, 2] -= BOUND[:2, 1]
    assert np.all(np.abs(got[:2, 1:3] - WANT[:2, 1:3]) == BOUND[:2]) and np.all(BOUND[:2] > 0)      # the arithmetic above was exact
    _compare(got)
    assert capsys.readouterr().out == "host: float32 sums, worst error / bound 1.000\n"
    _compare(WANT)


@pytest.mark.parametrize("col", [1, 2])
@pytest.mark.parametrize("env", [0, 1])
def test_compare_sums_refuses_one_ulp_beyond_the_bound(env, col):
    got = WANT.copy()
    at = WANT[env, col] + BOUND[env, col - 1]
    got[env, col] = np.nextafter(at, np.inf)
    assert got[env, col] - WANT[env, col] > BOUND[env, col - 1]
    with pytest.raises(AssertionError):
        _compare(got)
    got[env, col] = at
    _compare(got)


def test_compare_sums_refuses_one_bit_in_an_exact_column():
    got = WANT.astype(np.float32)
    _compare(got)
    got[1, 3] = np.nextafter(got[1, 3], np.float32(0))
    with pytest.raises(AssertionError, match="slot 3"):
        _compare(got)
    got = WANT.astype(np.float32)
    got[0, 0] += 1                                   # the sample count is an exact column too
    with pytest.raises(AssertionError, match="slot 0"):
        _compare(got)


@pytest.mark.parametrize("col", [1, 2])
def test_compare_sums_is_exact_where_no_sample_was_taken(col):
    assert np.all(BOUND[2] == 0.0)
    got = WANT.copy()
    got[2, col] = 5e-324                             # the least float64 above 0
    with pytest.raises(AssertionError):
        _compare(got)


# ---- first_episodes
GAIT_ENDS = dict(ends=(25, 0, 0, 11, 17), truncated=(2, 4))


def test_first_episodes_are_what_they_claim():
    T, n = 24, 37
    end_at, done, trunc, ended = RC.first_episodes(np.random.default_rng(5), T, n, **GAIT_ENDS)
    assert done.dtype == trunc.dtype == ended.dtype == np.float32 and done.shape == trunc.shape == ended.shape == (T, n)
    assert list(end_at[:10]) == [25, 0, 0, 11, 17, 25, 0, 0, 11, 17]
    strays = 0
    for e in range(n):
        assert np.all(done[:min(end_at[e], T), e] == 0)                         # none before the end
        if end_at[e] < T:
            assert done[end_at[e], e] == 1
            strays += int(done[end_at[e] + 1:, e].sum())
        np.testing.assert_array_equal(trunc[:, e], done[:, e] if e % 5 in (2, 4) else 0.0)      # truncation only for those residues
        np.testing.assert_array_equal(ended[:, e], np.arange(T) > end_at[e])
    assert strays > 20                                                          # stray flags after the end do occur
    assert set(end_at.clip(max=T)) == {0, 11, 17, T}                            # the sample counts of the gait and posture tests
    # one draw, of uniform(size=(T, n)): the caller's stream is where that leaves it
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    RC.first_episodes(a, T, n, **GAIT_ENDS)
    b.uniform(size=(T, n))
    assert a.integers(0, 2 ** 62) == b.integers(0, 2 ** 62)


# ---- assert_frozen_after_end
def test_assert_frozen_after_end_fails_on_one_changed_bit():
    T, n, nacc = 6, 4, 5
    end_at = np.array([7, 0, 3, 5])
    snaps = np.zeros((T, n, nacc), np.float32)
    for t in range(T):
        for e in range(n):
            snaps[t, e] = 0.0 if end_at[e] == 0 else min(t, end_at[e] - 1) + 1 + np.arange(nacc)      # a row changes until its last sample
    assert RC.assert_frozen_after_end(snaps, end_at) == 6 + 3 + 1
    for t, e in ((5, 2), (3, 2), (5, 3), (0, 1), (4, 1)):
        bad = snaps.copy()
        bad[t, e, 4] = np.nextafter(bad[t, e, 4], np.float32(np.inf)) if bad[t, e, 4] else np.float32(1e-45)      # one bit
        with pytest.raises(AssertionError, match=f"env {e} step {t}"):
            RC.assert_frozen_after_end(bad, end_at)
    ok = snaps.copy()
    ok[4, 0, 2] += 1                                 # a live row may change
    ok[1, 2, 2] += 1                                 # and so may a row before its end
    assert RC.assert_frozen_after_end(ok, end_at) == 10


# ---- the synthetic inputs keep their bits.  The digests were computed on the commit before the tests shared this scaffold, from the lines
# of each test that built the arrays, at the sizes the GPU tests use.  Those come from each robot's model on the host
# (RC.robot_sizes: engine.model_obs_sizes, the call a Batch makes), not from a batch.
def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("robot,nu,null_limit,sha", [
    ("duck", 14, False, "f4dee1d49db2881a40039b57ae32bd301221f335bf42e795fb253512a7705628"),
    ("tail_biped.xml", 15, False, "915709bd5b0ba115c5ab1b109b2e4e1ca7446d5d3963bdedc370bb9201b51c68"),
    ("biped_arms.xml", 16, True, "58343b25cbc497e784ba54fd3f3d72010662cfc29658b2861224792a99121a5b")])
def test_gait_inputs_keep_their_bits(robot, nu, null_limit, sha):
    nobs, npriv, nu_, _, _ = RC.robot_sizes(robot)
    assert nu_ == nu
    priv, done, trunc, ended, end_at, limit = gait.synthetic_inputs(nobs, npriv, nu, null_limit)
    assert (limit is None) == null_limit
    assert digest(priv, done, trunc, ended, *([] if limit is None else [limit])) == sha


@pytest.mark.parametrize("case,sha", [
    ("duck", "8e25fe4e073d5d23f8330258621d11634400c1d6fdee3727720ba25216c67a78"),
    ("tail_biped", "7c652773b4664c2e3bc0649c08b655221fc2598ca88d3ae724e8b9e66ebd9d70"),
    ("biped_arms", "5dae44b1c3c92746388a552485102a1f1d8a378e3d65a0377f568948e9c3fb61"),
    ("biped12", "2f2a49970cea16c590fb681157594274c5e34c9e6bdff62b09f6c81dedc6aa02")])
def test_posture_inputs_keep_their_bits(case, sha):
    assert list(posture.CASES) == ["duck", "tail_biped", "biped_arms", "biped12"]
    robot, nu, given = posture.CASES[case]
    nobs, npriv, nu_, _, kc = RC.robot_sizes(robot)
    assert nu_ == nu
    hmap = [5, 6, 7, 8] if given is None else list(given)
    priv, done, trunc, ended, cmd, end_at, pattern = posture.synthetic_inputs(nobs, npriv, nu, hmap, kc)
    assert digest(priv, done, trunc, ended, cmd) == sha


@pytest.mark.parametrize("case,sha", [
    ("duck", "93b2de3ea485e52786987c8dbbd840de473fd99505d085e8bc2af9e0c427fef6"),
    ("biped12", "b8f537a3d75ad329e5701234b93f5fe77859df8a6121c0a68d702f9b0148cfd9"),
    ("tail_biped", "ec27cb49f3a7a80307b61cce3231aff65b4e7c7c04ba902982adda91d439fe47"),
    ("biped_arms", "674c1377a81dbbf220bda47acee9609fd787aef43a6ef32e1471804c3c5f7ba6"),
    ("duck_unfolded", "93b2de3ea485e52786987c8dbbd840de473fd99505d085e8bc2af9e0c427fef6")])      # the duck's rows under another period
def test_imitation_inputs_keep_their_bits(case, sha):
    assert list(imitation.CASES) == ["duck", "biped12", "tail_biped", "biped_arms", "duck_unfolded"]
    robot, nu, _, _ = imitation.CASES[case]
    nobs, npriv, nu_, _, _ = RC.robot_sizes(robot)
    assert nu_ == nu
    priv, done, trunc, ended, end_at = imitation.synthetic_inputs(nobs, npriv, nu)
    assert digest(priv, done, trunc, ended) == sha


@pytest.mark.parametrize("robot,nu,limits,sha", [
    ("flat_terrain", 14, "given", "ceac1d6be55fb42524c3ef0103035daf76d365c8bd07c9a9243ad394295e0e30"),
    ("flat_terrain_backlash", 14, None, "7f867a3a1e61bd67805383d0e691d7fc983631e4d84b3a5d60d298699af33bb6"),
    ("biped_arms.xml", 16, "given", "bf0dcd8dbba2cb630c0d3c919abbf6509d0f3a2532574604d9e0f153c21ba964")])
def test_fall_inputs_keep_their_bits(robot, nu, limits, sha):
    nobs, npriv, nu_, nq, _ = RC.robot_sizes(robot)
    assert nu_ == nu
    priv, done, trunc, qpos, cmd, end_at, limit = falls.synthetic_inputs(nobs, npriv, nu, nq, limits)
    assert digest(priv, done, trunc, qpos, cmd, *([] if limit is None else [limit])) == sha
