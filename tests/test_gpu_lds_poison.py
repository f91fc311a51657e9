"""Every kernel that has LDS, started from NaN-filled LDS (csrc/odk_poison.h, libodk_poison.so), returns what the product library returns.

LDS is not cleared between launches: a word read before this launch wrote it holds what the CU's previous workgroup left there -- in any
other test of this suite the same kernel's data for a neighbouring env or tile, which looks right.  Here tests/lds_poison_driver.py runs
one kernel family in a child process on libodk.so and again on libodk_poison.so (same sources with -DODK_POISON_LDS: the only extra device
code is the fill at each kernel's start), and every array the two children stored must agree BIT FOR BIT (compared as uint32: NaN payloads
and the sign of zero count).  Not compared that way: the NaN-word counts of the debug images (the poison child's must be non-zero for every
instantiation: the fill ran on the device and survived where nothing wrote) and the four loss sums that workgroups fold with float atomics
(`@unordered`: their order is not fixed from run to run; both children hold them to float64 at the suite's own bounds).

The children run one after the other, each under a time limit of its own; one that ends on a signal, aborts (134), faults (139) or runs
into its limit fails its test with its stderr, and the other poison test then fails at once without starting anything on the GPU.
Time limits: ten times the product child's wall time measured on an MI355X (profiles/lds_poison/NOTES.md); process start and context
creation dominate -- the limits end a hang, they measure nothing."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "lds_poison_driver.py")
LIMITS = {"env": 40, "learner": 40}      # seconds = 10 x the product children measured on an MI355X (env 3.6 s, learner 3.9 s: profiles/lds_poison/NOTES.md)
_ended_badly = []                            # a child that faulted or hung: nothing more is started on the GPU by these tests


def _libraries():
    from open_duck_playground_amd import engine
    product = os.path.join(os.path.dirname(engine.POISON_LIB_PATH), "libodk.so")
    newest = max(os.path.getmtime(s) for s in engine.library_sources())
    for lib in (product, engine.POISON_LIB_PATH):
        assert os.path.exists(lib) and os.path.getmtime(lib) >= newest, \
            f"{lib} is missing or older than csrc/: run `python -c 'import __graft_entry__ as g; g.build()'` (no test compiles anything)"
    return product, engine.POISON_LIB_PATH


def _child(family, lib, out):
    assert not _ended_badly, f"not started: an earlier child ended badly ({_ended_badly[0]})"
    env = dict(os.environ, ODK_LIB=lib)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, DRIVER, "--family", family, "--out", out], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=LIMITS[family])
    except subprocess.TimeoutExpired as e:
        _ended_badly.append(f"{family} on {os.path.basename(lib)}: still running after {LIMITS[family]} s")
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"{_ended_badly[-1]}\n{err[-4000:]}")
    print(r.stdout)
    print(f"{family} child on {os.path.basename(lib)}: {time.time() - t0:.1f} s of a limit of {LIMITS[family]} s")
    if r.returncode < 0 or r.returncode in (134, 139):
        _ended_badly.append(f"{family} on {os.path.basename(lib)}: exit status {r.returncode}")
        pytest.fail(f"{_ended_badly[-1]}\n{r.stderr[-4000:]}")
    assert r.returncode == 0, f"{family} on {os.path.basename(lib)}: exit status {r.returncode}\n{r.stderr[-4000:]}"
    z = np.load(out)
    return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view(np.uint32 if a.dtype.itemsize % 4 == 0 else np.uint8)


def _compare(product, poison):
    """-> the differences, first differing element of each array named (for a stack of launches: the launch)"""
    lone = sorted(set(product) ^ set(poison))      # (a float64 check that stops early under the poison library records fewer calls)
    bad = [f"{len(lone)} arrays stored by one child only: {lone[:6]} ..."] if lone else []
    for k in sorted(set(product) & set(poison)):
        if k == "library" or k.endswith("/nan_words") or k.endswith("@unordered"):
            continue
        a, b = product[k], poison[k]
        if a.dtype.kind in "US":      # launch labels, refusals, verdicts of the float64 checks
            if not np.array_equal(a, b):
                bad.append(f"{k}: {a!r} != {b!r}")
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{k}: {a.dtype}{a.shape} != {b.dtype}{b.shape}")
            continue
        ua, ub = _bits(a), _bits(b)
        if not np.array_equal(ua, ub):
            i = int(np.flatnonzero(ua != ub)[0])
            idx = np.unravel_index(i * ua.dtype.itemsize // a.dtype.itemsize, a.shape) if a.ndim else ()
            where = ""
            run = k.rsplit("/", 1)[0]
            if f"{run}/launches" in product and a.ndim and a.shape[0] == len(product[f"{run}/launches"]):
                where = f" (launch {product[f'{run}/launches'][idx[0]]})"
            bad.append(f"{k}: {int((ua != ub).sum())} of {ua.size} words differ, first at {tuple(int(x) for x in idx)}{where}: "
                       f"{a[idx]!r} ({int(ua[i]):#010x}) != {b[idx]!r} ({int(ub[i]):#010x})")
    return bad


def _both(family, tmp_path):
    product_lib, poison_lib = _libraries()
    product = _child(family, product_lib, str(tmp_path / "product.npz"))
    poison = _child(family, poison_lib, str(tmp_path / "poison.npz"))
    assert os.path.basename(str(product["library"])) == "libodk.so"
    assert os.path.basename(str(poison["library"])) == "libodk_poison.so", str(poison["library"])      # the poison child really loaded it
    bad = _compare(product, poison)
    assert not bad, f"{len(bad)} arrays differ between libodk.so and libodk_poison.so:\n" + "\n".join(bad[:40])
    return product, poison


def test_env_kernels_from_poisoned_lds(tmp_path):
    """reset / step / debug step / physics kernels of all twelve (shape, lanes, floor) instantiations, defaults and everything on (and
    Standing): outputs, records and state after every launch agree bit for bit; refusals are the same refusal; and every instantiation
    has a dumped launch whose image holds NaN words under the poison library."""
    from lds_poison_driver import ENV_CASES
    product, poison = _both("env", tmp_path)
    for name, triple, *_ in ENV_CASES:
        counts = [poison[k] for k in poison if k.startswith(name + "/") and k.endswith("/nan_words")]
        assert counts, f"{name} {triple}: every configuration was refused"
        assert max(int(c.max()) for c in counts) > 0, f"{name} {triple}: no dumped image holds a NaN word: did the fill run?"


def test_learner_kernels_from_poisoned_lds(tmp_path):
    """The whole-network kernels, the weight-gradient GEMM and its finishing launch, GAE (three kernels), the loss head alone and fused,
    the clip + Adam forms with the packed copies, the column-sum and moments kernels: every tensor around every launch agrees bit for bit,
    and the float64 checks pass in both children."""
    product, poison = _both("learner", tmp_path)
    checks = [k for k in poison if k.endswith("/check")]
    assert checks and all(str(poison[k]) == "ok" for k in checks), {k: str(poison[k]) for k in checks if str(poison[k]) != "ok"}
