"""Host-side checks of the select census (tools/isa_select_census.py, profiles/selects), run on a listing of shape A's kernel set compiled here
(CPU only, cross-compiled for gfx950 with -DODK_MARK)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_SUBSTEP_SELECTS = 666     # v_cndmask_b32 in one substep of step_kernel<ShapeA,32,0> at the commit before (profiles/load_waits/isa_overhead_census.txt)
PARENT_SUBSTEP_VALU = 6450


@pytest.fixture(scope="module")
def listing_a(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_overhead_census as overhead
    import isa_select_census as census
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to compile the listing the census reads")
    out = os.path.join(str(tmp_path_factory.mktemp("select_census")), "odk_env_A.s")
    return overhead, census, overhead.compile_listing("A", out)


def test_regions_and_sums(listing_a):
    overhead, census, listing = listing_a
    stats = census.census(listing, "A", passes=2.0)
    regions = list(stats)
    assert regions[0] == "pre" and regions[-1] == "after 17" and "after 15" in regions and census.LOOP in regions, regions
    # the loop body is a region of its own, between the line search's set-up and its end
    loop = stats[census.LOOP]
    assert loop["sel"] > 0 and loop["valu"] > loop["sel"], dict(loop)
    assert loop["weight"] == 2.0 * census.SUBSTEPS and stats["after 8"]["weight"] == census.SUBSTEPS and stats["pre"]["weight"] == 1
    # every select of the function is in exactly one region
    body = open(listing).read().split("\n")
    start = next(i for i, l in enumerate(body) if l.startswith("_Z11step_kernel") and overhead.KEYS["A"] in l and "Li32ELi0E" in l)
    end = next(i for i in range(start, len(body)) if body[i].startswith(".Lfunc_end"))
    total = sum(1 for l in body[start:end] if re.match(r"\tv_cndmask_b32", l))
    assert total > 0 and all(d["sel"] >= 0 for d in stats.values())
    assert sum(d["sel"] for d in stats.values()) == total
    assert sum(1 for d in stats.values() if d["sel"] > 0) >= 15
    for d in stats.values():
        assert d["sel"] == d["vop2"] + d["vop3"] and d["zero_mulfma"] <= min(d["zero"], d["mulfma"]) and d["adj"] <= d["vop2"] and d["dyn_sel"] == d["weight"] * d["sel"]
        assert 0 <= d["dup"] <= d["cmp_fed"] and 0 <= d["fill"] <= d["sel"]
    # the regions agree with the overhead census, which knows no loop region: "after 15" there is "after 15" + the loop body here
    old = overhead.census(listing, "A")
    assert old["after 15"]["cndmask"] == stats["after 15"]["sel"] + loop["sel"]
    assert old["after 8"]["cndmask"] == stats["after 8"]["sel"] and old["after 8"]["valu"] == stats["after 8"]["valu"]


def test_substep_is_leaner_than_the_parent(listing_a):
    overhead, census, listing = listing_a
    sub = census.substep(census.census(listing, "A"))
    print(dict(sub))
    assert 0 < sub["sel"] < PARENT_SUBSTEP_SELECTS, sub["sel"]
    assert 0 < sub["valu"] <= PARENT_SUBSTEP_VALU, sub["valu"]


def test_command_line_and_listing_of_selects(listing_a):
    overhead, census, listing = listing_a
    tool = os.path.join(ROOT, "tools", "isa_select_census.py")
    txt = subprocess.run([sys.executable, tool, "A", "--listing", listing, "--passes", "2"], check=True, capture_output=True, text=True).stdout
    head = txt.splitlines()[0].split()
    assert head[:3] == ["region", "valu", "sel"] and head[-3:] == ["weight", "dyn_sel", "dyn_valu"]
    assert any(l.startswith(census.LOOP) for l in txt.splitlines()) and any(l.startswith("substep") for l in txt.splitlines())
    rows = subprocess.run([sys.executable, tool, "A", "--listing", listing, "--list"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(rows) == sum(d["sel"] for d in census.census(listing, "A").values())
    assert all("v_cndmask_b32" in r for r in rows) and any(" v_cmp_" in r for r in rows)


def test_a_listing_without_the_loop_marker_is_refused(listing_a, tmp_path):
    """No silent census without the loop region: a listing that lacks LS_LOOP_0 stops the tool, and --mark-loop-before puts the marker in."""
    overhead, census, listing = listing_a
    bare = os.path.join(str(tmp_path), "bare.s")
    with open(bare, "w") as f:
        f.write("\n".join(l for l in open(listing).read().split("\n") if "; LS_LOOP_" not in l))
    with pytest.raises(SystemExit, match="LS_LOOP_0"):
        census.census(bare, "A")
    with pytest.raises(SystemExit, match="no line of the kernel"):
        census.census(bare, "A", mark_before="no such instruction text")
    ref = census.census(listing, "A")
    # marked by hand in front of the first instruction behind the marker's place, the same loop is found
    body = open(listing).read().split("\n")
    start = next(i for i, l in enumerate(body) if l.startswith("_Z11step_kernel") and overhead.KEYS["A"] in l and "Li32ELi0E" in l)
    at = next(i for i in range(start, len(body)) if "; LS_LOOP_0" in body[i])
    text = next(body[i].strip() for i in range(at + 1, len(body)) if body[i].startswith("\tv_"))
    again = census.census(bare, "A", mark_before=text)
    assert again[census.LOOP]["sel"] == ref[census.LOOP]["sel"] and again[census.LOOP]["valu"] == ref[census.LOOP]["valu"]


def test_kernels_keep_f32_denormals(listing_a):
    """The line search of the plane-floor step kernel divides by 2 t2 (+ MINVAL for t2 = 0) without a guard against zero: that holds because a
    non-zero t2 doubled is never flushed to zero, i.e. because every kernel of the set runs with f32 denormals kept (mode 3)."""
    overhead, census, listing = listing_a
    modes = re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", open(listing).read())
    assert modes and set(modes) == {"3"}, sorted(set(modes))
