"""What the NaN-filled-LDS tests (tests/test_gpu_lds_poison.py) rest on, checked without a GPU: the driver's env table reaches every compiled
kernel instantiation, every source file with shared memory carries the switch, and the Makefile builds a poison object for every object of
the product library."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")


def _sets():
    """{set name: [(lanes, floor), ...]} from the ODK_ENV_SET_* lines of odk_shapes.h, found with the Makefile's own pattern"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    pat = re.search(r"set_names = \$\(shell sed -n 's/(.*)/\\1/p' \$\(1\)\)", mk).group(1)
    assert pat == r"^\#define ODK_ENV_SET_\([A-Za-z0-9]*\)(X).*", pat      # (the sed pattern restated as a Python one below)
    out = {}
    for line in open(os.path.join(CSRC, "odk_shapes.h")):
        m = re.match(r"^#define ODK_ENV_SET_([A-Za-z0-9]*)\(X\)(.*)", line)
        if m:
            out[m.group(1)] = [(int(g), int(hf)) for _, g, hf in re.findall(r"X\((\w+), (\d+), (\d+)\)", m.group(2))]
            assert out[m.group(1)], line
    return out


def test_the_env_table_covers_every_compiled_instantiation():
    from lds_poison_driver import ENV_CASES, ENV_CONFIGS, NENV, NOT_COVERED
    sets = _sets()
    compiled = {(name, g, hf) for name, inst in sets.items() for g, hf in inst}
    assert len(compiled) == 12 and not any(re.fullmatch(r"U\d+", name) for name in sets)      # user shapes live in odk_shapes_user.h ...
    assert NOT_COVERED == "U<k>"                                                                 # ... and are named as not covered
    covered = {triple for _, triple, *_ in ENV_CASES}
    assert covered == compiled, (sorted(compiled - covered), sorted(covered - compiled))
    assert NENV == 5 and ENV_CONFIGS == ("defaults", "everything")      # three workgroups at 32 lanes, the last with a dead slot
    specs = {c[2] for c in ENV_CASES}
    assert {"tail_biped.xml", "tail_biped_equality.xml", "tail_biped_loop.xml"} <= specs
    for c in ENV_CASES:
        if isinstance(c[2], str) and c[2].endswith(".xml"):
            assert os.path.exists(os.path.join(ROOT, "tests", "assets", c[2]))


def test_every_file_with_shared_memory_has_the_switch():
    """... and as many fills as kernels that declare some: a fill follows every group of __shared__ declarations"""
    with_lds = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")) or f == "odk_poison.h":
            continue
        lines = open(os.path.join(CSRC, f)).read().split("\n")
        decl = [i for i, l in enumerate(lines) if re.match(r"\s*(extern )?__shared__ ", l)]
        if not decl:
            continue
        with_lds.append(f)
        text = "\n".join(lines)
        assert "#ifdef ODK_POISON_LDS" in text and "odk_poison_fill(" in text and '#include "odk_poison.h"' in text, f
        for i in decl:
            if i + 1 < len(lines) and re.match(r"\s*(extern )?__shared__ ", lines[i + 1]):
                continue      # (the fill follows the last declaration of the group)
            window = "\n".join(lines[i + 1: i + 14])
            assert "#ifdef ODK_POISON_LDS" in window and "odk_poison_fill(" in window, (f, i + 1, lines[i])
    assert with_lds == ["odk_env_kernels.h", "odk_learner.hip", "odk_mlp.hip"], with_lds
    assert "odk_poison.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_make_lists_a_poison_object_for_every_object_of_the_library(tmp_path):
    """`make -n libodk.so libodk_poison.so` in a copy of the sources (nothing is compiled: -n prints the commands)"""
    dst = tmp_path / "open_duck_playground_amd" / "csrc"
    dst.parent.mkdir(parents=True)
    shutil.copytree(CSRC, dst, ignore=shutil.ignore_patterns("*.o", "*.so", "*.s", "loader_check"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    out = subprocess.run(["make", "-n", "-C", str(dst), "libodk.so", "libodk_poison.so"], capture_output=True, text=True, check=True).stdout
    objs = set(re.findall(r"-o (\w+)\.o ", out))
    product = {o for o in objs if not o.endswith("_poison")}
    assert len(product) >= 11 and {o + "_poison" for o in product} == objs - product, sorted(objs)
    link = [l for l in out.split("\n") if "-o libodk_poison.so" in l]
    assert len(link) == 1 and all(f"{o}_poison.o" in link[0] for o in product) and "-DODK_POISON_LDS" in out
