"""engine.py's accumulator slot constants (TRACK_*, PUSH_*, GAIT_*, POSTURE_*, IMIT_*, SCHED_*, RESP_*, FALL_*) are hand copies of include/odk.h's
ODK_* defines and enum entries: every one has its constant with the same value, and no such constant lacks one."""
import os
import re

from open_duck_playground_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIXES = "TRACK|PUSH|GAIT|POSTURE|IMIT|SCHED|RESP|FALL"
NUMBER = r"\d+(?:\.\d*)?(?:[eE][+-]?\d+)?f?"
TERM = rf"(?:{NUMBER}|ODK_\w+)"


def header_defines():
    """name (without ODK_) -> value of every `#define ODK_<PREFIX>_<NAME> <integer, float or product of such and earlier defines>` and of
    every `ODK_<PREFIX>_<NAME> = <integer>` of an enum"""
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    lines = re.findall(rf"^#define ODK_((?:{PREFIXES})_\w+)[ \t]+(.*?)[ \t]*(?://.*|/\*.*)?$", text, re.M)
    vals = {}
    for name, body in lines:
        m = re.fullmatch(rf"\(?\s*({TERM}(?:\s*\*\s*{TERM})*)\s*\)?", body)
        assert m, f"ODK_{name}: '{body}' is no integer, float or simple product"
        v = 1
        for t in re.split(r"\s*\*\s*", m.group(1)):
            if t.startswith("ODK_"):
                v *= vals[t[4:]]
            else:
                t = t.rstrip("f")
                v *= int(t) if t.isdigit() else float(t)
        vals[name] = v
    for block in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for name, v in re.findall(rf"\bODK_((?:{PREFIXES})_\w+)\s*=\s*(\d+)\s*(?:,|$)", re.sub(r"/\*.*?\*/", "", block).strip()):
            assert name not in vals, f"ODK_{name} twice"
            vals[name] = int(v)
    return vals


def test_every_slot_define_has_its_engine_constant_and_the_other_way_round():
    defines = header_defines()
    # the parser sees what is there: a product, a float, an enum entry, and every ODK_<PREFIX>_ name that the header gives a value at all
    assert defines["RESP_NACC"] == 192 and defines["SCHED_NEVER"] == 1.0e9 and defines["GAIT_RANGE_MAX"] == 128
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    assert set(re.findall(rf"\bODK_((?:{PREFIXES})_\w+)\s*=\s*\d", text)) | set(re.findall(rf"#define ODK_((?:{PREFIXES})_\w+)", text)) == set(defines)
    for name, v in defines.items():
        assert hasattr(engine, name), f"include/odk.h defines ODK_{name}, engine.py has no {name}"
        got = getattr(engine, name)
        assert got == v and isinstance(got, float) == isinstance(v, float), f"engine.{name} = {got!r}, include/odk.h says {v!r}"
    ours = [n for n in vars(engine) if re.fullmatch(rf"(?:{PREFIXES})_[A-Z0-9_]+", n)]
    assert sorted(set(ours) - set(defines)) == []
