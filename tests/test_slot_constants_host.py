"""engine.header_constants(), the one reader of include/odk.h's constants: it finds every ODK_ name the header gives a value, engine carries
each as a module global of that value and type, nothing else in engine looks like one, and each thing the grammar refuses is refused by
the constant's name."""
import re

import pytest

from open_duck_playground_amd import engine

# engine's upper-case numbers that the header does not define
BY_HAND = ("NCOMMAND", "MLP_MAX_OUT", "CURR_STREAM0", "ACTION_DELAY_ROWS")


def header_text() -> str:
    """include/odk.h without comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(engine.library_sources()[-1]).read(), flags=re.S)


def test_the_reader_finds_every_name_the_header_gives_a_value():
    consts = engine.header_constants()
    text = header_text()
    defined = set(re.findall(r"^\s*#\s*define\s+ODK_([A-Z0-9_]+)[ \t]+\S", text, re.M))       # `#define ODK_H` has no body, ODK_LOG_ROW( no blank
    assigned = set(re.findall(r"\bODK_([A-Z0-9_]+)\s*=[^=]", text))
    assert len(defined) == 48 and len(assigned) == 206 and not defined & assigned
    assert set(consts) == defined | assigned
    assert all(type(v) in (int, float) for v in consts.values())
    assert [k for k, v in consts.items() if type(v) is float] == ["SCHED_NEVER"]
    assert consts["RESP_NACC"] == 192 and consts["GAIT_RANGE_MAX"] == 128 and consts["SENSOR_NSTATE"] == 400 and consts["FAULT_NSLOT"] == 96
    assert consts["PATH_COURSE_FLOATS"] == 17 and consts["ADAM_ACC_FLOATS"] == 1026 and consts["ERR_INVALID"] == -1
    assert consts["SCHED_NEVER"] == 1.0e9 and isinstance(consts["SCHED_NEVER"], float)
    assert "H" not in consts and "LOG_ROW" not in consts


def test_every_header_constant_is_an_engine_global_and_the_other_way_round():
    consts = engine.header_constants()
    for name, v in consts.items():
        assert name in vars(engine), f"include/odk.h defines ODK_{name}, engine has no {name}"
        got = vars(engine)[name]
        assert got == v and type(got) is type(v), f"engine.{name} = {got!r}, include/odk.h says {v!r}"
    ours = {n for n, v in vars(engine).items() if n.isupper() and type(v) in (int, float)}
    assert sorted(ours - set(consts)) == sorted(BY_HAND)
    assert engine.MLP_HIDDEN == (512, 256, 128) and engine.NXTERM == len(engine.XTERM_NAMES) == 12
    assert engine.XTERM_NAMES == ("lin_vel_z", "ang_vel_xy", "orientation", "base_height", "energy", "joint_pos_limits", "termination", "pose",
                                  "feet_slip", "feet_clearance", "feet_height", "feet_air_time")
    assert [consts["XTERM_" + n.upper()] for n in engine.XTERM_NAMES] == list(range(12))


def test_the_grammar_on_synthetic_text():
    text = """
    #ifndef ODK_H
    #define ODK_H            /* no body: skipped */
    #define ODK_ROW(nu) (15 + 3 * (nu))     // function-like: skipped
    #define ODK_A 3 /* a comment
                       over two lines */
    #define ODK_B (1 + 2 * ODK_A)
    #define ODK_C 2.5e-1f
    #define ODK_D (ODK_B * ODK_C)
    #  define ODK_E -ODK_A - 1
    enum odk_kind { ODK_K0 = 0, ODK_K1 = ODK_B /* [2] */, ODK_K2 = -2, };
    enum { ODK_L = 4 };
    int odk_f(enum odk_kind k);
    """
    consts = engine.header_constants(text)
    assert consts == {"A": 3, "B": 7, "C": 0.25, "D": 1.75, "E": -4, "K0": 0, "K1": 7, "K2": -2, "L": 4}
    assert list(consts) == ["A", "B", "C", "D", "E", "K0", "K1", "K2", "L"]
    assert [type(consts[k]) for k in "ABCDE"] == [int, int, float, float, int]


@pytest.mark.parametrize("name,text", [
    ("ODK_A", "#define ODK_A 1\n#define ODK_A 2"),                              # a value twice: two defines
    ("ODK_A", "#define ODK_A 1\nenum { ODK_A = 1 };"),                          # ... a define and an enum entry
    ("ODK_B", "enum { ODK_A = 0, ODK_B = 1, ODK_B = 2 };"),                     # ... two enum entries
    ("ODK_A", "#define ODK_A (2 * ODK_B)\n#define ODK_B 1"),                    # a name not yet defined
    ("ODK_B", "enum { ODK_B = ODK_B };"),
    ("ODK_A", "#define ODK_A (1 << 4)"),                                        # other operators and characters
    ("ODK_A", "#define ODK_A 8 / 2"),
    ("ODK_A", "#define ODK_A 0x10"),
    ("ODK_A", "#define ODK_A 16u"),
    ("ODK_A", "#define ODK_A sizeof(int)"),
    ("ODK_A", "#define ODK_A __import__('os')"),
    ("ODK_A", "#define ODK_A \"text\""),
    ("ODK_B", "enum { ODK_A = 0, ODK_B = ODK_A | 2 };"),
    ("ODK_A", "#define ODK_A (1 +"),                                            # the right characters, no expression
    ("ODK_A", "#define ODK_A ()"),
    ("ODK_B", "enum { ODK_A = 0, ODK_B, ODK_C = 2 };"),                         # an enum entry without = value
    ("ODK_A", "enum { ODK_A };"),
])
def test_what_the_grammar_refuses_is_refused_by_the_constants_name(name, text):
    with pytest.raises(engine.OdkError, match=rf"^{name}:"):
        engine.header_constants(text)


def test_a_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "odk.h")
    monkeypatch.setattr(engine, "library_sources", lambda: ["Makefile", missing])
    with pytest.raises(engine.OdkError, match=re.escape(missing)):
        engine.header_constants()
