"""engine.SIGNATURES, the one ctypes declaration of every C entry point, held to the prototypes of include/odk.h: names, argument count and
kind, return type, and a struct pointer bound as a pointer to that struct's Structure; and every Structure held to its struct's layout as
the host C compiler sees it: size, and each field's offset and size.  Host-only: reads the header's text and the table, needs neither
libodk.so nor a device."""
import ctypes as C
import os
import re
import shlex
import subprocess

from conftest import ROOT
from open_duck_playground_amd import engine

SCALARS = {"long long": C.c_longlong, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double, "float": C.c_float, "int": C.c_int}
STRUCTS = {"odk_env_config": engine.EnvConfig, "odk_outputs": engine.Outputs, "odk_reward_terms": engine.RewardTerms,
           "odk_curriculum": engine.Curriculum, "odk_mlp_desc": engine.MlpDesc, "odk_step_tail": engine.StepTail,
           "odk_gae_head_args": engine.GaeHeadArgs, "odk_grad_finish": engine.GradFinish, "odk_weight_table": engine.WeightTableC}


def stripped_header() -> str:
    """include/odk.h without comments and preprocessor lines."""
    text = open(os.path.join(ROOT, "include", "odk.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)


def c_kind(name: str, decl: str, is_return: bool = False) -> str:
    """'pointer', 'void' (a return type only) or one of SCALARS' keys for a parameter declaration / a return type; fails by name otherwise."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    for kind in (" ".join(words), " ".join(words[:-1])):      # without, then with a parameter name behind the type
        if kind in SCALARS or (is_return and kind == "void"):
            return kind
    raise AssertionError(f"{name}: no rule for the C declaration {decl!r}")


def header_prototypes() -> dict:
    """name -> (return kind, [parameter kinds], [struct name or None per parameter]) of every odk_*( ... ); in the header."""
    text = stripped_header()
    protos = {}
    for m in re.finditer(r"\b(odk_[a-z_0-9]+)\s*\(", text):
        name = m.group(1)
        assert name not in protos, f"{name}: declared twice"
        tail = re.match(r"([^()]*)\)\s*;", text[m.end():])
        assert tail, f"{name}: not a plain prototype `{name}( ... );`"
        ret = re.split(r"[;{}]", text[:m.start()])[-1]
        assert ret.strip(), f"{name}: no return type in front of it"
        params = [p.strip() for p in tail.group(1).split(",")]
        if params in ([""], ["void"]):
            params = []
        structs = [next((s for s in STRUCTS if re.search(rf"\b{s}\b", p)), None) if "*" in p else None for p in params]
        protos[name] = (c_kind(name, ret, is_return=True), [c_kind(name, p) for p in params], structs)
    return protos


def ctypes_kind(name: str, t) -> str:
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C.Array))):
        return "pointer"
    for kind, ct in SCALARS.items():
        if t is ct:
            return kind
    raise AssertionError(f"{name}: no rule for the ctypes type {t!r}")


def mismatches(table: dict, protos: dict) -> list:
    """Every disagreement between a signature table and the header's prototypes, one line each, the function's name first."""
    bad = [f"{n}: declared in odk.h, missing from the table" for n in protos if n not in table]
    bad += [f"{n}: in the table, not declared in odk.h" for n in table if n not in protos]
    for n in protos:
        if n not in table:
            continue
        restype, argtypes = table[n]
        ret, kinds, structs = protos[n]
        if ctypes_kind(n, restype) != ret:
            bad.append(f"{n}: restype {restype!r} against the header's {ret}")
        have = [ctypes_kind(n, t) for t in argtypes]
        if have != kinds:
            bad.append(f"{n}: argtypes {have} against the header's {kinds}")
            continue
        for k, (t, s) in enumerate(zip(argtypes, structs)):
            if s is not None and t is not C.POINTER(STRUCTS[s]):
                bad.append(f"{n}: argument {k} is {t!r}, the header takes a pointer to {s}: POINTER({STRUCTS[s].__name__})")
    return bad


def test_signature_table_agrees_with_the_header():
    protos = header_prototypes()
    declared = set(re.findall(r"\b(odk_[a-z_0-9]+)\s*\(", stripped_header()))       # tests/test_capi_and_model.py's regex: nothing skipped
    assert len(protos) == len(declared) >= 74
    assert engine.EXPORTED_SYMBOLS == tuple(engine.SIGNATURES)
    assert set(engine.SIGNATURES) == set(protos) == declared
    assert engine.SIGNATURES["odk_last_error"][0] is C.c_char_p
    for name, (restype, _) in engine.SIGNATURES.items():
        assert restype in (None, C.c_int) or name == "odk_last_error", name
    assert sorted(n for n, (r, _) in engine.SIGNATURES.items() if r is None) == sorted(
        ["odk_default_config", "odk_default_config_standing", "odk_obs_sizes", "odk_model_free", "odk_batch_destroy", "odk_set_debug_dump",
         "odk_dw_set_profile", "odk_mlp_set_profile", "odk_mlp_set_wg_profile"])
    assert {s for _, _, structs in protos.values() for s in structs if s} == set(STRUCTS)      # every struct of the map is met in a prototype
    assert set(re.findall(r"\btypedef\s+struct\s*\w*\s*\{[^{}]*\}\s*(odk_\w+)\s*;", stripped_header())) == set(STRUCTS)     # and the header defines no other
    assert {v for v in vars(engine).values() if isinstance(v, type) and issubclass(v, C.Structure)} == set(STRUCTS.values())
    assert mismatches(engine.SIGNATURES, protos) == []


def test_the_comparison_reports_a_broken_entry_by_name():
    protos = header_prototypes()

    def broken(name, change):
        table = {n: (r, list(a)) for n, (r, a) in engine.SIGNATURES.items()}
        change(table)
        bad = mismatches(table, protos)
        assert len(bad) == 1 and bad[0].startswith(name + ":"), bad
        return bad[0]

    assert "argtypes" in broken("odk_step", lambda t: t["odk_step"][1].pop())                                   # an argument dropped
    k = engine.SIGNATURES["odk_physics_step"][1].index(C.c_int)
    assert "argtypes" in broken("odk_physics_step", lambda t: t["odk_physics_step"][1].__setitem__(k, C.c_float))   # an int turned float
    assert "missing from the table" in broken("odk_record_field", lambda t: t.pop("odk_record_field"))         # a name removed
    assert "not declared" in broken("odk_nothing", lambda t: t.__setitem__("odk_nothing", (C.c_int, [])))
    assert "restype" in broken("odk_model_free", lambda t: t.__setitem__("odk_model_free", (C.c_int, t["odk_model_free"][1])))
    assert "odk_outputs" in broken("odk_reset", lambda t: t["odk_reset"][1].__setitem__(3, C.c_void_p))        # a struct pointer left bare


def header_layout(structs: dict, workdir) -> dict:
    """What the host C compiler ($CC, else cc) makes of include/odk.h's structs: "odk_x" -> (sizeof,) and "odk_x.field" -> (offsetof, sizeof)
    for every field the map's Structures name, printed by a program generated from their `_fields_` and compiled in `workdir`."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "odk.h"', "int main(void) {"]
    for cname, S in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, *_ in S._fields_]
    src, exe = os.path.join(str(workdir), "layout.c"), os.path.join(str(workdir), "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines + ["  return 0;", "}", ""]))
    cc = shlex.split(os.environ.get("CC") or "cc")
    subprocess.run(cc + ["-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {words[0]: tuple(int(w) for w in words[1:]) for words in (line.split() for line in out.splitlines())}


def layout_mismatches(structs: dict, layout: dict) -> list:
    """Every disagreement between the Structures of a struct map and a `header_layout`, one line each, `struct` or `struct.field` first."""
    bad = []
    for cname, S in structs.items():
        if (C.sizeof(S),) != layout[cname]:
            bad.append(f"{cname}: sizeof {C.sizeof(S)} against the header's {layout[cname][0]}")
        for f, *_ in S._fields_:
            have = (getattr(S, f).offset, getattr(S, f).size)
            if have != layout[f"{cname}.{f}"]:
                bad.append(f"{cname}.{f}: (offset, size) {have} against the header's {layout[f'{cname}.{f}']}")
    return bad


def test_every_structure_has_its_structs_layout_and_a_swapped_pair_is_reported_by_name(tmp_path):
    layout = header_layout(STRUCTS, tmp_path)
    assert len(layout) == len(STRUCTS) + sum(len(S._fields_) for S in STRUCTS.values()) == 9 + 121
    assert layout_mismatches(STRUCTS, layout) == []

    fields = list(engine.Curriculum._fields_)
    i, j = (next(k for k, f in enumerate(fields) if f[0] == name) for name in ("tol_lin", "tol_yaw"))      # two floats, side by side
    fields[i], fields[j] = fields[j], fields[i]
    swapped = type("Curriculum", (C.Structure,), {"_fields_": fields})
    assert C.sizeof(swapped) == C.sizeof(engine.Curriculum)
    bad = layout_mismatches({**STRUCTS, "odk_curriculum": swapped}, layout)
    assert sorted(line.split(":")[0] for line in bad) == ["odk_curriculum.tol_lin", "odk_curriculum.tol_yaw"], bad
