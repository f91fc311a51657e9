"""Static census of the VALU instructions that do no arithmetic, per phase of step_kernel<Shape, 32, 0> (CPU only):
    python tools/isa_overhead_census.py [A|B|C|D|E] [--listing odk_env_A.s] [--json]
Without --listing the shape's kernel set is compiled with -DODK_MARK (phase markers as comments in the ISA, as tools/isa_phase_stats.py does).
Per phase ("after <marker>"): all VALU, v_cndmask_b32, v_mov_b32_e32 split by source (immediate / VGPR / SGPR), v_mov_b32_dpp, s_nop, and
  unfused  v_mov_b32_dpp whose every reader is a plain (non-DPP) add / fmac / fma: a cross-lane read the compiler could not fold into its
           consumer -- two instructions where one v_add_f32_dpp would do (the final stage of a row reduction sunk under a branch);
  unf_rm   the row_mirror ones among them (the last butterfly stage).
Readers are found by a linear scan from the move to the next write of its destination (at most SCAN lines, across labels: a listing
has no control-flow graph; the classes this tool reports sit in straight-line code or directly in front of the branch they were sunk under)."""
import collections, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = 600
KEYS = {"A": "ILi21ELi20E", "B": "ILi31ELi30E", "C": "ILi22ELi21E", "D": "ILi19ELi18E", "E": "ILi23ELi22E"}
COLS = ("valu", "cndmask", "mov", "mov_imm", "mov_vgpr", "mov_sgpr", "mov_dpp", "unfused", "unf_rm", "s_nop")
ENGINE_FLAGS = ["-fno-slp-vectorize", "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-load-store-vectorizer=0"]


def compile_listing(shape, out):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *ENGINE_FLAGS, "-DODK_MARK", f"-DODK_ENV_SET={shape}",
                           "-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "open_duck_playground_amd/csrc/odk_env_unit.hip")], stderr=subprocess.DEVNULL)
    return out


def _vregs(operand):
    """VGPR numbers an operand names: v12 -> {12}, v[12:15] -> {12..15}; anything else -> {}"""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _parse(line):
    """(opcode, [operands], trailing modifiers) of an instruction line, or None"""
    if not line.startswith("\t") or line.startswith("\t.") or line.startswith("\t;"):
        return None
    code = line.split(";")[0].strip()
    if not code:
        return None
    op, _, rest = code.partition(" ")
    parts = [p.strip() for p in rest.split(",")] if rest.strip() else []
    ops, mods = [], ""
    for i, p in enumerate(parts):
        first, _, tail = p.partition(" ")
        ops.append(first)
        if tail and i == len(parts) - 1:
            mods = tail
    return op, ops, mods


_NO_DST = ("v_cmp", "v_nop", "ds_write", "ds_store", "global_store", "buffer_store", "scratch_store", "s_", "v_readlane", "v_readfirstlane", "v_cmpx")


def _writes(op, ops):
    if not ops or op.startswith(_NO_DST):
        return set()
    w = _vregs(ops[0])
    if op.startswith(("v_permlane", "v_swap")) and len(ops) > 1:     # both operands are written
        w |= _vregs(ops[1])
    return w


def _reads(op, ops):
    src = ops if op.startswith(_NO_DST) else ops[1:]
    r = set()
    for o in src:
        r |= _vregs(o)
    if op.startswith(("v_fmac", "v_mac", "v_permlane", "v_swap")) and ops:      # the destination is a source too
        r |= _vregs(ops[0])
    return r


def _plain_sum(op, mods):
    return op.startswith(("v_add_f32", "v_fmac_f32", "v_fma_f32", "v_pk_add_f32", "v_pk_fma_f32")) and "dpp" not in op and "row_" not in mods and "quad_perm" not in mods


def census(listing, shape="A", lanes=32, hf=0):
    """{phase: Counter} of step_kernel<Shape, lanes, hf> in `listing`, phases in listing order"""
    lines = open(listing).read().split("\n")
    tag = f"Li{lanes}ELi{hf}E"
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z11step_kernel") and KEYS[shape] in l and tag in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    parsed = [_parse(l) for l in body]
    stats = collections.OrderedDict()
    phase = "pre"
    for i, l in enumerate(body):
        m = re.search(r"; ODK_PHASE_(END|BEGIN)\s*(\d*)", l)
        if m:
            phase = "after " + (m.group(2) or "begin")
            continue
        if parsed[i] is None:
            continue
        op, ops, mods = parsed[i]
        d = stats.setdefault(phase, collections.Counter())
        if op == "s_nop":
            d["s_nop"] += 1
        if not op.startswith("v_"):
            continue
        d["valu"] += 1
        if op.startswith("v_cndmask_b32"):
            d["cndmask"] += 1
        elif op == "v_mov_b32_e32":
            d["mov"] += 1
            s = ops[1] if len(ops) > 1 else ""
            d["mov_vgpr" if _vregs(s) else "mov_sgpr" if re.match(r"(s\d|s\[|vcc|exec|ttmp|m0)", s) else "mov_imm"] += 1
        elif op == "v_mov_b32_dpp":
            d["mov_dpp"] += 1
            dst = _vregs(ops[0])
            readers = []
            for j in range(i + 1, min(i + 1 + SCAN, len(body))):
                if parsed[j] is None:
                    continue
                o2, p2, m2 = parsed[j]
                if _reads(o2, p2) & dst:
                    readers.append((o2, m2))
                if _writes(o2, p2) & dst:
                    break
            if readers and all(_plain_sum(o2, m2) for o2, m2 in readers):
                d["unfused"] += 1
                if "row_mirror" in mods:
                    d["unf_rm"] += 1
    return stats


def main(argv):
    shape = next((a for a in argv if a in KEYS), "A")
    listing = argv[argv.index("--listing") + 1] if "--listing" in argv else compile_listing(shape, os.path.join(tempfile.gettempdir(), f"odk_census_{shape}.s"))
    stats = census(listing, shape)
    if "--json" in argv:
        print(json.dumps({k: dict(v) for k, v in stats.items()}))
        return
    print(f"{'region':12s} " + " ".join(f"{c:>8s}" for c in COLS))
    tot = collections.Counter()
    for k, d in stats.items():
        tot.update(d)
        print(f"{k:12s} " + " ".join(f"{d[c]:8d}" for c in COLS))
    print(f"{'total':12s} " + " ".join(f"{tot[c]:8d}" for c in COLS))
    sub = collections.Counter()
    for k, d in stats.items():
        if k not in ("pre",) and k != list(stats)[-1]:
            sub.update(d)
    print(f"{'substep':12s} " + " ".join(f"{sub[c]:8d}" for c in COLS) + "   (markers begin .. last: one substep, static)")


if __name__ == "__main__":
    main(sys.argv[1:])
