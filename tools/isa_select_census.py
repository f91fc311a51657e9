"""Static census of the selects (v_cndmask_b32) of step_kernel<Shape, 32, 0>, per phase of a -DODK_MARK listing (CPU only):
    python tools/isa_select_census.py [A|B|C|D|E] [--listing odk_env_A.s] [--passes 2.3] [--list] [--json] [--mark-loop-before TEXT]
Regions are those of tools/isa_overhead_census.py ("after <marker>") plus "ls loop": one pass of the line search's bracketing loop, the loop
whose body holds the LS_LOOP_0 / LS_LOOP_1 markers (it is taken OUT of "after 15", so that the regions still sum to the total).  Per select:
  cmp      the instruction that wrote its mask (vcc for the VOP2 form, the SGPR pair of the VOP3 form), found by a linear scan upwards: a
           v_cmp*, an s_and / s_or / ... of two masks, or "?" when the write is not in sight (a mask kept over a branch);
  share    how many selects read that mask before it is written again;
  zero     one side is the constant 0 and the other a register (the compiler swaps the sides freely, so src0 or src1; the 0 / 1.0 weights of the
           line search are two constants and are not counted);
  mulfma   every reader of the result is a multiply or an FMA (scan downwards to the next write of the destination, as
           isa_overhead_census.py does for its moves);
  dup      the compare behind its mask has the same text (opcode and sources) as an earlier compare of the same region that fed a select, and none
           of its source registers was written in between: a duplicated predicate;
  fill     the register operand of a select with a constant on the other side, or either register operand, was last written by a
           `v_mov_b32` of an immediate: a fill that the select then overwrites per lane;
  adj      a VOP2 select whose preceding VALU instruction is a VOP2 select too (s_nop and scalar instructions between them do not count):
           the one stream in which tools/ubench/valu_issue.hip measures a select at four times a plain instruction.
Columns: valu, sel (all selects), vop2 / vop3, cmp_fed (mask straight from a v_cmp), masks (distinct mask writes feeding selects), shared
(selects whose mask feeds more than one), zero, mulfma, zero_mulfma (both: the multiply would produce the zero anyway), adj, dup, fill, then
weight (how often the region runs per env step: 1 for prologue and epilogue, 10 substeps, the loop body 10 x --passes, the measured mean
pass count of tools/gpu_phase_profile.py) and dyn_sel / dyn_valu = weight x static count.
A listing without the LS_LOOP_0 marker is refused; for a listing of a commit that has no marker yet, --mark-loop-before TEXT puts it in
front of the first line of the kernel that contains TEXT (an instruction at the top of the loop body, read from that listing).
The scan is linear -- a listing has no control-flow graph -- so the figures are static: a select inside a block that is skipped at run time
is listed too."""
import collections, json, os, re, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_overhead_census as oc

COLS = ("valu", "sel", "vop2", "vop3", "cmp_fed", "masks", "shared", "zero", "mulfma", "zero_mulfma", "adj", "dup", "fill")
SUBSTEPS = 10
LOOP = "ls loop"
_MULFMA = ("v_mul_f32", "v_fma_f32", "v_fmac_f32", "v_pk_mul_f32", "v_pk_fma_f32", "v_mul_legacy_f32", "v_mad_f32", "v_mac_f32")
UP = 400


def _sregs(operand):
    """SGPR numbers an operand names; vcc is (-1, -2)"""
    if operand in ("vcc", "vcc_lo"):
        return {-1, -2}
    m = re.fullmatch(r"s(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _mask_write(op, ops):
    """SGPRs (or vcc) this instruction writes as a lane mask or scalar result"""
    if not ops:
        return set()
    if op.startswith("v_cmp"):
        return {-1, -2} if op.endswith("_e32") else _sregs(ops[0])
    if op.startswith(("v_add_co", "v_sub_co", "v_subrev_co", "v_addc_co", "v_subb_co", "v_subbrev_co")) and len(ops) > 1:
        return _sregs(ops[1])
    if op.startswith(("v_readlane", "v_readfirstlane", "v_mad_u64_u32", "v_mad_i64_i32", "v_div_scale")):
        return _sregs(ops[0]) | (_sregs(ops[1]) if len(ops) > 1 else set())
    if op.startswith("s_") and not op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_barrier", "s_bitcmp", "s_setpc", "s_endpgm")):
        return _sregs(ops[0])
    return set()


def selects(listing, shape="A", lanes=32, hf=0, mark_before=None):
    """[(region, line number in the function, record)] for every select of step_kernel<shape, lanes, hf>, and {region: VALU count}"""
    lines = open(listing).read().split("\n")
    tag = f"Li{lanes}ELi{hf}E"
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z11step_kernel") and oc.KEYS[shape] in l and tag in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    if mark_before is not None:
        at = next((i for i, l in enumerate(body) if mark_before in l), None)
        if at is None:
            raise SystemExit(f"isa_select_census: no line of the kernel contains {mark_before!r}")
        body.insert(at, "\t; LS_LOOP_0")
    if not any("; LS_LOOP_0" in l for l in body):
        raise SystemExit("isa_select_census: the listing has no LS_LOOP_0 marker (compile with -DODK_MARK at a commit that has ODK_LS_LOOP, or pass --mark-loop-before TEXT)")
    parsed = [oc._parse(l) for l in body]
    # The loop body is not contiguous in a listing (the compiler lays the tail of the body in front of the loop's header), so the region is
    # taken from the compiler's own block annotations: every block "in Loop: Header=<H>" of the loop H whose body holds the LS_LOOP_0
    # marker, and the header block itself (the exit test: a few compares).
    header, cur, label = [None] * len(body), None, None
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            label, cur = m.group(1)[2:], None
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
        if m and (l.startswith(".LBB") or l.startswith("; %bb.")):
            cur = m.group(1)
        if "This Inner Loop Header" in l or "This Loop Header" in l:
            cur = label
        header[i] = cur
    ls_header = next((header[i] for i, l in enumerate(body) if "; LS_LOOP_0" in l), None)
    region, phase = [None] * len(body), "pre"
    for i, l in enumerate(body):
        m = re.search(r"; ODK_PHASE_(END|BEGIN)\s*(\d*)", l)
        if m:
            phase = "after " + (m.group(2) or "begin")
        region[i] = LOOP if ls_header is not None and header[i] == ls_header else phase
    valu = collections.OrderedDict()
    out = []
    prev_valu = None
    fed = {}     # region -> {compare text: line} of the compares that fed a select so far
    for i, pr in enumerate(parsed):
        if pr is None:
            continue
        op, ops, mods = pr
        if not op.startswith("v_"):
            continue
        valu[region[i]] = valu.get(region[i], 0) + 1
        was, prev_valu = prev_valu, op
        if not op.startswith("v_cndmask_b32"):
            continue
        vop2 = op.endswith("_e32")
        mask = {-1, -2} if vop2 else _sregs(ops[3])
        # the write of the mask, upwards
        cmp_op, w = "?", None
        for j in range(i - 1, max(i - UP, -1), -1):
            if parsed[j] is None:
                continue
            o2, p2, _ = parsed[j]
            if _mask_write(o2, p2) & mask:
                cmp_op, w = o2, j
                break
        # the selects that read this mask value: from its write (or from UP lines above) down to the next write
        share = 0
        for j in range((w + 1) if w is not None else max(i - UP, 0), len(body)):
            if parsed[j] is None:
                continue
            o2, p2, _ = parsed[j]
            if o2.startswith("v_cndmask_b32") and (({-1, -2} if o2.endswith("_e32") else _sregs(p2[3])) & mask):
                share += 1
            if j > i and _mask_write(o2, p2) & mask:
                break
            if j > i + oc.SCAN:
                break
        dup = False
        if w is not None and cmp_op.startswith("v_cmp"):
            o2, p2, _ = parsed[w]
            src = p2 if o2.endswith("_e32") else p2[1:]
            text = o2.replace("_e32", "").replace("_e64", "") + " " + ",".join(src)
            seen = fed.setdefault(region[i], {})
            if text in seen and seen[text] != w:
                regs = set().union(*[oc._vregs(x.lstrip("-|").rstrip("|")) for x in src]) if src else set()
                dup = not any(parsed[j] is not None and oc._writes(parsed[j][0], parsed[j][1]) & regs for j in range(seen[text] + 1, w))
            seen[text] = w
        fill = False
        for operand in ops[1:3]:
            regs = oc._vregs(operand)
            for j in range(i - 1, max(i - UP, -1), -1) if regs else ():
                if parsed[j] is not None and oc._writes(parsed[j][0], parsed[j][1]) & regs:
                    o2, p2, _ = parsed[j]
                    fill = fill or (o2 == "v_mov_b32_e32" and not oc._vregs(p2[1]) and not re.match(r"(s\d|s\[|vcc|exec|ttmp|m0)", p2[1]))
                    break
        dst = oc._vregs(ops[0])
        readers = []
        for j in range(i + 1, min(i + 1 + oc.SCAN, len(body))):
            if parsed[j] is None:
                continue
            o2, p2, _ = parsed[j]
            if oc._reads(o2, p2) & dst:
                readers.append(o2)
            if oc._writes(o2, p2) & dst:
                break
        out.append((region[i], i, dict(text=body[i].strip(), vop2=vop2, cmp=cmp_op, cmp_line=w, share=max(share, 1), zero=(ops[1] == "0") != (ops[2] == "0") and bool(oc._vregs(ops[1]) | oc._vregs(ops[2])),
                                       mulfma=bool(readers) and all(r.startswith(_MULFMA) for r in readers),
                                       dup=dup, fill=fill,
                                       adj=vop2 and was is not None and was.startswith("v_cndmask_b32") and was.endswith("_e32"))))
    return out, valu


def census(listing, shape="A", passes=1.0, mark_before=None):
    """{region: {column: count}} in listing order, with weight / dyn_sel / dyn_valu"""
    sel, valu = selects(listing, shape, mark_before=mark_before)
    regions = list(valu)
    stats = collections.OrderedDict((r, collections.Counter(valu=valu[r])) for r in regions)
    masks = collections.defaultdict(set)
    for r, i, s in sel:
        d = stats[r]
        d["sel"] += 1
        d["vop2" if s["vop2"] else "vop3"] += 1
        d["cmp_fed"] += s["cmp"].startswith("v_cmp")
        d["shared"] += s["share"] > 1
        d["zero"] += s["zero"]
        d["mulfma"] += s["mulfma"]
        d["zero_mulfma"] += s["zero"] and s["mulfma"]
        d["adj"] += s["adj"]
        d["dup"] += s["dup"]
        d["fill"] += s["fill"]
        masks[r].add(s["cmp_line"] if s["cmp_line"] is not None else -i)
    for r in regions:
        d = stats[r]
        d["masks"] = len(masks[r])
        d["weight"] = 1 if r in (regions[0], regions[-1]) else SUBSTEPS * passes if r == LOOP else SUBSTEPS
        d["dyn_sel"] = d["weight"] * d["sel"]
        d["dyn_valu"] = d["weight"] * d["valu"]
    return stats


def substep(stats):
    """the columns summed over one substep: every region but the first (prologue) and the last (epilogue), the loop body once"""
    regions = list(stats)
    tot = collections.Counter()
    for r in regions[1:-1]:
        for c in COLS:
            tot[c] += stats[r][c]
    return tot


def main(argv):
    shape = next((a for a in argv if a in oc.KEYS), "A")
    listing = argv[argv.index("--listing") + 1] if "--listing" in argv else oc.compile_listing(shape, os.path.join(tempfile.gettempdir(), f"odk_census_{shape}.s"))
    passes = float(argv[argv.index("--passes") + 1]) if "--passes" in argv else 1.0
    mark_before = argv[argv.index("--mark-loop-before") + 1] if "--mark-loop-before" in argv else None
    stats = census(listing, shape, passes, mark_before)
    if "--json" in argv:
        print(json.dumps({k: dict(v) for k, v in stats.items()}))
        return
    if "--list" in argv:
        for r, i, s in selects(listing, shape, mark_before=mark_before)[0]:
            print(f"{r:12s} {i:6d} {s['cmp']:24s} share {s['share']:2d} {'zero ' if s['zero'] else '     '}{'mulfma ' if s['mulfma'] else '       '}{'adj ' if s['adj'] else '    '}"
                  f"{'dup ' if s['dup'] else '    '}{'fill ' if s['fill'] else '     '}{s['text']}")
        return
    print(f"{'region':12s} " + " ".join(f"{c:>8s}" for c in COLS) + f" {'weight':>8s} {'dyn_sel':>9s} {'dyn_valu':>9s}")
    tot = collections.Counter()
    for k, d in stats.items():
        tot.update({c: d[c] for c in COLS + ("dyn_sel", "dyn_valu")})
        print(f"{k:12s} " + " ".join(f"{d[c]:8d}" for c in COLS) + f" {d['weight']:8.1f} {d['dyn_sel']:9.0f} {d['dyn_valu']:9.0f}")
    print(f"{'total':12s} " + " ".join(f"{tot[c]:8d}" for c in COLS) + f" {'':8s} {tot['dyn_sel']:9.0f} {tot['dyn_valu']:9.0f}")
    sub = substep(stats)
    print(f"{'substep':12s} " + " ".join(f"{sub[c]:8d}" for c in COLS) + "   (one substep, static, the loop body once)")


if __name__ == "__main__":
    main(sys.argv[1:])
