"""How much cover every global load of the substep has before the wait that needs it, in step_kernel<Shape, 32, 0> (CPU only):
    python tools/isa_load_waits.py [A|B|C|D|E] [--listing odk_env_A.s] [--below N] [--json]
Without --listing the shape's kernel set is compiled with -DODK_MARK (phase markers as comments in the ISA, as tools/isa_overhead_census.py does).
For every global_load between the phase markers: the phase ("after <marker>": P2 = after 1, P7 = after 6, the foot-foot cull = after 7,
P8 = after 8, the candidates of P9 = after 9, the line search = after 15), its line in the kernel and in the listing, the instruction, and
the number of ALL and of VALU instructions up to the first `s_waitcnt vmcnt(N)` that covers it.  Vector memory instructions return in
issue order and vmcnt counts loads and stores alike on gfx9, so a wait vmcnt(N) completes every outstanding one except the last N; the
tool keeps that queue in issue order.  A call (s_swappc_b64) counts as a full wait.  --below N prints only loads with fewer than N VALU
instructions of cover.  The scan is linear, across labels: a listing has no control-flow graph, so a load whose wait sits behind a branch
not taken is charged the skipped block's instructions too -- the figures are upper bounds of the cover, which is the safe side here."""
import collections, json, os, re, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_overhead_census import KEYS, compile_listing  # noqa: E402

_VM = ("global_load", "global_store", "global_atomic", "buffer_load", "buffer_store", "buffer_atomic", "scratch_load", "scratch_store", "flat_load", "flat_store", "flat_atomic")


def load_waits(listing, shape="A", lanes=32, hf=0):
    """[{phase, line, listing_line, text, n_all, n_valu, wait}] of the global loads of step_kernel<Shape, lanes, hf>, in issue order
    (n_all / n_valu None: no wait covers the load before the function ends)"""
    lines = open(listing).read().split("\n")
    tag = f"Li{lanes}ELi{hf}E"
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z11step_kernel") and KEYS[shape] in l and tag in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    phase, n_all, n_valu = "pre", 0, 0
    queue, out = [], []        # queue: outstanding vector-memory instructions, oldest first (None: not a load we report)
    for i in range(start, end):
        l = lines[i]
        m = re.search(r"; ODK_PHASE_(END|BEGIN)\s*(\d*)", l)
        if m:
            phase = "after " + (m.group(2) or "begin")
            continue
        if not l.startswith("\t") or l.startswith("\t.") or l.startswith("\t;"):
            continue
        code = l.split(";")[0].strip()
        if not code:
            continue
        op = code.split()[0]
        covered = None
        if op == "s_waitcnt":
            w = re.search(r"vmcnt\((\d+)\)", code)
            if w:
                covered = int(w.group(1))
            elif re.fullmatch(r"s_waitcnt\s+(0|0x0)", code):
                covered = 0
        elif op.startswith("s_swappc"):
            covered = 0
        if covered is not None:
            done, queue = (queue[:len(queue) - covered], queue[len(queue) - covered:]) if covered else (queue, [])
            for rec in done:
                if rec is not None:
                    rec.update(n_all=n_all - rec.pop("_all"), n_valu=n_valu - rec.pop("_valu"), wait=code)
        n_all += 1
        n_valu += op.startswith("v_")
        if op.startswith(_VM):
            rec = None
            if op.startswith("global_load"):
                rec = dict(phase=phase, line=i - start, listing_line=i + 1, text=re.sub(r"\s+", " ", code), n_all=None, n_valu=None, wait=None, _all=n_all, _valu=n_valu)
                out.append(rec)
            queue.append(rec)
    for rec in out:
        rec.pop("_all", None); rec.pop("_valu", None)
    return out


def substep(recs):
    """the loads between the first and the last phase marker: one substep"""
    return [r for r in recs if r["phase"] not in ("pre", "after 17")]


def main(argv):
    shape = next((a for a in argv if a in KEYS), "A")
    listing = argv[argv.index("--listing") + 1] if "--listing" in argv else compile_listing(shape, os.path.join(tempfile.gettempdir(), f"odk_census_{shape}.s"))
    below = int(argv[argv.index("--below") + 1]) if "--below" in argv else None
    recs = substep(load_waits(listing, shape))
    if "--json" in argv:
        print(json.dumps(recs))
        return
    print(f"{'phase':10s} {'line':>6s} {'listing':>7s} {'all':>5s} {'valu':>5s}  instruction -> covering wait")
    per = collections.OrderedDict()
    for r in recs:
        d = per.setdefault(r["phase"], [0, 0, 0])
        d[0] += 1
        d[1] += r["n_valu"] is not None and r["n_valu"] < 20
        d[2] += r["n_valu"] is not None and r["n_valu"] < 5
        if below is not None and (r["n_valu"] is None or r["n_valu"] >= below):
            continue
        na, nv = ("-", "-") if r["n_all"] is None else (r["n_all"], r["n_valu"])
        print(f"{r['phase']:10s} {r['line']:6d} {r['listing_line']:7d} {na:>5} {nv:>5}  {r['text']} -> {r['wait']}")
    print(f"\n{'phase':10s} {'loads':>6s} {'<20 valu':>9s} {'<5 valu':>8s}")
    for k, d in per.items():
        print(f"{k:10s} {d[0]:6d} {d[1]:9d} {d[2]:8d}")
    print(f"{'substep':10s} {sum(d[0] for d in per.values()):6d} {sum(d[1] for d in per.values()):9d} {sum(d[2] for d in per.values()):8d}")


if __name__ == "__main__":
    main(sys.argv[1:])
