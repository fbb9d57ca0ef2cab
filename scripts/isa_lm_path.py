#!/usr/bin/env python3
"""Instruction classes along ONE path through the LM loop of a pose-unit kernel's assembly: from the line after the totals' last ds_read of the
candidate evaluation, round the loop, to the v_rsq_f64 of the next make_rot.  The path is stated, not guessed: every conditional branch met
takes the next letter of DECISIONS (T = taken, N = falls through), unconditional branches are followed, and each one is printed with its line
so that the walk can be checked against the listing.
    python scripts/isa_lm_path.py FILE.s START_LINE DECISIONS          (profiles/lmstep/NOTES.md has the two walks on record)
A fourth argument replaces the instruction the walk stops at (a prefix of its mnemonic).  With s_memtime and the assembly of a -DLC_STAMPS
build, a walk from the line behind one stamp runs to the next stamp: ONE PHASE, make_rot or the LDL^T, as the stamps delimit it (they are
scheduling barriers, so nothing of a neighbouring phase is interleaved; the stamp's own s_waitcnt is the first line to start behind).
    python scripts/isa_lm_path.py FILE.s START_LINE DECISIONS s_memtime  (profiles/makerot/NOTES.md)"""
import re
import sys

path, start, decisions = sys.argv[1], int(sys.argv[2]), sys.argv[3]
stop = sys.argv[4] if len(sys.argv) > 4 else "v_rsq_f64"
lines = open(path).read().split("\n")
labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
CLASSES = ["fp64 arithmetic", "  of it: v_max x, x (canonicalise)", "  of it: v_max / v_min", "v_mov / v_cndmask", "v_cmp + SALU mask work", "branches", "  of them taken",
           "waits and nops", "transcendental", "other"]
count = dict.fromkeys(CLASSES, 0)
i, d, total = start - 1, 0, 0
while True:
    l = lines[i]
    i += 1
    if not l.startswith("\t") or l.strip().startswith((";", ".")):
        continue
    op, *rest = l.split(None, 1)
    args = rest[0] if rest else ""
    if op.startswith(stop):
        break
    total += 1
    if op in ("s_branch",) or op.startswith("s_cbranch"):
        count["branches"] += 1
        take = True if op == "s_branch" else decisions[d] == "T"
        if op != "s_branch":
            d += 1
        print(f"  line {i}: {op} {args} -> {'taken' if take else 'falls through'}")
        if take:
            count["  of them taken"] += 1
            i = labels[args.strip()]
    elif op in ("s_waitcnt", "s_nop"):
        count["waits and nops"] += 1
    elif op.startswith(("v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")):
        count["transcendental"] += 1
    elif re.match(r"v_(add|mul|fma|fmac|max|min|div_\w+)_f64", op):
        count["fp64 arithmetic"] += 1
        if op.startswith(("v_max", "v_min")):
            a = [x.strip() for x in args.split(",")]
            count["  of it: v_max x, x (canonicalise)" if len(a) == 3 and a[1] == a[2] else "  of it: v_max / v_min"] += 1
    elif op.startswith(("v_mov", "v_cndmask")):
        count["v_mov / v_cndmask"] += 1
    elif op.startswith(("v_cmp", "s_")):
        count["v_cmp + SALU mask work"] += 1
    else:
        count["other"] += 1
print(f"decisions used {d} of {len(decisions)}; stopped at line {i} ({lines[i - 1].strip()})")
for c in CLASSES:
    print(f"{c:40s} {count[c]:4d}")
print(f"{'all':40s} {total:4d}")
