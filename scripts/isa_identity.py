#!/usr/bin/env python3
"""Is the device code of two trees the same?  The proof a refactor of the kernels' sources rests on: the gfx950 assembly of every
translation unit of every library (lc_amd/build.py: TARGETS, LATER_TARGETS and EXTRA_TARGETS), compiled from each tree, compared by hash.  Needs hipcc, no GPU.

    python scripts/isa_identity.py BEFORE AFTER [> profiles/<topic>/isa_identity.txt]

Each .hip of THIS tree's targets is compiled at the same relative path from the root of either tree (e.g. the parent commit as a
git worktree) with

    hipcc --cuda-device-only -S <build.COMMON_FLAGS> -D<the target's hash macro>="isa-identity" <build.PER_FILE_FLAGS of the file> FILE

and the lines containing __hip_cuid_ are dropped (the symbol changes with the file's path and the macro's value).  One line per unit:
file, lines compared, sha256 of BEFORE's assembly, sha256 of AFTER's, verdict.  Exit status 1 when any unit differs or is missing.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lc_amd import build  # noqa: E402


def device_asm(tree: str, rel: str, macro: str):
    """The unit's device assembly without its __hip_cuid_ lines, or None when the tree has no such file or it does not compile."""
    if not os.path.exists(os.path.join(tree, rel)):
        return None
    cmd = [build._hipcc(), "--cuda-device-only", "-S", *build.COMMON_FLAGS, f'-D{macro}="isa-identity"',
           *build.PER_FILE_FLAGS.get(os.path.basename(rel), []), rel, "-o", "-"]
    run = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    if run.returncode:
        sys.stderr.write(run.stderr)
        return None
    return [ln for ln in run.stdout.splitlines() if "__hip_cuid_" not in ln]


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    before, after = (os.path.abspath(a) for a in argv[1:])
    units = [(os.path.relpath(src, ROOT), t.hash_marker.decode().rstrip(":")) for t in build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS for src in build.sources(t)]
    units.sort()

    def one(unit):
        return [device_asm(tree, *unit) for tree in (before, after)]

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(one, units))
    same = 0
    for (rel, _), (a, b) in zip(units, results):
        sha = ["-" * 64 if x is None else hashlib.sha256("\n".join(x).encode()).hexdigest() for x in (a, b)]
        ok = a is not None and a == b
        same += ok
        print(f"{rel}  {len(b or a or [])}  {sha[0]}  {sha[1]}  {'identical' if ok else 'DIFFERENT'}")
    print(f"{same} of {len(units)} units identical")
    return 0 if same == len(units) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
