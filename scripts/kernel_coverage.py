#!/usr/bin/env python3
"""Which compiled kernel forms of liblc_amd.so a run actually launched: the library's gfx950 kernel symbols (the `.name` entries
of the code objects' metadata, read as scripts/kernel_resources.py reads them) against the kernel names of every
`*kernel_stats.csv` / `*kernel_trace.csv` below a rocprofv3 output directory.

    rocprofv3 --kernel-trace --stats -M -f csv -d DIR -- python -m pytest -m gpu -q tests/test_gpu_....py
    python scripts/kernel_coverage.py DIR [path/to/liblc_amd.so]      -> launched / never launched, grouped by source file

`-M` keeps the names mangled, so they compare with the symbols as they are.  The source file of a symbol is the .hip translation
unit whose offload bundle holds it (one bundle per unit, linked in sorted order by lc_amd/build.py; a template instantiated from a
header is listed under the unit that instantiated it).
"""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kernel_resources import READELF, _device_elfs, kernel_resources  # noqa: E402


def _elf_names(elf: bytes):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    return [m.group(1).strip().strip("'") for m in re.finditer(r"^\s*\.name:\s*(\S+)\s*$", txt, re.M)]


def kernel_symbols(so_path=None):
    """{mangled kernel name: source file} for every gfx950 kernel in the library."""
    so_path = so_path or os.path.join(ROOT, "lc_amd", "_C", "liblc_amd.so")
    full = set(kernel_resources(so_path))
    elfs = _device_elfs(open(so_path, "rb").read())
    srcs = [os.path.basename(s) for s in sorted(glob.glob(os.path.join(ROOT, "lc_amd", "csrc", "*.hip")))]
    if len(srcs) != len(elfs):  # lc_amd/build.py links the units in sorted order, one bundle each; otherwise name no unit
        srcs = ["?"] * len(elfs)
    out = {}
    for elf, src in zip(elfs, srcs):
        for n in _elf_names(elf):
            if n in full:
                out.setdefault(n, src)
    for n in full - set(out):
        out[n] = "?"
    return out


def launched_names(trace_dir):
    """Mangled kernel names of every dispatch recorded below trace_dir (rocprofv3 csv output, any depth)."""
    got, files = set(), []
    for pat in ("**/*kernel_stats.csv", "**/*kernel_trace.csv"):
        files += glob.glob(os.path.join(trace_dir, pat), recursive=True)
    for path in sorted(set(files)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or row.get("KernelName") or ""
                if name:
                    got.add(name.strip())
    return got, sorted(set(files))


def _base(name: str) -> str:
    # a dispatch name may carry the descriptor's ".kd" suffix; compare on the symbol itself
    return re.sub(r"\.kd$", "", name)


def report(trace_dir, so_path=None):
    syms = kernel_symbols(so_path)
    got, files = launched_names(trace_dir)
    got = {_base(g) for g in got}
    lines = [f"# trace files read: {len(files)}"]
    n_hit = sum(1 for s in syms if s in got)
    lines.append(f"# kernel symbols in the library: {len(syms)}; launched: {n_hit}; never launched: {len(syms) - n_hit}")
    by_src = {}
    for s, src in syms.items():
        by_src.setdefault(src, []).append(s)
    for src in sorted(by_src):
        names = sorted(by_src[src])
        hit = [n for n in names if n in got]
        miss = [n for n in names if n not in got]
        lines.append("")
        lines.append(f"== {src}: {len(hit)} launched, {len(miss)} never launched")
        for n in miss:
            lines.append(f"  NEVER     {n}")
        for n in hit:
            lines.append(f"  launched  {n}")
    other = sorted(g for g in got if g not in syms and ("lc_" in g))
    if other:
        lines.append("")
        lines.append("== launched lc_ kernels that are not in this library")
        lines += [f"  {n}" for n in other]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.stdout.write(report(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None))
