#!/usr/bin/env python3
"""Times the oriented model box search (lc_amd.obox.oriented_box) on the GPU and writes profiles/obox/bench_obox.json.

    python scripts/bench_obox.py [--out profiles/obox/bench_obox.json] [--quick]

Shapes: one mesh and 21 meshes (YCB-V's object count) of V = 5 000, 40 000 and 250 000 vertices each (seeded Gaussian clouds, three times as
long as wide and turned off the axes: the work does not depend on the values), the default six refinement levels, in both modes: all
orientations (1419 + 6 x 125 candidates) and about the z axis (10 + 6 x 5).

Two figures per row, named for what they are:
  * `device_us`: the call captured in a graph after a warm-up and replayed; device events around ONE replay, median over the replays
    (p10 / p90 beside it).  It is the 17 launches of a call and the gaps between them -- not a per-kernel trace.
  * `call_us`: a host clock around the eager `oriented_box(...)` followed by a device synchronise, median: allocation of the outputs and the
    workspace, the argument checks, the launches and the kernels.
`cand_verts_per_s` is meshes x V x candidates (every level's, the final pass included) over the device time.
Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import obox  # noqa: E402
from lc_amd.render import MeshSet  # noqa: E402

FACES0 = np.zeros((0, 3), np.int32)
MODES = {"all": None, "about_z": 2}


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)), n=int(len(ts)))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    dev = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    call = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e6)
    return stats(dev), stats(call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obox", "bench_obox.json"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the vertices: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_obox: needs the GPU")
    dev = torch.device("cuda:0")
    turn = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.96, -0.28], [0.0, 0.28, 0.96]])
    rows = []
    for V, iters in ((5000, 50), (40000, 30), (250000, 10)):
        if args.quick:
            V //= 10
        for n in (1, 21):
            rng = np.random.default_rng(V + n)
            ms = MeshSet([(((rng.standard_normal((V, 3)) * (0.02, 0.045, 0.07)) @ turn.T).astype(np.float32), FACES0) for _ in range(n)], dev)
            for mode, axis in MODES.items():
                device, call = timed(lambda: obox.oriented_box(ms, axis=axis), iters, 2)
                _, n0, n1 = obox.delta_table(axis, obox.DEFAULT_LEVELS)
                cands = n0 + obox.DEFAULT_LEVELS * n1 + 1
                box = obox.oriented_box(ms, axis=axis)
                row = dict(meshes=n, verts_per_mesh=V, mode=mode, levels=obox.DEFAULT_LEVELS, candidates=cands, device_us=device, call_us=call,
                           workspace_bytes=obox.workspace_bytes(n, axis), cand_verts_per_s=n * V * cands / (device["median_us"] * 1e-6),
                           volume_over_aabb_mesh0=float(box.volume[0] / box.aabb_volume[0]))
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), quick=bool(args.quick), tile=obox.TILE, split=obox.SPLIT, level0=obox.LEVEL0_COUNT, rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
