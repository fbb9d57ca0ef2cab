#!/usr/bin/env python3
"""Times the symmetry deviation (lc_amd.symfind.deviation) on the GPU beside the diameter kernel of lc_amd.models, and the two tools of
`python -m lc_amd.prep_models` end to end, and writes profiles/symfind/bench_symfind.json.

    python scripts/bench_symfind.py [--out profiles/symfind/bench_symfind.json] [--quick]

Kernel rows: one mesh of V = 5 000 and 40 000 vertices (a seeded Gaussian cloud: the work does not depend on the values), K = 384 rows (the
identity and 383 turns about z), with every vertex as a query and with 1024 queries.  `device_us` is the call captured in a graph after a
warm-up and replayed, device events around ONE replay, median over the replays (p10 / p90 beside it): the three launches of a call and the
gaps between them, not a per-kernel trace.  `pairs_per_s` = K x queries x V over it.  Beside each V, IN THE SAME SESSION, the diameter of
`lc_amd.models.prepare(want_extents=False)` on the same mesh the same way: its pairs are V (V - 1) / 2.
Tool rows: a host clock around `prep_models.main` (reading the .ply files, the device calls, the host rules, writing the JSON) on a
directory of three meshes of 5 000 vertices -- a cuboid's surface, a surface of revolution and a cloud.
Needs the GPU; there is no CPU fallback.
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import models, prep_models, symfind  # noqa: E402
from lc_amd.render import MeshSet  # noqa: E402

FACES0 = np.zeros((0, 3), np.int32)


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)), n=int(len(ts)))


def timed(fn, iters, warmup=2):
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
    return stats(dev)


def write_ply(path, v):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n"
                "property list uchar int vertex_indices\nend_header\n")
        f.writelines(f"{float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in v)


def tool_meshes(V, rng):
    u = rng.uniform(-1, 1, (V, 3))
    u[np.arange(V), rng.integers(0, 3, V)] = rng.choice([-1.0, 1.0], V)
    phi, h = rng.uniform(0, 2 * math.pi, V), rng.uniform(-1, 1, V)
    r = 20.0 + 15.0 * np.cos(1.3 * h)
    return [u * (30.0, 45.0, 65.0), np.stack([r * np.cos(phi), r * np.sin(phi), 50.0 * h], -1), rng.standard_normal((V, 3)) * (20.0, 35.0, 55.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symfind", "bench_symfind.json"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the vertices: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_symfind: needs the GPU")
    dev = torch.device("cuda:0")
    K = 384
    table = np.stack([symfind.turn_row(np.eye(3)[2], np.zeros(3), 2.0 * math.pi * s / K) for s in range(K)])
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    rows = []
    for V, iters in ((5000, 30), (40000, 8)):
        if args.quick:
            V //= 10
        rng = np.random.default_rng(V)
        ms = MeshSet([((rng.standard_normal((V, 3)) * (20.0, 45.0, 70.0)).astype(np.float32), FACES0)], dev)
        diam = timed(lambda: models.prepare(ms, 0, want_extents=False), iters)
        rows.append(dict(kernel="models diameter", verts=V, pairs=V * (V - 1) // 2, device_us=diam, pairs_per_s=V * (V - 1) / 2 / (diam["median_us"] * 1e-6)))
        print(json.dumps(rows[-1]), flush=True)
        tab, jobs = torch.from_numpy(table).to(dev), [as_dev([0]), as_dev([0]), as_dev([K])]
        for nq in (V, min(1024, V)):
            q = [] if nq == V else [as_dev(rng.permutation(V)[:nq]), as_dev([0]), as_dev([nq])]
            kw = dict(max_k=K) if nq == V else dict(max_k=K, max_queries=nq)
            t = timed(lambda: symfind.deviation(ms, tab, *jobs, *q, **kw), iters)
            rows.append(dict(kernel="symfind deviation", verts=V, rows=K, queries=nq, all_vertices=nq == V, pairs=K * nq * V, device_us=t,
                             pairs_per_s=K * nq * V / (t["median_us"] * 1e-6), over_diameter_rate=K * nq * V / (t["median_us"] * 1e-6) / rows[-1 if nq == V else -2]["pairs_per_s"]))
            print(json.dumps(rows[-1]), flush=True)
    V = 500 if args.quick else 5000
    tools = []
    with tempfile.TemporaryDirectory() as d:
        for k, v in enumerate(tool_meshes(V, np.random.default_rng(7))):
            write_ply(os.path.join(d, f"obj_{k + 1:06d}.ply"), v.astype(np.float32))
        for name, argv in (("--symmetries (1024 queries, obox frame)", ["--fps", "0", "--symmetries", "--force"]),
                           ("--check-symmetries (every vertex)", ["--check-symmetries"])):
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    rc = prep_models.main([d] + argv)
                ts.append(time.perf_counter() - t0)
            info = json.load(open(os.path.join(d, "models_info.json")))
            tools.append(dict(tool=name, meshes=3, verts_per_mesh=V, exit_code=rc, wall_s=[round(t, 4) for t in ts], wall_s_last=ts[-1],
                              proposed={k: [len(e.get("symmetries_discrete", ())), len(e.get("symmetries_continuous", ()))] for k, e in info.items()}))
            print(json.dumps(tools[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), quick=bool(args.quick), tile=symfind.TILE, queries_per_workgroup=symfind.QUERIES, rows=rows, tools=tools,
               not_measured="per-kernel times from a trace; occupancy and VALU utilisation counters")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
