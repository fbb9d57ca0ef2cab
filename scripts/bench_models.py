#!/usr/bin/env python3
"""Times the model preparation (lc_amd.models.prepare) on the GPU and writes profiles/models/bench_models.json.

    python scripts/bench_models.py [--out profiles/models/bench_models.json] [--quick]

Shapes: one mesh and 21 meshes (YCB-V's object count) of V = 5 000, 40 000 and 250 000 vertices each (seeded Gaussian clouds: neither
the diameter's pair walk nor the selection's passes depend on the values), fps_count = 256.  Three parts are timed on their own:
`diameter` (extents off, no farthest points), `fps` (extents + 256 farthest points, no diameter) and `all`.

Two figures per part, named for what they are:
  * `device_us`: the part captured in a graph after a warm-up and replayed; device events around ONE replay, median over the replays
    (p10 / p90 beside it).  It is the kernels of the part plus the gaps between its two or three launches -- not a per-kernel trace.
  * `call_us`: a host clock around the eager `prepare(...)` followed by a device synchronise, median: allocation of the outputs and the
    workspace, the argument checks, the launches and the kernels.
`pairs_per_s` is V (V - 1) / 2 pairs per mesh over the diameter's device time; `picks_per_s` the 256 picks of a mesh over the
selection's device time (the meshes of a set are selected side by side, one workgroup each).
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

from lc_amd import models  # noqa: E402
from lc_amd.render import MeshSet  # noqa: E402

FPS = 256
FACES0 = np.zeros((0, 3), np.int32)
PARTS = {"diameter": dict(fps_count=0, want_diameter=True, want_extents=False),
         "fps": dict(fps_count=FPS, want_diameter=False, want_extents=True),
         "all": dict(fps_count=FPS, want_diameter=True, want_extents=True)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "models", "bench_models.json"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the vertices: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_models: needs the GPU")
    dev = torch.device("cuda:0")
    rows = []
    for V, iters in ((5000, 100), (40000, 40), (250000, 20)):
        if args.quick:
            V //= 10
        for n in (1, 21):
            rng = np.random.default_rng(V + n)
            ms = MeshSet([((rng.standard_normal((V, 3)) * 0.05).astype(np.float32), FACES0) for _ in range(n)], dev)
            for part, kw in PARTS.items():
                device, call = timed(lambda: models.prepare(ms, **kw), iters, 2)
                row = dict(meshes=n, verts_per_mesh=V, part=part, fps_count=kw["fps_count"], device_us=device, call_us=call,
                           workspace_bytes=models.workspace_bytes(n, V, kw["fps_count"]))
                if part == "diameter":
                    row["pairs_per_s"] = n * V * (V - 1) / 2 / (device["median_us"] * 1e-6)
                if part == "fps":
                    row["picks_per_s"] = FPS / (device["median_us"] * 1e-6)
                    row["form"] = "resident" if V <= models.FPS_RESIDENT else "streaming"
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), quick=bool(args.quick), fps_count=FPS, diam_tile=models.DIAM_TILE, fps_resident=models.FPS_RESIDENT,
               rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
