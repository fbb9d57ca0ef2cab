#!/usr/bin/env python3
"""Times the depth rasteriser (lc_amd.render.render_depth) on the GPU and writes profiles/render/bench_render.json.

    python scripts/bench_render.py [--iters 200] [--warmup 20] [--out profiles/render/bench_render.json]

Every shape is captured in a graph after a warm-up and replayed; a time is the median over `--iters` replays timed one by one with
device events (p10 / p90 beside it).  Shapes: B = 32 at 64x64 and 128x128 with a 20 480-face and a 327 680-face icosphere (the
subdivisions nearest to 20 k and 200 k faces), B = 1 at 480x640 with the 20 480-face icosphere and with a 12-face box that fills
the frame (every tile holds faces far larger than itself: the whole-wave path).

The two launches are timed separately from a kernel trace, in runs of their own: per shape one child process under
`rocprofv3 --kernel-trace --stats` (tracing off in the timed replays above) renders the shape `--trace-calls` times, and `setup_us` /
`raster_us` are the trace's average durations of lc_render_setup_kernel / lc_render_raster_kernel.  `large_tile_share` is the share of
(row, tile) pairs in which some face's box covers more than 64 samples (the whole-wave path), counted on the host -- a count of tiles, NOT
a share of time, which is not measured.  `record_GBps` is the record
bytes the raster launch has to read (tiles x faces x 16 bytes, plus 48 more for every face whose box meets the tile -- counted on the
host from the oracle's projection) over raster_us, against the 8 TB/s of HBM; the records of a row are shared by its tiles, so most
of those reads are cache hits and the figure is a rate of requests, not of HBM traffic.
Needs the GPU; there is no CPU fallback.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import render  # noqa: E402
from tests import render_cases as rc  # noqa: E402
from tests import render_oracle as ro  # noqa: E402

LABEL_STEP_US = 92.0  # README.md: the label step at zlmo's shape (B = 32, 128x128), which a render now precedes


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
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def record_bytes(v, f, R, t, K, size):
    """Bytes of face records the raster launch requests for one row: 16 per (tile, face), 48 more where the face's box meets the tile."""
    H, W = size
    z, s, _ = ro.project(v, R, t, K)
    ok = (z[f] > rc.NEAR).all(1)
    sx, sy = s[f][..., 0], s[f][..., 1]
    x0, x1 = np.ceil((sx.min(1) - 128) / 256), np.floor((sx.max(1) - 128) / 256)
    y0, y1 = np.ceil((sy.min(1) - 128) / 256), np.floor((sy.max(1) - 128) / 256)
    x0, x1, y0, y1 = np.maximum(x0, 0), np.minimum(x1, W - 1), np.maximum(y0, 0), np.minimum(y1, H - 1)
    live = ok & (x0 <= x1) & (y0 <= y1)
    tiles = (-(-H // 32)) * (-(-W // 32))
    met = np.where(live, (x1 // 32 - x0 // 32 + 1) * (y1 // 32 - y0 // 32 + 1), 0).sum()
    big = np.zeros((-(-H // 32), -(-W // 32)), dtype=bool)
    for k in np.nonzero(live & ((x1 - x0 + 1) * (y1 - y0 + 1) > 64))[0]:  # only a box of more than 64 samples can have them in one tile
        for ty in range(int(y0[k]) // 32, int(y1[k]) // 32 + 1):
            for tx in range(int(x0[k]) // 32, int(x1[k]) // 32 + 1):
                w = min(x1[k], tx * 32 + 31) - max(x0[k], tx * 32) + 1
                h = min(y1[k], ty * 32 + 31) - max(y0[k], ty * 32) + 1
                big[ty, tx] |= w * h > 64
    return int(tiles * len(f) * 16 + met * 48), int(big.sum()), int(tiles)


def make_shape(i, dev):
    """(MeshSet, idx, R, t, K on the device; host copies) of shape i, from a fixed seed."""
    name, B, size = SHAPES[i]
    v, f = MESH_MAKERS[name]()
    ms = render.MeshSet([(v, f)], dev)
    rng = np.random.default_rng(100 + i)
    K = rc.camera(size)
    R = np.stack([rc.rot(rng.normal(size=3), rng.uniform(0, 180)) for _ in range(B)])
    t = np.stack([np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.35, 0.6)], dtype=np.float32) for _ in range(B)])
    if name == "box12":
        t[:, 2] = 0.75
    dv = (ms, ms.index_of([0] * B), torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(np.stack([K] * B)).to(dev))
    return (v, f, R, t, K), dv


def traced_kernels(i, calls):
    """Average durations (us) of the two kernels of shape i from a rocprofv3 kernel trace of a fresh child process."""
    with tempfile.TemporaryDirectory(prefix="lc_render_trace_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--one-shape", str(i), "--trace-calls", str(calls)]
        subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                for key in ("setup", "raster"):
                    if f"lc_render_{key}_kernel" in r["Name"]:
                        out[key] = float(r["AverageNs"]) * 1e-3
    if set(out) != {"setup", "raster"}:
        raise RuntimeError(f"bench_render: the kernel trace of shape {i} names {sorted(out)}")
    return out


MESH_MAKERS = {"ico20k": lambda: rc.icosphere(5, 0.1), "ico328k": lambda: rc.icosphere(7, 0.1), "box12": lambda: rc.box((0.6, 0.5, 0.4))}
SHAPES = [("ico20k", 32, (64, 64)), ("ico20k", 32, (128, 128)), ("ico328k", 32, (64, 64)), ("ico328k", 32, (128, 128)),
          ("ico20k", 1, (480, 640)), ("box12", 1, (480, 640))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render", "bench_render.json"))
    ap.add_argument("--trace-calls", type=int, default=50)
    ap.add_argument("--one-shape", type=int, default=None, help="render one shape --trace-calls times and exit (the traced child)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: needs the GPU")
    dev = torch.device("cuda:0")
    if args.one_shape is not None:
        _, (ms, idx, Rd, td, Kd) = make_shape(args.one_shape, dev)
        for _ in range(args.trace_calls):
            render.render_depth(ms, idx, Rd, td, Kd, SHAPES[args.one_shape][2], near=rc.NEAR, far=rc.FAR, want_homo=True)
        torch.cuda.synchronize()
        return
    rows = []
    for i, (name, B, size) in enumerate(SHAPES):
        (v, f, R, t, K), (ms, idx, Rd, td, Kd) = make_shape(i, dev)
        total = timed(lambda: render.render_depth(ms, idx, Rd, td, Kd, size, near=rc.NEAR, far=rc.FAR, want_homo=True), args.iters, args.warmup)
        out = render.render_depth(ms, idx, Rd, td, Kd, size, near=rc.NEAR, far=rc.FAR)
        hit_share = float(out.mask.float().mean())
        torch.cuda.synchronize()
        kern = traced_kernels(i, args.trace_calls)
        counts = [record_bytes(v, f, R[b], t[b], K, size) for b in range(B)]
        nbytes, big_tiles, tiles = (sum(c[k] for c in counts) for k in range(3))
        rows.append(dict(mesh=name, faces=int(len(f)), B=B, size=list(size), total=total, setup_us=kern["setup"], raster_us=kern["raster"],
                         record_bytes=nbytes, record_GBps=nbytes / kern["raster"] * 1e-3, share_of_8TBps=nbytes / kern["raster"] * 1e-3 / 8000.0,
                         large_tile_share=big_tiles / tiles, hit_share=hit_share, vs_label_step=total["median_us"] / LABEL_STEP_US))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, label_step_us=LABEL_STEP_US, shapes=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
