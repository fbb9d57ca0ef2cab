#!/usr/bin/env python3
"""Times the crop geometry drawn on the device (lc_amd.geometry.zoom_geometry) and the chained training input behind it
(lc_amd.train_inputs.train_inputs) beside the route they replace, and writes profiles/geometry/bench_geometry.json.

    python scripts/bench_geometry.py [--iters 200] [--warmup 20] [--host-iters 20] [--out profiles/geometry/bench_geometry.json]

Shapes: 32 and 64 rows over four 480 x 640 frames, a 256 x 256 input, 128 x 128 and 64 x 64 outputs, 256 check points, eight backgrounds,
float32 output with `normalize`.  Per case, one fresh draw per step:

  zoom         a captured graph of `zoom_geometry` alone.  Median over `--iters` replays timed one by one with device events (p10 / p90
               beside it).
  chain        a captured graph of `seed_word.add_(1)` and `train_inputs`: every replay redraws geometry, check points and colours.
  host_route   what a step cost before: `zoom_geometry_host` (wall clock, median of `--host-iters`), the copies of its arrays and of the
               seed into the captured buffers (wall clock, with the wait for them), and a replay of the same chain reading those buffers
               (device events).  `total_us` is their sum.

Before anything is timed the script confirms that the twelve libraries of `build.TARGETS` before geometry are built from the sources recorded in
profiles/geometry/source_hashes_of_the_twelve.json (the geometry library changes none of them), and that the chain's outputs at a seed
EQUAL the host route's at that seed; it stops otherwise.  Needs the GPU; there is no CPU fallback.
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

from lc_amd import augment, build, geometry  # noqa: E402
from lc_amd.train_inputs import train_inputs  # noqa: E402

F, H, W, G = 4, 480, 640, 8
IN_HW = (256, 256)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 20240229
HASHES = os.path.join(ROOT, "profiles", "geometry", "source_hashes_of_the_twelve.json")


def check_the_twelve():
    """The twelve libraries' sources are the recorded ones, and each built library carries that hash."""
    recorded = json.load(open(HASHES))
    twelve = [t for t in build.TARGETS if t is not build.GEOMETRY]
    if sorted(recorded) != sorted(t.name for t in twelve):
        raise SystemExit(f"bench_geometry: {HASHES} does not list the twelve libraries of build.TARGETS before geometry")
    for t in twelve:
        now = build.source_hash(t)
        if now != recorded[t.name]:
            raise SystemExit(f"bench_geometry: the source hash of {t.name} changed: {recorded[t.name]} recorded, {now} now")
        if os.path.exists(t.so_path) and build.embedded_hash(t.so_path, t.hash_marker) != now:
            raise SystemExit(f"bench_geometry: {t.so_path} was built from other sources than the recorded ones")
    return recorded


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def graphed(fn, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    return g, res


def replay_times(g, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return stats(ts)


def same(a, b):
    nan = torch.isnan(b) if b.is_floating_point() else torch.zeros_like(b, dtype=torch.bool)
    return a.dtype == b.dtype and (not b.is_floating_point() or torch.equal(torch.isnan(a), nan)) and torch.equal(a[~nan], b[~nan])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry", "bench_geometry.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry: needs the GPU")
    hashes = check_the_twelve()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    cfg = augment.AugmentConfig(use_peper_salt=True, use_motion_blur=True, use_invert=True, rotate_prob=0.5)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    masks_h = np.zeros((F, H, W), dtype=np.uint8)
    for f in range(F):
        masks_h[f, 100 + 20 * f:340 - 10 * f, 150 + 30 * f:470 + 10 * f] = 1
    masks = torch.from_numpy(masks_h).to(dev)
    bg = torch.from_numpy(rng.integers(0, 256, (G, 3) + IN_HW, dtype=np.uint8)).to(dev)
    K_h = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)
    K = torch.from_numpy(K_h).to(dev)
    rows = []
    for B in (32, 64):
        ids_h = np.arange(B, dtype=np.int32) * 3 - 7
        x1, y1 = rng.uniform(120, 300, B), rng.uniform(80, 200, B)
        box_h = np.stack((x1, y1, x1 + rng.uniform(60, 220, B), y1 + rng.uniform(60, 200, B)), axis=1).astype(np.float32)
        fidx = torch.from_numpy((np.arange(B) % F).astype(np.int32)).to(dev)
        sid, box = torch.from_numpy(ids_h).to(dev), torch.from_numpy(box_h).to(dev)
        for out_hw in ((128, 128), (64, 64)):
            in_wh, out_wh = IN_HW[::-1], out_hw[::-1]
            kw = dict(masks=masks, mask_index=fidx, bbox_xyxy=box, cam_K=K, sample_id=sid, cfg=cfg, backgrounds=bg, in_hw=IN_HW, out_hw=out_hw, valid_th=100,
                      n_check=256, normalize=(MEAN, STD))
            word = torch.full((1,), SEED, dtype=torch.int64, device=dev)

            def upload(seed, into=None):
                """`zoom_geometry_host` at `seed`, as device tensors: new ones, or copied into the captured buffers."""
                h = geometry.zoom_geometry_host(cfg, seed, ids_h, box_h, (H, W), K_h, in_wh, out_wh)
                arrays = [torch.from_numpy(np.ascontiguousarray(a)) for a in h[:6]]
                if into is None:
                    return geometry.ZoomGeometry(*[a.to(dev) for a in arrays], None, None, None, None)
                for dst, src in zip(into[:6], arrays):
                    dst.copy_(src)
                return into

            # the outputs first: the chain against the host route, at two seeds
            for s in (SEED, SEED + 1):
                got = train_inputs(frames, fidx, seed=s, **kw)
                want = train_inputs(frames, fidx, seed=s, geometry=upload(s), **kw)
                torch.cuda.synchronize()
                for name in got:
                    if not same(got[name], want[name]):
                        raise SystemExit(f"bench_geometry: B={B} out={out_hw} seed={s}: {name} of the chain differs from the host route's")
            refused = int((got["info"] != 0).sum())

            g_zoom, _ = graphed(lambda: geometry.zoom_geometry(cfg, seed=word, sample_id=sid, bbox_xyxy=box, im_hw=(H, W), cam_K=K, in_wh=in_wh, out_wh=out_wh),
                                args.warmup)
            zoom = replay_times(g_zoom, args.iters)

            def fresh():
                word.add_(1)
                return train_inputs(frames, fidx, seed=word, **kw)

            g_chain, _ = graphed(fresh, args.warmup)
            chain = replay_times(g_chain, args.iters)

            bufs = upload(SEED)
            g_host, _ = graphed(lambda: train_inputs(frames, fidx, seed=word, geometry=bufs, **kw), args.warmup)
            t_draw, t_copy, t_replay = [], [], []
            for i in range(args.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = geometry.zoom_geometry_host(cfg, SEED + 1 + i, ids_h, box_h, (H, W), K_h, in_wh, out_wh)
                t1 = time.perf_counter()
                for dst, src in zip(bufs[:6], h[:6]):
                    dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
                word.fill_(SEED + 1 + i)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                t_draw.append((t1 - t0) * 1e6)
                t_copy.append((t2 - t1) * 1e6)
                t_replay.append(replay_times(g_host, 1)["median_us"])
            host = dict(draw_wall=stats(t_draw), copy_wall=stats(t_copy), replay=stats(t_replay))
            host["total_us"] = host["draw_wall"]["median_us"] + host["copy_wall"]["median_us"] + host["replay"]["median_us"]
            rows.append(dict(rows=B, out_hw=list(out_hw), refused_rows=refused, zoom=zoom, chain=chain, host_route=host,
                             fresh_step_speedup_vs_host_route=host["total_us"] / chain["median_us"], outputs_equal_to_the_host_route=True))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, host_iters=args.host_iters, frames=[F, H, W], in_hw=list(IN_HW),
               backgrounds=G, n_check=256, source_hashes_of_the_twelve_unchanged=True, source_hashes=hashes, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
