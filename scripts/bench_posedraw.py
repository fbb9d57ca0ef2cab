#!/usr/bin/env python3
"""Times the scene poses drawn on the device (lc_amd.posedraw.draw_scene_poses) and the chained synthetic scene behind them
(lc_amd.synthscene.synth_scenes) beside the route they replace, and writes profiles/posedraw/bench_posedraw.json.

    python scripts/bench_posedraw.py [--iters 200] [--warmup 20] [--host-iters 20] [--out profiles/posedraw/bench_posedraw.json]

  draw         a captured graph of `draw_scene_poses` alone at S = 32, M = 8 and at S = 64, M = 64 (a full wave of slots).  Median over
               `--iters` replays timed one by one with device events (p10 / p90 beside it).
  chain        a captured graph of `seed_word.add_(1)` and `synth_scenes` at S = 8, M = 8 on 480 x 640 frames with a 20 480-face
               icosphere: every replay draws, renders, shades and annotates new scenes.
  host_route   what a step costs without the kernel: `draw_scene_poses_host` (wall clock, median of `--host-iters`), the copies of its
               arrays into the captured buffers (wall clock, with the wait for them), and a replay of the same stages reading those
               buffers (`synthscene.render_and_annotate`, device events).  `total_us` is their sum.

Before anything is timed the script confirms that the draw's outputs at a seed EQUAL the host contract's, and the chain's the host
route's; it stops otherwise.  Needs the GPU; there is no CPU fallback.
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

from lc_amd import posedraw, render, shade, synthscene  # noqa: E402

H, W = 480, 640
NEAR, FAR, DELTA = 0.01, 6.5, 0.015
SEED = 20240229
K_H = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)


def icosphere(subdiv, radius):
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, dtype=np.int32)


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


def same_poses(got, want):
    return all(np.array_equal(g.cpu().numpy().view(np.int32), np.ascontiguousarray(w).view(np.int32)) for g, w in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posedraw", "bench_posedraw.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posedraw: needs the GPU")
    dev = torch.device("cuda:0")
    K = torch.from_numpy(K_H).to(dev)
    cfg = posedraw.PoseDrawConfig(z_range=(0.6, 1.4), centre_box=(0.0, 0.0, float(W), float(H)), gap=0.005, near=NEAR)

    # (a) the draw alone
    draws = []
    for S, M, n_meshes in ((32, 8, 8), (64, 64, 8)):
        ids_h = np.arange(S, dtype=np.int32) * 3 - 7
        slots_h = ((np.arange(S)[:, None] * M + np.arange(M)[None]) % n_meshes).astype(np.int32)
        radius_h = np.linspace(0.03, 0.07, n_meshes).astype(np.float32)
        ids, slots, radius = torch.from_numpy(ids_h).to(dev), torch.from_numpy(slots_h).to(dev), torch.from_numpy(radius_h).to(dev)
        word = torch.full((1,), SEED, dtype=torch.int64, device=dev)
        want = posedraw.draw_scene_poses_host(cfg, SEED, ids_h, slots_h, radius_h, K_H)
        got = posedraw.draw_scene_poses(cfg, seed=word, scene_id=ids, mesh_index=slots, radius=radius, cam_K=K)
        torch.cuda.synchronize()
        if not same_poses(got, want):
            raise SystemExit(f"bench_posedraw: S={S} M={M}: the draw differs from the host contract")
        g, _ = graphed(lambda: posedraw.draw_scene_poses(cfg, seed=word, scene_id=ids, mesh_index=slots, radius=radius, cam_K=K), args.warmup)
        draws.append(dict(S=S, M=M, placed=int((want.info == 0).sum()), no_room=int((want.info == -1).sum()), mean_tries=float(want.tries[want.info == 0].mean()),
                          draw=replay_times(g, args.iters), outputs_equal_to_the_host_contract=True))
        print(json.dumps(draws[-1]), flush=True)

    # (b) the chain per fresh step, and (c) the route it replaces
    S, M = 8, 8
    mesh = icosphere(5, 0.06)  # 20 480 faces
    ms = render.MeshSet([mesh], dev)
    apx = shade.Appearance(ms)
    radius_h = posedraw.mesh_radii([mesh])
    radius = torch.from_numpy(radius_h).to(dev)
    ids_h, slots_h = np.arange(S, dtype=np.int32), np.zeros((S, M), dtype=np.int32)
    ids, slots = torch.from_numpy(ids_h).to(dev), torch.from_numpy(slots_h).to(dev)
    word = torch.full((1,), SEED, dtype=torch.int64, device=dev)
    kw = dict(frame_hw=(H, W), near=NEAR, far=FAR, delta=DELTA, light=torch.tensor(shade.DEFAULT_LIGHT, device=dev), phong=torch.tensor(shade.DEFAULT_PHONG, device=dev))

    def upload(seed, into=None):
        h = posedraw.draw_scene_poses_host(cfg, seed, ids_h, slots_h, radius_h, K_H)
        arrays = [torch.from_numpy(np.ascontiguousarray(a)) for a in h]
        if into is None:
            return posedraw.ScenePoses(*[a.to(dev) for a in arrays])
        for dst, src in zip(into, arrays):
            dst.copy_(src)
        return into

    for s in (SEED, SEED + 1):
        got = synthscene.synth_scenes(ms, apx, radius, cfg, seed=s, scene_id=ids, mesh_index=slots, cam_K=K, **kw)
        want = synthscene.render_and_annotate(ms, apx, upload(s), K, **kw)
        torch.cuda.synchronize()
        for name, a, b in (("frames", got.frames, want.frames), ("depth", got.scene.depth, want.scene.depth), ("instance", got.scene.instance, want.scene.instance),
                           ("records", got.gt.info, want.gt.info), ("masks", got.gt.mask_visib, want.gt.mask_visib)):
            if not torch.equal(a, b):
                raise SystemExit(f"bench_posedraw: seed={s}: {name} of the chain differs from the host route's")

    def fresh():
        word.add_(1)
        return synthscene.synth_scenes(ms, apx, radius, cfg, seed=word, scene_id=ids, mesh_index=slots, cam_K=K, **kw)

    g_chain, _ = graphed(fresh, args.warmup)
    chain = replay_times(g_chain, args.iters)
    bufs = upload(SEED)
    g_host, _ = graphed(lambda: synthscene.render_and_annotate(ms, apx, bufs, K, **kw), args.warmup)
    t_draw, t_copy, t_replay = [], [], []
    for i in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = posedraw.draw_scene_poses_host(cfg, SEED + 1 + i, ids_h, slots_h, radius_h, K_H)
        t1 = time.perf_counter()
        for dst, src in zip(bufs, h):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_draw.append((t1 - t0) * 1e6)
        t_copy.append((t2 - t1) * 1e6)
        t_replay.append(replay_times(g_host, 1)["median_us"])
    host = dict(draw_wall=stats(t_draw), copy_wall=stats(t_copy), replay=stats(t_replay))
    host["total_us"] = host["draw_wall"]["median_us"] + host["copy_wall"]["median_us"] + host["replay"]["median_us"]
    scene = dict(S=S, M=M, frame_hw=[H, W], faces=int(len(mesh[1])), chain=chain, host_route=host, fresh_step_speedup_vs_host_route=host["total_us"] / chain["median_us"],
                 outputs_equal_to_the_host_route=True)
    print(json.dumps(scene), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, host_iters=args.host_iters, draws=draws, scene=scene)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
