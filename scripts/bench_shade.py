#!/usr/bin/env python3
"""Times the shading pass (lc_amd.shade) beside a float64 torch statement of the same bytes, and writes profiles/shade/bench_shade.json.

    python scripts/bench_shade.py [--iters 100] [--warmup 10] [--out profiles/shade/bench_shade.json]

The mesh is the 20 480-face icosphere of the other benchmarks with random vertex colours.  Two shapes: B = 32 maps of 128 x 128, and one
480 x 640 frame of 64 instances.  Per shape, device events around replayed graphs (median, p10 / p90 beside it):

  shade          `shade` alone on a resident face map
  render_color   `render_depth(want_face=True)` and `shade`
  render_scene   (the frame only) the instances' renders, the composition and `shade_scene`
  torch_f64      the same bytes stated with torch in float64 on the device -- gathers by face and vertex index, then element-wise
                 operations in the header's order -- on the resident face map: what `shade` stands beside

Before anything is timed the kernel's bytes are compared with the torch statement's on every hit pixel; the script reports the number
that differ (torch's float64 sqrt and division are correctly rounded too, so it expects 0).  Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lc_amd import render, shade  # noqa: E402
from tests import render_cases  # noqa: E402

NEAR, FAR = 0.01, 6.5


def stats(ts):
    ts = np.asarray(ts)
    return dict(median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)))


def graphed(fn, warmup):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
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


def torch_f64(ms, ap, face, R, t, K, light, phong, center=(0.5, 0.5)):
    """include/lc_amd_shade.h in float64 torch operations for full-size maps of one mesh: (B,h,w,3) uint8 over zeros."""
    B, h, w = face.shape
    hit = face >= 0
    tri = ms.faces[face.clamp(min=0).long()].long()                                  # (B,h,w,3)
    V, Nm, Cm = ms.verts.double()[tri], ap.normals.double()[tri], ap.colors.double()[tri]  # (B,h,w,3 vertices,3)
    Rd, td, Kd = R.double()[:, None, None], t.double()[:, None, None], K.double()[:, None, None]

    def dot3(a0, a1, a2, b0, b1, b2):
        return (a0 * b0 + a1 * b1) + a2 * b2

    def unit(x, y, z):
        n = torch.sqrt(dot3(x, y, z, x, y, z))
        return [torch.where(n == 0, torch.zeros_like(n), v / n) for v in (x, y, z)]

    Xc = torch.stack([dot3(Rd[..., r, 0, None], Rd[..., r, 1, None], Rd[..., r, 2, None], V[..., 0], V[..., 1], V[..., 2]) + td[..., r, None] for r in range(3)], -1)
    z = Xc[..., 2]
    su = torch.round(dot3(Kd[..., 0, 0, None], Kd[..., 0, 1, None], Kd[..., 0, 2, None], Xc[..., 0], Xc[..., 1], z) / z * 256.0)
    sv = torch.round(dot3(Kd[..., 1, 0, None], Kd[..., 1, 1, None], Kd[..., 1, 2, None], Xc[..., 0], Xc[..., 1], z) / z * 256.0)
    px = (torch.arange(w, device=face.device, dtype=torch.float64) * 256.0 + center[0] * 256.0)[None, None, :]
    py = (torch.arange(h, device=face.device, dtype=torch.float64) * 256.0 + center[1] * 256.0)[None, :, None]

    def edge(i, j):
        return (su[..., j] - su[..., i]) * (py - sv[..., i]) - (sv[..., j] - sv[..., i]) * (px - su[..., i])

    q = [edge(1, 2) / z[..., 0], edge(2, 0) / z[..., 1], edge(0, 1) / z[..., 2]]
    Q = (q[0] + q[1]) + q[2]
    lam = [qk / Q for qk in q]
    interp = lambda A: [dot3(lam[0], lam[1], lam[2], A[..., 0, i], A[..., 1, i], A[..., 2, i]) for i in range(3)]  # noqa: E731
    c, n, P = interp(Cm), interp(Nm), interp(Xc)
    Rr = R.double()[:, None, None]
    N = unit(*[dot3(Rr[..., r, 0], Rr[..., r, 1], Rr[..., r, 2], n[0], n[1], n[2]) for r in range(3)])
    ld, ph = light.double()[:, None, None], phong.double()[:, None, None]
    L = unit(ld[..., 0] - P[0], ld[..., 1] - P[1], ld[..., 2] - P[2])
    Vv = unit(-P[0], -P[1], -P[2])
    nl = dot3(N[0], N[1], N[2], L[0], L[1], L[2])
    two = 2.0 * nl
    rv = dot3(two * N[0] - L[0], two * N[1] - L[1], two * N[2] - L[2], Vv[0], Vv[1], Vv[2])
    I = (ph[..., 0] + ph[..., 1] * nl.clamp(min=0)) + ph[..., 2] * rv.clamp(min=0)
    pre = I[..., None] * torch.stack(c, -1)
    byte = torch.where(pre >= 255.0, torch.full_like(pre, 255.0), torch.where(pre > 0, torch.round(pre), torch.zeros_like(pre)))
    return torch.where(hit[..., None], byte, torch.zeros_like(byte)).to(torch.uint8)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--iters", type=int, default=100)
    ap_.add_argument("--warmup", type=int, default=10)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade", "bench_shade.json"))
    args = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shade: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    v, f = render_cases.icosphere(5, 0.1)  # 20 480 faces
    ms = render.MeshSet([(v, f)], dev)
    ap = shade.Appearance(ms, [rng.integers(0, 256, (len(v), 3), dtype=np.uint8)])
    result = dict(device=torch.cuda.get_device_name(0), faces=int(len(f)), iters=args.iters, shapes=[])
    for label, B, (h, w), frame in (("B32_128x128", 32, (128, 128), False), ("frame_480x640_64_instances", 64, (480, 640), True)):
        fpx = 1.25 * max(h, w)
        K = torch.tensor([[fpx, 0.0, w / 2 + 0.37], [0.0, 0.97 * fpx, h / 2 - 0.21], [0.0, 0.0, 1.0]], device=dev).expand(B, 3, 3).contiguous()
        R = torch.from_numpy(np.stack([render_cases.rot(rng.normal(size=3), float(rng.uniform(0, 360))) for _ in range(B)])).to(dev)
        if frame:  # 64 instances spread over the frame, each some 60 px across
            t = np.stack((rng.uniform(-0.35, 0.35, B), rng.uniform(-0.25, 0.25, B), rng.uniform(1.0, 1.6, B)), -1)
        else:      # one object filling most of its map
            t = np.stack((rng.uniform(-0.02, 0.02, B), rng.uniform(-0.02, 0.02, B), rng.uniform(0.3, 0.45, B)), -1)
        t = torch.from_numpy(t.astype(np.float32)).to(dev)
        mi = torch.zeros(B, dtype=torch.int32, device=dev)
        light = (torch.rand(B, 3, device=dev) - 0.5) * 2.0
        phong = torch.tensor(shade.DEFAULT_PHONG, device=dev).expand(B, 3).contiguous()
        face = render.render_depth(ms, mi, R, t, K, (h, w), near=NEAR, far=FAR, want_face=True).face
        out = torch.zeros(B, h, w, 3, dtype=torch.uint8, device=dev)
        shade.shade(ms, ap, face, mi, R, t, K, light=light, phong=phong, out=out)
        row = dict(shape=label, B=B, hw=[h, w], hit_pixels=int((face >= 0).sum()), pixels=B * h * w)
        chunk = 8 if frame else B  # the torch statement holds some forty float64 maps: it goes by 8 rows of the frame's size
        stated = torch.cat([torch_f64(ms, ap, face[i:i + chunk], R[i:i + chunk], t[i:i + chunk], K[i:i + chunk], light[i:i + chunk], phong[i:i + chunk])
                            for i in range(0, B, chunk)])
        row["pixels_differing_from_torch_f64"] = int((stated != out).any(-1).sum())
        del stated
        g, _ = graphed(lambda: shade.shade(ms, ap, face, mi, R, t, K, light=light, phong=phong, out=out), args.warmup)
        row["shade"] = replay_times(g, args.iters)
        g, _ = graphed(lambda: shade.render_color(ms, ap, mi, R, t, K, (h, w), near=NEAR, far=FAR, light=light, phong=phong), args.warmup)
        row["render_color"] = replay_times(g, args.iters)
        if frame:
            sidx = torch.zeros(B, dtype=torch.int32, device=dev)
            g, res = graphed(lambda: shade.render_scene(ms, ap, mi, sidx, R, t, K, (h, w), 1, near=NEAR, far=FAR, light=light, phong=phong), args.warmup)
            row["render_scene"] = replay_times(g, args.iters)
            row["scene_hit_pixels"] = int((res[1].instance >= 0).sum())
        n = min(chunk, B)
        g, _ = graphed(lambda: torch_f64(ms, ap, face[:n], R[:n], t[:n], K[:n], light[:n], phong[:n]), 3)
        row["torch_f64"] = dict(rows=n, **replay_times(g, max(10, args.iters // 5)))
        row["torch_f64"]["scaled_to_B_us"] = row["torch_f64"]["median_us"] * B / n
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
