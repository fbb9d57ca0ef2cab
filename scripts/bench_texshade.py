#!/usr/bin/env python3
"""Times the textured shading pass (lc_amd.texture) beside lc_amd.shade on the same maps and beside a float64 torch statement of the same
bytes, and writes profiles/texshade/bench_texshade.json.

    python scripts/bench_texshade.py [--iters 100] [--warmup 10] [--out profiles/texshade/bench_texshade.json]

The shapes and the protocol are scripts/bench_shade.py's: the 20 480-face icosphere, B = 32 maps of 128 x 128 and one 480 x 640 frame of 64
instances; device events around replayed graphs (median, p10 / p90 beside it).  The sphere carries a generated UV map (longitude and
latitude per vertex, gathered to face corners) and one 1024 x 1024 texture of random bytes with its full mip chain.  Per shape:

  texshade_lod     `texture.shade(lod=True)` on a resident face map: three perspective-correct interpolations, the level, four texel gathers
  texshade_flat    `texture.shade(lod=False)`: level 0, one interpolation
  shade            `lc_amd.shade.shade` on the same maps with per-vertex colours: what the textured pass adds to
  render_color     `render_depth(want_face=True)` and `texture.shade(lod=True)`
  torch_f64        the same bytes as texshade_lod stated with torch in float64 on the device, on the resident face map

Before anything is timed the kernel's bytes (lod on and off) are compared with the torch statement's on every pixel; the script reports
the number that differ and expects 0.  Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_shade import FAR, NEAR, graphed, replay_times  # noqa: E402
from lc_amd import render, shade, texture  # noqa: E402
from tests import render_cases  # noqa: E402


def sphere_uv(verts, faces) -> np.ndarray:
    """(Nf,3,2): longitude / 2 pi and latitude / pi of every vertex, gathered to the corners (the seam at longitude pi is left as it falls)."""
    v = verts.astype(np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    uv = np.stack((np.arctan2(v[:, 1], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 2], -1, 1)) / np.pi), -1).astype(np.float32)
    return uv[faces.astype(np.int64)]


def level_tables(store, dev):
    """(sizes (n_levels,2), offsets (n_levels,)) of texture 0 as int64 tensors on the device: made once, outside any capture."""
    off0, Ht, Wt, n_levels = (int(v) for v in store.table_host[0])
    sizes = torch.tensor(texture.level_sizes(Ht, Wt, n_levels), device=dev, dtype=torch.long)
    return sizes, off0 + torch.cumsum(sizes[:, 0] * sizes[:, 1], 0) - sizes[:, 0] * sizes[:, 1]


def torch_f64(ms, ap, tables, face, R, t, K, light, phong, wrap, lod, center=(0.5, 0.5)):
    """include/lc_amd_texture.h in float64 torch operations for full-size maps of ONE mesh with texture 0: (B,h,w,3) uint8 over zeros."""
    B, h, w = face.shape
    hit = face >= 0
    fidx = face.clamp(min=0).long()
    tri = ms.faces[fidx].long()                                                  # (B,h,w,3)
    V, Nm = ms.verts.double()[tri], ap.normals.double()[tri]                     # (B,h,w,3 vertices,3)
    UV = ap.uv.double()[fidx]                                                    # (B,h,w,3 corners,2)
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

    def weights(px, py):
        def edge(i, j):
            return (su[..., j] - su[..., i]) * (py - sv[..., i]) - (sv[..., j] - sv[..., i]) * (px - su[..., i])

        q = [edge(1, 2) / z[..., 0], edge(2, 0) / z[..., 1], edge(0, 1) / z[..., 2]]
        Q = (q[0] + q[1]) + q[2]
        return [qk / Q for qk in q]

    def coords(lam):
        return dot3(lam[0], lam[1], lam[2], UV[..., 0, 0], UV[..., 1, 0], UV[..., 2, 0]), dot3(lam[0], lam[1], lam[2], UV[..., 0, 1], UV[..., 1, 1], UV[..., 2, 1])

    lam = weights(px, py)
    U, Vt = coords(lam)
    _, Ht, Wt, n_levels = (int(v) for v in ap.textures.table_host[0])
    level = torch.zeros_like(face, dtype=torch.long)
    if lod:
        rho2 = []
        for lam_n in (weights(px + 256.0, py), weights(px, py + 256.0)):
            Un, Vn = coords(lam_n)
            du, dv = (Un - U) * float(Wt), (Vn - Vt) * float(Ht)
            rho2.append(du * du + dv * dv)
        r2 = torch.where(rho2[0] > rho2[1], rho2[0], rho2[1])
        for L in range(1, n_levels):
            level += r2 > 2.0 ** (2 * L - 1)
    sizes, offs = tables
    HL, WL, off = sizes[level, 0], sizes[level, 1], offs[level]
    tx = U * WL.double() - 0.5
    ty = (1.0 - Vt) * HL.double() - 0.5
    tx, ty = torch.where(hit, tx, torch.zeros_like(tx)), torch.where(hit, ty, torch.zeros_like(ty))
    fx, fy = torch.floor(tx), torch.floor(ty)
    a8, b8 = torch.floor(256.0 * (tx - fx)).long(), torch.floor(256.0 * (ty - fy)).long()
    x0, y0 = fx.long(), fy.long()

    def into(i, n):
        return torch.remainder(i, n) if wrap else torch.minimum(i.clamp(min=0), n - 1)

    xa, xb, ya, yb = into(x0, WL), into(x0 + 1, WL), into(y0, HL), into(y0 + 1, HL)
    tex = ap.textures.texels[:, :3]
    t00, t10, t01, t11 = (tex[off + yy * WL + xx].long() for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    c16 = ((256 - a8) * (256 - b8))[..., None] * t00 + (a8 * (256 - b8))[..., None] * t10 + ((256 - a8) * b8)[..., None] * t01 + (a8 * b8)[..., None] * t11
    c = c16.double() / 65536.0

    interp = lambda A: [dot3(lam[0], lam[1], lam[2], A[..., 0, i], A[..., 1, i], A[..., 2, i]) for i in range(3)]  # noqa: E731
    n, P = interp(Nm), interp(Xc)
    Rr = R.double()[:, None, None]
    N = unit(*[dot3(Rr[..., r, 0], Rr[..., r, 1], Rr[..., r, 2], n[0], n[1], n[2]) for r in range(3)])
    ld, ph = light.double()[:, None, None], phong.double()[:, None, None]
    L = unit(ld[..., 0] - P[0], ld[..., 1] - P[1], ld[..., 2] - P[2])
    Vv = unit(-P[0], -P[1], -P[2])
    nl = dot3(N[0], N[1], N[2], L[0], L[1], L[2])
    two = 2.0 * nl
    rv = dot3(two * N[0] - L[0], two * N[1] - L[1], two * N[2] - L[2], Vv[0], Vv[1], Vv[2])
    I = (ph[..., 0] + ph[..., 1] * nl.clamp(min=0)) + ph[..., 2] * rv.clamp(min=0)
    pre = I[..., None] * c
    byte = torch.where(pre >= 255.0, torch.full_like(pre, 255.0), torch.where(pre > 0, torch.round(pre), torch.zeros_like(pre)))
    return torch.where(hit[..., None], byte, torch.zeros_like(byte)).to(torch.uint8)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--iters", type=int, default=100)
    ap_.add_argument("--warmup", type=int, default=10)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "texshade", "bench_texshade.json"))
    args = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texshade: needs the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    v, f = render_cases.icosphere(5, 0.1)  # 20 480 faces
    ms = render.MeshSet([(v, f)], dev)
    colors = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    store = texture.TextureStore.from_images([rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)], dev)
    tap = texture.TexturedAppearance(ms, [sphere_uv(v, f)], [0], store, [colors])
    vap = shade.Appearance(ms, [colors])
    tables = level_tables(store, dev)
    result = dict(device=torch.cuda.get_device_name(0), faces=int(len(f)), texture=[1024, 1024], levels=int(store.table_host[0, 3]), iters=args.iters, shapes=[])
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
        wrap = torch.ones(B, dtype=torch.int32, device=dev)
        face = render.render_depth(ms, mi, R, t, K, (h, w), near=NEAR, far=FAR, want_face=True).face
        out = torch.zeros(B, h, w, 3, dtype=torch.uint8, device=dev)
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        row = dict(shape=label, B=B, hw=[h, w], hit_pixels=int((face >= 0).sum()), pixels=B * h * w)
        chunk = 4 if frame else B // 2  # the torch statement holds some sixty float64 maps: it goes by a few rows at a time
        for lod in (True, False):
            out.zero_()
            texture.shade(ms, tap, face, mi, R, t, K, light=light, phong=phong, wrap=wrap, lod=lod, out=out, info=info)
            stated = torch.cat([torch_f64(ms, tap, tables, face[i:i + chunk], R[i:i + chunk], t[i:i + chunk], K[i:i + chunk], light[i:i + chunk], phong[i:i + chunk], 1, lod)
                                for i in range(0, B, chunk)])
            row["pixels_differing_from_torch_f64_lod" if lod else "pixels_differing_from_torch_f64_flat"] = int((stated != out).any(-1).sum())
            row["rows_with_refusals"] = int((info != 0).sum()) + row.get("rows_with_refusals", 0)
            del stated
        g, _ = graphed(lambda: texture.shade(ms, tap, face, mi, R, t, K, light=light, phong=phong, wrap=wrap, lod=True, out=out), args.warmup)
        row["texshade_lod"] = replay_times(g, args.iters)
        g, _ = graphed(lambda: texture.shade(ms, tap, face, mi, R, t, K, light=light, phong=phong, wrap=wrap, lod=False, out=out), args.warmup)
        row["texshade_flat"] = replay_times(g, args.iters)
        g, _ = graphed(lambda: shade.shade(ms, vap, face, mi, R, t, K, light=light, phong=phong, out=out), args.warmup)
        row["shade"] = replay_times(g, args.iters)
        g, _ = graphed(lambda: texture.render_color(ms, tap, mi, R, t, K, (h, w), near=NEAR, far=FAR, light=light, phong=phong, wrap=wrap), args.warmup)
        row["render_color"] = replay_times(g, args.iters)
        n = min(chunk, B)
        g, _ = graphed(lambda: torch_f64(ms, tap, tables, face[:n], R[:n], t[:n], K[:n], light[:n], phong[:n], 1, True), 3)
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
