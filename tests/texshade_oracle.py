"""fp64 numpy restatement of the textured shading pass's contract (TEST INFRASTRUCTURE ONLY; include/lc_amd_texture.h states the contract,
lc_amd/csrc/texture/lc_texture.hip is the kernel).  The unchanged steps are tests/shade_oracle.py's: a mesh without a texture goes through
`shade_oracle.shade_pixels` as it is, and a textured one through that module's `_dot3`, `_unit` and `_edge` in the stated order, each numpy
operation one rounded fp64 operation.

    mip_chain(image, levels=None) -> [(H_L,W_L,3) uint8, ...]                the store's rule for the levels behind level 0
    store(images, levels=None) -> (texels (N,4) uint8, table (n_tex,4) int64)  the layout of lc_amd.texture.TextureStore
    tex_pixels(tm, mi, R, t, K, light, phong, wrap, lod, f, x, y) -> Pixels   one row's pixels
    shade(tm, face, mesh_index, R, t, K, light, phong, wrap, lod, out) -> Shaded          the instance form over a copy of `out`
    shade_scene(tm, frames, instance, face, mesh_index, scene_index, R, t, K, light, phong, wrap, lod, origin_xy) -> Shaded
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from tests import render_oracle, shade_oracle
from tests.shade_oracle import SUB, Shaded, _dot3, _edge, _unit

MAX_SIZE, MAX_LEVELS = 16384, 15
COORD_LIMIT = 2.0 ** 30


class TexMeshes(NamedTuple):
    base: shade_oracle.Meshes
    uv: np.ndarray         # (total_faces,3,2) float32
    tex_index: np.ndarray  # (n_meshes,) int32
    texels: np.ndarray     # (N,4) uint8
    tex_table: np.ndarray  # (n_tex,4) int64: offset, Ht, Wt, n_levels


class Pixels(NamedTuple):
    ok: np.ndarray     # (n,) bool: not refused
    byte: np.ndarray   # (n,3) uint8
    pre: np.ndarray    # (n,3) float64
    level: np.ndarray  # (n,) the level sampled (-1: a mesh without a texture)


def level_sizes(Ht, Wt, n):
    out = []
    for _ in range(n):
        out.append((Ht, Wt))
        Ht, Wt = max(1, Ht >> 1), max(1, Wt >> 1)
    return out


def mip_chain(image, levels=None):
    """Level 0 is the image; per channel, texel (x, y) of level L+1 is (c(x0,y0) + c(x1,y0) + c(x0,y1) + c(x1,y1) + 2) >> 2 of level L with
    x0 = min(2x, W_L-1), x1 = min(2x+1, W_L-1) and the same for y.  levels None: down to 1 x 1."""
    im = np.asarray(image, dtype=np.uint8)
    full = max(im.shape[0], im.shape[1]).bit_length()
    n = full if levels is None else min(full, levels)
    chain = [im]
    for _ in range(1, n):
        src = chain[-1].astype(np.int64)
        Hs, Ws = src.shape[:2]
        Hd, Wd = max(1, Hs >> 1), max(1, Ws >> 1)
        y, x = np.arange(Hd), np.arange(Wd)
        y0, y1, x0, x1 = np.minimum(2 * y, Hs - 1), np.minimum(2 * y + 1, Hs - 1), np.minimum(2 * x, Ws - 1), np.minimum(2 * x + 1, Ws - 1)
        total = src[y0][:, x0] + src[y0][:, x1] + src[y1][:, x0] + src[y1][:, x1] + 2
        chain.append((total >> 2).astype(np.uint8))
    return chain


def store(images, levels=None):
    table, parts, off = [], [], 0
    for im in images:
        chain = mip_chain(im, levels)
        table.append((off, chain[0].shape[0], chain[0].shape[1], len(chain)))
        for lev in chain:
            parts.append(np.concatenate([lev.reshape(-1, 3), np.zeros((lev.shape[0] * lev.shape[1], 1), np.uint8)], 1))
            off += lev.shape[0] * lev.shape[1]
    return (np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.uint8)), np.asarray(table, dtype=np.int64).reshape(-1, 4)


def entry_ok(entry, total_texels) -> bool:
    off, Ht, Wt, n = (int(v) for v in entry)
    if off < 0 or not (1 <= Ht <= MAX_SIZE and 1 <= Wt <= MAX_SIZE and 1 <= n <= MAX_LEVELS):
        return False
    return off + sum(h * w for h, w in level_sizes(Ht, Wt, n)) <= total_texels


def row_ok(tm: TexMeshes, mi: int, wrap: int) -> bool:
    if not shade_oracle.row_ok(tm.base, mi) or wrap not in (0, 1):
        return False
    ti = int(tm.tex_index[mi])
    return ti == -1 or (0 <= ti < len(tm.tex_table) and entry_ok(tm.tex_table[ti], len(tm.texels)))


def _into(i, n, wrap):
    return np.mod(i, n) if wrap else np.clip(i, 0, n - 1)


def tex_pixels(tm: TexMeshes, mi: int, R, t, K, light, phong, wrap, lod, f, x, y, center=(0.5, 0.5)) -> Pixels:
    """The pixels (x, y) of a row whose mesh `mi` has passed `row_ok`, with the face indices f."""
    ms = tm.base
    ti = int(tm.tex_index[mi])
    if ti < 0:  # include/lc_amd_shade.h's pixel, as it is
        px = shade_oracle.shade_pixels(ms, mi, R, t, K, light, phong, f, x, y, center)
        return Pixels(px.ok, px.byte, px.pre, np.full(len(px.ok), -1))
    f, x, y = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (f, x, y))
    n = len(f)
    vo, nv, fo, nf = (int(v) for v in ms.table[mi])
    ok = (f >= 0) & (f < nf)
    tri = np.zeros((n, 3), dtype=np.int64)
    tri[ok] = ms.faces[fo + f[ok]]
    ok &= ((tri >= 0) & (tri < nv)).all(1)
    tri[~ok] = 0
    if nv == 0:
        return Pixels(np.zeros(n, bool), np.zeros((n, 3), np.uint8), np.full((n, 3), np.nan), np.zeros(n, np.int64))
    gi = vo + tri
    R, t, K, light, phong = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (R, t, K, light, phong))
    _, s_all, _ = render_oracle.project(ms.verts, R, t, K)
    V = ms.verts.astype(np.float64)[gi]
    Nm = ms.normals.astype(np.float64)[gi]
    UV = tm.uv.astype(np.float64)[fo + np.where(ok, f, 0)]  # (n,3 corners,2)
    off0, Ht, Wt, n_levels = (int(v) for v in tm.tex_table[ti])
    with np.errstate(all="ignore"):
        Xc = np.stack([_dot3(R[r, 0], R[r, 1], R[r, 2], V[..., 0], V[..., 1], V[..., 2]) + t[r] for r in range(3)], -1)
        z = Xc[..., 2]
        s = s_all[gi]
        px = (x * SUB + int(center[0] * SUB)).astype(np.float64)
        py = (y * SUB + int(center[1] * SUB)).astype(np.float64)
        (ax, ay), (bx, by), (cx, cy) = ((s[:, k, 0], s[:, k, 1]) for k in range(3))

        def weights(px, py):
            w = [_edge(bx, by, cx, cy, px, py), _edge(cx, cy, ax, ay, px, py), _edge(ax, ay, bx, by, px, py)]
            q = [w[k] / z[:, k] for k in range(3)]
            Q = q[0] + q[1]
            Q = Q + q[2]
            return [q[k] / Q for k in range(3)]

        def coords(lam):
            return _dot3(lam[0], lam[1], lam[2], UV[:, 0, 0], UV[:, 1, 0], UV[:, 2, 0]), _dot3(lam[0], lam[1], lam[2], UV[:, 0, 1], UV[:, 1, 1], UV[:, 2, 1])

        lam = weights(px, py)
        U, Vt = coords(lam)
        ok &= np.isfinite(U) & np.isfinite(Vt)
        level = np.zeros(n, dtype=np.int64)
        if lod:
            rho2 = []
            for lam_n in (weights(px + 256.0, py), weights(px, py + 256.0)):
                Un, Vn = coords(lam_n)
                du = (Un - U) * float(Wt)
                dv = (Vn - Vt) * float(Ht)
                rho2.append(du * du + dv * dv)
            r2 = np.where(rho2[0] > rho2[1], rho2[0], rho2[1])
            for L in range(1, n_levels):
                level += r2 > 2.0 ** (2 * L - 1)
        sizes = np.asarray(level_sizes(Ht, Wt, n_levels), dtype=np.int64)
        offs = off0 + np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])[:-1]])
        HL, WL, off = sizes[level, 0], sizes[level, 1], offs[level]
        tx = U * WL.astype(np.float64) - 0.5
        ty = (1.0 - Vt) * HL.astype(np.float64) - 0.5
        ok &= (np.abs(tx) < COORD_LIMIT) & (np.abs(ty) < COORD_LIMIT)  # (a NaN compares false)
        tx, ty = np.where(ok, tx, 0.0), np.where(ok, ty, 0.0)
        fx, fy = np.floor(tx), np.floor(ty)
        a8, b8 = np.floor(256.0 * (tx - fx)).astype(np.int64), np.floor(256.0 * (ty - fy)).astype(np.int64)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        xa, xb, ya, yb = _into(x0, WL, wrap), _into(x0 + 1, WL, wrap), _into(y0, HL, wrap), _into(y0 + 1, HL, wrap)
        tex = tm.texels.astype(np.int64)
        t00, t10, t01, t11 = tex[off + ya * WL + xa, :3], tex[off + ya * WL + xb, :3], tex[off + yb * WL + xa, :3], tex[off + yb * WL + xb, :3]
        c16 = ((256 - a8) * (256 - b8))[:, None] * t00 + (a8 * (256 - b8))[:, None] * t10 + ((256 - a8) * b8)[:, None] * t01 + (a8 * b8)[:, None] * t11
        c = c16.astype(np.float64) / 65536.0

        interp = lambda A: np.stack([_dot3(lam[0], lam[1], lam[2], A[:, 0, i], A[:, 1, i], A[:, 2, i]) for i in range(3)], -1)  # noqa: E731
        nrm, P = interp(Nm), interp(Xc)
        m = [_dot3(R[r, 0], R[r, 1], R[r, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2]) for r in range(3)]
        N = _unit(*m)
        Lv = _unit(light[0] - P[:, 0], light[1] - P[:, 1], light[2] - P[:, 2])
        Vv = _unit(-P[:, 0], -P[:, 1], -P[:, 2])
        nl = _dot3(N[0], N[1], N[2], Lv[0], Lv[1], Lv[2])
        d = np.where(nl > 0.0, nl, 0.0)
        two = 2.0 * nl
        Rv = [two * N[i] - Lv[i] for i in range(3)]
        rv = _dot3(Rv[0], Rv[1], Rv[2], Vv[0], Vv[1], Vv[2])
        sp = np.where(rv > 0.0, rv, 0.0)
        kdd = phong[1] * d
        kss = phong[2] * sp
        I = phong[0] + kdd
        I = I + kss
        pre = I[:, None] * c
        byte = np.where(pre >= 255.0, 255.0, np.where(pre > 0.0, np.rint(pre), 0.0))
    return Pixels(ok, byte.astype(np.uint8), pre, level)


def _row_info(tm, mesh_index, wrap):
    return np.array([0 if row_ok(tm, int(mi), int(wr)) else -1 for mi, wr in zip(mesh_index, wrap)], dtype=np.int32)


def shade(tm: TexMeshes, face, mesh_index, R, t, K, light, phong, wrap, lod, out, center=(0.5, 0.5)):
    """The instance form over a copy of out (B,h,w,3) uint8 -> (Shaded, level (B,h,w): the level sampled, -1 where no texture was)."""
    face = np.asarray(face, dtype=np.int32)
    out = np.array(out, dtype=np.uint8)
    pre, hit, info, level = np.full(out.shape, np.nan), np.zeros(face.shape, bool), _row_info(tm, mesh_index, wrap), np.full(face.shape, -1)
    for b in range(len(face)):
        if info[b] < 0:
            continue
        ys, xs = np.nonzero(face[b] != -1)
        px = tex_pixels(tm, int(mesh_index[b]), R[b], t[b], K[b], light[b], phong[b], int(wrap[b]), lod, face[b, ys, xs], xs, ys, center)
        if not px.ok.all():
            info[b] = 1
        ys, xs = ys[px.ok], xs[px.ok]
        out[b, ys, xs], pre[b, ys, xs], hit[b, ys, xs], level[b, ys, xs] = px.byte[px.ok], px.pre[px.ok], True, px.level[px.ok]
    return Shaded(out, pre, info, hit), level


def shade_scene(tm: TexMeshes, frames, instance, face, mesh_index, scene_index, R, t, K, light, phong, wrap, lod, origin_xy=None, center=(0.5, 0.5)) -> Shaded:
    """The scene form over a copy of frames (S,H,W,3) uint8."""
    face, instance = np.asarray(face, dtype=np.int32), np.asarray(instance, dtype=np.int32)
    frames = np.array(frames, dtype=np.uint8)
    B, h, w = face.shape
    pre, hit, info = np.full(frames.shape, np.nan), np.zeros(instance.shape, bool), _row_info(tm, mesh_index, wrap)
    for s in range(len(frames)):
        for b in np.unique(instance[s]):
            b = int(b)
            if not 0 <= b < B or info[b] < 0:
                continue
            Ys, Xs = np.nonzero(instance[s] == b)
            x0, y0 = (0, 0) if origin_xy is None else (int(origin_xy[b][0]), int(origin_xy[b][1]))
            xs, ys = Xs - x0, Ys - y0
            ok = (int(scene_index[b]) == s) & (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
            if not ok.all():
                info[b] = 1
            Xs, Ys, xs, ys = Xs[ok], Ys[ok], xs[ok], ys[ok]
            px = tex_pixels(tm, int(mesh_index[b]), R[b], t[b], K[b], light[b], phong[b], int(wrap[b]), lod, face[b, ys, xs], xs, ys, center)
            if not px.ok.all():
                info[b] = 1
            Xs, Ys = Xs[px.ok], Ys[px.ok]
            frames[s, Ys, Xs], pre[s, Ys, Xs], hit[s, Ys, Xs] = px.byte[px.ok], px.pre[px.ok], True
    return Shaded(frames, pre, info, hit)
