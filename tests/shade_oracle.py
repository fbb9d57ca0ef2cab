"""fp64 numpy restatement of the shading pass's contract (TEST INFRASTRUCTURE ONLY; include/lc_amd_shade.h states the contract,
lc_amd/csrc/shade/lc_shade.hip is the kernel): every operation of steps 1 to 8 in the stated order, each numpy operation one rounded fp64
operation, vectorised over the hit pixels of a row.  The snapped screen coordinates are tests/render_oracle.project's.

    concat(meshes) -> Meshes                                    [(verts, faces, normals, colors), ...] concatenated, with the table
    shade(ms, face, mesh_index, R, t, K, light, phong, out, ...) -> Shaded            the instance form over a copy of `out`
    shade_scene(ms, frames, instance, face, mesh_index, scene_index, R, t, K, light, phong, origin_xy, ...) -> Shaded
    compose(depth, scene_index, origin_xy, frame_hw, S) -> (depth (S,H,W), instance (S,H,W))     include/lc_amd_gtinfo.h's composition

`Shaded.pre` holds the values `I c` before the final rounding (NaN where nothing was written): what a case's distance from a rounding
boundary is measured on.  `mistake` plants one of MISTAKES; tests/test_shade_host.py shows that each changes the bytes of the case list.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from tests import render_oracle

SUB = 256
MISTAKES = ("affine_weights", "normal_not_rotated", "light_in_gl_frame", "round_half_up", "misses_cleared", "vert_off_of_mesh_0")


class Meshes(NamedTuple):
    verts: np.ndarray    # (total_verts,3) float32
    faces: np.ndarray    # (total_faces,3) int32, indices relative to the mesh
    normals: np.ndarray  # (total_verts,3) float32
    colors: np.ndarray   # (total_verts,3) uint8
    table: np.ndarray    # (n_meshes,4) int32: vert_off, n_vert, face_off, n_face


class Shaded(NamedTuple):
    out: np.ndarray   # (...,h,w,3) uint8
    pre: np.ndarray   # (...,h,w,3) float64, NaN where nothing was written
    info: np.ndarray  # (B,) int32
    hit: np.ndarray   # (...,h,w) bool: written


class Pixels(NamedTuple):
    ok: np.ndarray    # (n,) bool: not refused
    byte: np.ndarray  # (n,3) uint8
    pre: np.ndarray   # (n,3) float64
    lam: np.ndarray   # (n,3) the weights
    c: np.ndarray     # (n,3) the interpolated colour


def concat(meshes) -> Meshes:
    table, vo, fo = [], 0, 0
    for v, f, _, _ in meshes:
        table.append((vo, len(v), fo, len(f)))
        vo, fo = vo + len(v), fo + len(f)
    cat = lambda k, dt: np.concatenate([np.asarray(m[k], dtype=dt).reshape(-1, 3) for m in meshes], 0)  # noqa: E731
    return Meshes(cat(0, np.float32), cat(1, np.int32), cat(2, np.float32), cat(3, np.uint8), np.asarray(table, dtype=np.int32))


def row_ok(ms: Meshes, mi: int) -> bool:
    if not 0 <= mi < len(ms.table):
        return False
    vo, nv, fo, nf = (int(v) for v in ms.table[mi])
    return min(vo, nv, fo, nf) >= 0 and vo + nv <= len(ms.verts) and fo + nf <= len(ms.faces)


def _dot3(a0, a1, a2, b0, b1, b2):
    p0 = a0 * b0
    p1 = a1 * b1
    p2 = a2 * b2
    s = p0 + p1
    return s + p2


def _unit(x, y, z):
    length = np.sqrt(_dot3(x, y, z, x, y, z))
    with np.errstate(all="ignore"):
        return [np.where(length == 0.0, 0.0, v / length) for v in (x, y, z)]


def _edge(bx, by, cx, cy, px, py):
    ex = cx - bx
    ey = cy - by
    dx = px - bx
    dy = py - by
    m0 = ex * dy
    m1 = ey * dx
    return m0 - m1


def shade_pixels(ms: Meshes, mi: int, R, t, K, light, phong, f, x, y, center=(0.5, 0.5), mistake=None) -> Pixels:
    """Steps 1 to 8 for the pixels (x, y) (window coordinates, (n,) integers) of a row whose mesh `mi` has passed `row_ok`, with the face
    indices f (n,)."""
    f, x, y = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (f, x, y))
    n = len(f)
    vo, nv, fo, nf = (int(v) for v in ms.table[mi])
    ok = (f >= 0) & (f < nf)
    tri = np.zeros((n, 3), dtype=np.int64)
    tri[ok] = ms.faces[fo + f[ok]]
    ok &= ((tri >= 0) & (tri < nv)).all(1)
    tri[~ok] = 0
    if nv == 0:
        return Pixels(np.zeros(n, bool), np.zeros((n, 3), np.uint8), np.full((n, 3), np.nan), np.full((n, 3), np.nan), np.full((n, 3), np.nan))
    gi = (int(ms.table[0][0]) if mistake == "vert_off_of_mesh_0" else vo) + tri
    R, t, K, light, phong = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (R, t, K, light, phong))
    _, s_all, _ = render_oracle.project(ms.verts, R, t, K)  # the rasteriser's snapped coordinates, as integer-valued doubles
    V = ms.verts.astype(np.float64)[gi]      # (n,3 vertices,3)
    Nm = ms.normals.astype(np.float64)[gi]
    Cm = ms.colors.astype(np.float64)[gi]
    with np.errstate(all="ignore"):
        Xc = np.stack([_dot3(R[r, 0], R[r, 1], R[r, 2], V[..., 0], V[..., 1], V[..., 2]) + t[r] for r in range(3)], -1)  # (n,3 vertices,3)
        z = Xc[..., 2]
        s = s_all[gi]                        # (n,3,2)
        px = (x * SUB + int(center[0] * SUB)).astype(np.float64)
        py = (y * SUB + int(center[1] * SUB)).astype(np.float64)
        (ax, ay), (bx, by), (cx, cy) = ((s[:, k, 0], s[:, k, 1]) for k in range(3))
        w = [_edge(bx, by, cx, cy, px, py), _edge(cx, cy, ax, ay, px, py), _edge(ax, ay, bx, by, px, py)]
        q = w if mistake == "affine_weights" else [w[k] / z[:, k] for k in range(3)]
        Q = q[0] + q[1]
        Q = Q + q[2]
        lam = [q[k] / Q for k in range(3)]
        interp = lambda A: np.stack([_dot3(lam[0], lam[1], lam[2], A[:, 0, i], A[:, 1, i], A[:, 2, i]) for i in range(3)], -1)  # noqa: E731
        c, nrm, P = interp(Cm), interp(Nm), interp(Xc)
        if mistake == "normal_not_rotated":
            m = [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
        else:
            m = [_dot3(R[r, 0], R[r, 1], R[r, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2]) for r in range(3)]
        if mistake == "light_in_gl_frame":  # OpenGL's camera: y up, z backward
            light = light * np.array([1.0, -1.0, -1.0])
        N = _unit(*m)
        L = _unit(light[0] - P[:, 0], light[1] - P[:, 1], light[2] - P[:, 2])
        Vv = _unit(-P[:, 0], -P[:, 1], -P[:, 2])
        nl = _dot3(N[0], N[1], N[2], L[0], L[1], L[2])
        d = np.where(nl > 0.0, nl, 0.0)
        two = 2.0 * nl
        Rv = [two * N[i] - L[i] for i in range(3)]
        rv = _dot3(Rv[0], Rv[1], Rv[2], Vv[0], Vv[1], Vv[2])
        sp = np.where(rv > 0.0, rv, 0.0)
        kdd = phong[1] * d
        kss = phong[2] * sp
        I = phong[0] + kdd
        I = I + kss
        pre = I[:, None] * c
        mid = np.floor(pre + 0.5) if mistake == "round_half_up" else np.rint(pre)
        byte = np.where(pre >= 255.0, 255.0, np.where(pre > 0.0, mid, 0.0))
    return Pixels(ok, byte.astype(np.uint8), pre, np.stack(lam, -1), c)


def _row_info(ms, mesh_index):
    return np.array([0 if row_ok(ms, int(mi)) else -1 for mi in mesh_index], dtype=np.int32)


def shade(ms: Meshes, face, mesh_index, R, t, K, light, phong, out, center=(0.5, 0.5), mistake=None) -> Shaded:
    """The instance form over a copy of out (B,h,w,3) uint8."""
    face = np.asarray(face, dtype=np.int32)
    out = np.array(out, dtype=np.uint8)
    B = len(face)
    pre, hit, info = np.full(out.shape, np.nan), np.zeros(face.shape, bool), _row_info(ms, mesh_index)
    for b in range(B):
        if info[b] < 0:
            continue
        ys, xs = np.nonzero(face[b] != -1)
        px = shade_pixels(ms, int(mesh_index[b]), R[b], t[b], K[b], light[b], phong[b], face[b, ys, xs], xs, ys, center, mistake)
        if not px.ok.all():
            info[b] = 1
        ys, xs = ys[px.ok], xs[px.ok]
        out[b, ys, xs], pre[b, ys, xs], hit[b, ys, xs] = px.byte[px.ok], px.pre[px.ok], True
    if mistake == "misses_cleared":
        out[~hit] = 0
    return Shaded(out, pre, info, hit)


def shade_scene(ms: Meshes, frames, instance, face, mesh_index, scene_index, R, t, K, light, phong, origin_xy=None, center=(0.5, 0.5),
                mistake=None) -> Shaded:
    """The scene form over a copy of frames (S,H,W,3) uint8."""
    face, instance = np.asarray(face, dtype=np.int32), np.asarray(instance, dtype=np.int32)
    frames = np.array(frames, dtype=np.uint8)
    B, h, w = face.shape
    pre, hit, info = np.full(frames.shape, np.nan), np.zeros(instance.shape, bool), _row_info(ms, mesh_index)
    for s in range(len(frames)):
        for b in np.unique(instance[s]):
            b = int(b)
            if not 0 <= b < B or info[b] < 0:
                continue  # -1: a miss; another value outside [0, B) names no row; a refused row writes nothing
            Ys, Xs = np.nonzero(instance[s] == b)
            x0, y0 = (0, 0) if origin_xy is None else (int(origin_xy[b][0]), int(origin_xy[b][1]))
            xs, ys = Xs - x0, Ys - y0
            ok = (int(scene_index[b]) == s) & (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
            if not ok.all():
                info[b] = 1
            Xs, Ys, xs, ys = Xs[ok], Ys[ok], xs[ok], ys[ok]
            px = shade_pixels(ms, int(mesh_index[b]), R[b], t[b], K[b], light[b], phong[b], face[b, ys, xs], xs, ys, center, mistake)
            if not px.ok.all():
                info[b] = 1
            Xs, Ys = Xs[px.ok], Ys[px.ok]
            frames[s, Ys, Xs], pre[s, Ys, Xs], hit[s, Ys, Xs] = px.byte[px.ok], px.pre[px.ok], True
    if mistake == "misses_cleared":
        frames[~hit] = 0
    return Shaded(frames, pre, info, hit)


def compose(depth, scene_index, origin_xy, frame_hw, S):
    """include/lc_amd_gtinfo.h's scene: per frame pixel the smallest z > 0 of the scene's rows that cover it, the lowest row among equal z
    -> (depth (S,H,W) float32, instance (S,H,W) int32, -1 where nothing is hit)."""
    H, W = frame_hw
    out = np.full((S, H, W), np.inf, dtype=np.float32)
    inst = np.full((S, H, W), -1, dtype=np.int32)
    for b, d in enumerate(np.asarray(depth, dtype=np.float32)):
        s = int(scene_index[b])
        x0, y0 = (0, 0) if origin_xy is None else (int(origin_xy[b][0]), int(origin_xy[b][1]))
        ys, xs = np.nonzero(d > 0)
        Ys, Xs = ys + y0, xs + x0
        keep = (Xs >= 0) & (Xs < W) & (Ys >= 0) & (Ys < H)
        ys, xs, Ys, Xs = ys[keep], xs[keep], Ys[keep], Xs[keep]
        win = d[ys, xs] < out[s, Ys, Xs]  # strictly: the lowest row keeps an equal z
        out[s, Ys[win], Xs[win]] = d[ys[win], xs[win]]
        inst[s, Ys[win], Xs[win]] = b
    return np.where(inst >= 0, out, np.float32(0)).astype(np.float32), inst
