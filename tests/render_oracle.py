"""fp64 numpy restatement of the depth rasteriser's contract (TEST INFRASTRUCTURE ONLY; include/lc_amd_render.h states the contract,
lc_amd/csrc/render/lc_render.hip is the kernel): vectorised per face over its box.

    render(verts, faces, R, t, K, size_hw, near, far, center=(0.5, 0.5)) -> Ref

Vertices are transformed and projected in fp64 and snapped to 2^-8 px (round-half-even, np.rint); the edge functions are
integer-valued doubles (exact); a sample is covered when all three have one sign or are zero; 1/z is interpolated with the exact
barycentric weights and z rounded once to fp32; the smallest (fp32 bits of z, face index) wins.  A face with a vertex at z <= near
(or projecting beyond 2^17 px) is dropped and counted.

Besides the result the oracle returns what the GPU test's tolerances and exclusions are made of:
    z64       the winner's z before the rounding to fp32
    z_f32     the winner's z with the interpolation evaluated in fp32 (the role of an fp32 renderer: its error sets the tolerance)
    second    the runner-up's z (inf where only one face covers the pixel): pixels where it lies within the tolerance of the winner are
              "tie pixels", on which `face` is not compared
    margin    the smallest distance, in px, of a projected fp64 vertex coordinate to a snapping boundary: the kernel may contract
              multiply-adds that numpy does not, so a coordinate may differ in its last fp64 bits; a case must keep 2^-30 px clear
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

SUB = 256
MAX_SNAP = float(2 ** 25)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


class Ref(NamedTuple):
    depth: np.ndarray   # (H,W) float32
    mask: np.ndarray    # (H,W) bool
    face: np.ndarray    # (H,W) int32, -1 = miss
    z64: np.ndarray     # (H,W) float64, 0 = miss
    z_f32: np.ndarray   # (H,W) float32
    second: np.ndarray  # (H,W) float64, inf = no runner-up
    info: int
    margin: float


def project(verts, R, t, K):
    """(camera z (Nv,), snapped grid coordinates (Nv,2) as integer-valued doubles, margin in px) -- fp64 throughout."""
    V = np.asarray(verts, dtype=np.float32).astype(np.float64)
    R, t, K = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (R, t, K))
    Xc = V @ R.T + t
    z = Xc[:, 2]
    with np.errstate(all="ignore"):
        u = (K[0, 0] * Xc[:, 0] + K[0, 1] * Xc[:, 1] + K[0, 2] * z) / z
        v = (K[1, 0] * Xc[:, 0] + K[1, 1] * Xc[:, 1] + K[1, 2] * z) / z
        uv = np.stack((u, v), -1) * SUB
        s = np.rint(uv)
        frac = uv - np.floor(uv)
        margin = np.abs(frac - 0.5) / SUB
    return z, s, margin


def render(verts, faces, R, t, K, size_hw, near, far, center=(0.5, 0.5)) -> Ref:
    H, W = size_hw
    near32, far32 = np.float32(near), np.float32(far)
    cxi, cyi = center[0] * SUB, center[1] * SUB
    assert cxi == int(cxi) and cyi == int(cyi), "sample offsets lie on the 2^-8 grid"
    cxi, cyi = int(cxi), int(cyi)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    z, s, marg = project(verts, R, t, K)
    key1 = np.full((H, W), EMPTY, dtype=np.uint64)
    key2 = np.full((H, W), EMPTY, dtype=np.uint64)
    z64 = np.zeros((H, W))
    zf = np.zeros((H, W), dtype=np.float32)
    info = 0
    used = np.zeros(len(z), dtype=bool)
    for fi, (a, b, c) in enumerate(faces):
        zz = z[[a, b, c]]
        ss = s[[a, b, c]]
        if not (zz > float(near32)).all() or not (np.abs(ss) <= MAX_SNAP).all():
            info += 1
            continue
        used[[a, b, c]] = True
        (ax, ay), (bx, by), (cx, cy) = ss
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0:
            continue
        x0 = max(int(-((-(ss[:, 0].min() - cxi)) // SUB)), 0)
        x1 = min(int((ss[:, 0].max() - cxi) // SUB), W - 1)
        y0 = max(int(-((-(ss[:, 1].min() - cyi)) // SUB)), 0)
        y1 = min(int((ss[:, 1].max() - cyi) // SUB), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        px = (np.arange(x0, x1 + 1, dtype=np.float64) * SUB + cxi)[None, :]
        py = (np.arange(y0, y1 + 1, dtype=np.float64) * SUB + cyi)[:, None]
        w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
        w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
        w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        cov = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        if not cov.any():
            continue
        iz = 1.0 / zz
        with np.errstate(all="ignore"):
            zc = (w0 + w1 + w2) / (w0 * iz[0] + w1 * iz[1] + w2 * iz[2])
            z32 = zc.astype(np.float32)
            iz32 = iz.astype(np.float32)
            w032, w132, w232 = w0.astype(np.float32), w1.astype(np.float32), w2.astype(np.float32)
            zc32 = (w032 + w132 + w232) / (w032 * iz32[0] + w132 * iz32[1] + w232 * iz32[2])
        cov &= (z32 > near32) & (z32 < far32)
        if not cov.any():
            continue
        key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(fi)
        key = np.where(cov, key, EMPTY)
        k1 = key1[y0:y1 + 1, x0:x1 + 1]
        k2 = key2[y0:y1 + 1, x0:x1 + 1]
        win = key < k1
        key2[y0:y1 + 1, x0:x1 + 1] = np.minimum(k2, np.maximum(k1, key))
        key1[y0:y1 + 1, x0:x1 + 1] = np.minimum(k1, key)
        z64[y0:y1 + 1, x0:x1 + 1][win] = zc[win]
        zf[y0:y1 + 1, x0:x1 + 1][win] = zc32[win]
    mask = key1 != EMPTY
    depth = np.where(mask, (key1 >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    face = np.where(mask, (key1 & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    second = np.where(key2 != EMPTY, (key2 >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64), np.inf)
    margin = float(marg[used].min()) if used.any() else 1.0
    return Ref(depth, mask, face, z64, zf, second, info, margin)


def z_tolerance(ref: Ref) -> float:
    """Bound on max |z - z64| / z64 over hit pixels: twice the same measure of the oracle's own fp32 evaluation, at least 4 * 2^-24."""
    if not ref.mask.any():
        return 4 * 2.0 ** -24
    e32 = float((np.abs(ref.z_f32.astype(np.float64) - ref.z64)[ref.mask] / ref.z64[ref.mask]).max())
    return max(2 * e32, 4 * 2.0 ** -24)


def tie_pixels(ref: Ref, tol: float) -> np.ndarray:
    """(H,W) bool: covered pixels whose runner-up lies within `tol` (relative) of the winner; `face` is not compared there."""
    with np.errstate(all="ignore"):
        return ref.mask & (np.abs(ref.second - ref.z64) <= tol * ref.z64)


def points(ref: Ref, K, center=(0.5, 0.5), pix2k=None):
    """Camera-space fp64 intersection points (H,W,3) of the hit pixels (rows of zeros elsewhere): z64 K^-1 (x + cx, y + cy, 1)."""
    H, W = ref.mask.shape
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + center[0], np.arange(H, dtype=np.float64) + center[1])
    pix = np.stack((xs, ys, np.ones_like(xs)), -1)
    rays = pix @ np.linalg.inv(K).T
    return rays * ref.z64[..., None]
