"""Scenes on the depth rasteriser's 2^-8 px grid and an integer reference of its contract (TEST INFRASTRUCTURE ONLY; the contract is
include/lc_amd_render.h, the kernel lc_amd/csrc/render/lc_render.hip).

A scene is given in integers: every vertex by the grid coordinates (units of 2^-8 px) it must project to and a camera depth that is a
power of two, the faces, the map size, the sample centre in grid units, near and far.  `scene()` turns that into float32 verts, R, t
and K with R a signed permutation, t dyadic and K = [[2^a, K01, K02], [0, 2^b, K12], [0, 0, 1]] with dyadic K01, K02, K12, so that
every intermediate of the kernel is exact: the fp64 transform, the projection (a division by a power of two), u * 256, 1/z, the edge
functions and w0 iz0 + w1 iz1 + w2 iz2.  An exact product plus an exact sum is the same with and without a fused multiply-add, so the
expected output is known to the last bit whatever the compiler contracts.  `scene()` asserts this for what it returns: it recomputes the
pipeline from the float32 arrays with fractions.Fraction, gets the intended grid coordinates back and bounds every product and sum by
53 bits.  (One scene, `near-rounds-onto-near`, cannot be exact -- its depth 2^-3 + 2^-40 is no power of two -- and is marked so: there
the projected coordinates lie within 2^-30 px of the intended ones, far from any snapping boundary, and the expected map is empty.)

`raster_int(scene)` is the reference, written from the header in Python integers and Fractions; it does not use tests/render_oracle.py.
tests/test_render_grid.py holds the two against each other, against hand counts, and asserts the reason each scene is there.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction as Fr
from typing import NamedTuple

import numpy as np

SUB = 256            # grid units per pixel
MAX_SNAP = 2 ** 25   # the largest snapped coordinate the contract accepts
TILE = 32            # the kernel's tile edge
COOP = 64            # box-in-tile samples above which the kernel's whole wave takes a face
EMPTY = (1 << 64) - 1
NEAR, FAR = 0.125, 8.0
CENTER = (128, 128)  # (0.5, 0.5) px
PIX2K = np.array([[0.5, 0.25, -3.125], [-0.125, 2.0, 7.5]], dtype=np.float32)  # a dyadic pix2k: every p z product is exact in fp64


class Camera(NamedTuple):
    R: tuple  # 3x3 signed permutation
    t: tuple  # dyadic
    K: tuple  # (fx, K01, K02, fy, K12): fx, fy powers of two, the rest dyadic


CAMERAS = (
    Camera(((1, 0, 0), (0, 1, 0), (0, 0, 1)), (0, 0, 0), (64, 0, 0, 64, 0)),
    Camera(((0, -1, 0), (0, 0, 1), (-1, 0, 0)), (Fr(1, 2), Fr(-1, 4), Fr(1, 2)), (128, Fr(1, 2), Fr(65, 4), 32, Fr(-7, 2))),
    Camera(((-1, 0, 0), (0, 1, 0), (0, 0, -1)), (-1, 2, -1), (32, Fr(-1, 4), 8, 64, Fr(19, 4))),
)
FAR_CAMERA = Camera(((0, 0, 1), (-1, 0, 0), (0, 1, 0)), (2048, 2048, 0), (64, 0, 0, 64, 0))  # t carries 2^25 grid units, the vertices the rest


class Scene(NamedTuple):
    name: str
    pts: tuple        # per vertex (gx, gy, z): Fractions, the projected coordinates in grid units BEFORE snapping and the camera depth
    faces: np.ndarray  # (F,3) int32
    size_hw: tuple
    center: tuple     # sample centre in grid units
    near: float
    far: float
    exact: bool
    verts: np.ndarray  # (Nv,3) float32
    R: np.ndarray
    t: np.ndarray
    K: np.ndarray

    @property
    def center_px(self):
        return (self.center[0] / SUB, self.center[1] / SUB)

    @property
    def group(self):
        """What one batched call shares."""
        return (self.size_hw, self.center, self.near, self.far)


def fits(x, bits=53) -> bool:
    """x is a dyadic rational with at most `bits` significant bits (exponents here are nowhere near fp64's limits)."""
    x = Fr(x)
    if x == 0:
        return True
    if x.denominator & (x.denominator - 1):
        return False
    n = abs(x.numerator)
    return (n // (n & -n)).bit_length() <= bits


def _dot(row, vec):
    """row . vec as the kernel forms it, left to right; every product and partial sum exact in fp64."""
    acc = None
    for a, b in zip(row, vec):
        p = a * b
        assert fits(p)
        acc = p if acc is None else acc + p
        assert fits(acc)
    return acc


def _verify(sc: Scene):
    """The kernel's setup in Fractions from the float32 arrays: the intended coordinates and depths come back, every step fits 53 bits."""
    V, R, t, K = (np.asarray(a, dtype=np.float32) for a in (sc.verts, sc.R, sc.t, sc.K))
    R, t, K = [[Fr(float(x)) for x in r] for r in R], [Fr(float(x)) for x in t], [[Fr(float(x)) for x in r] for r in K]
    for v, (gx, gy, z) in zip(V, sc.pts):
        v = [Fr(float(x)) for x in v]
        cam = []
        for r in range(3):
            c = _dot(R[r], v) + t[r]
            assert fits(c)
            cam.append(c)
        assert cam[2] == z
        for row, g in ((K[0], gx), (K[1], gy)):
            s = _dot(row, cam) / cam[2] * SUB
            if sc.exact:
                assert fits(cam[2], 1) and fits(s) and s == g, (sc.name, s, g)  # a division by a power of two, then the grid coordinate itself
            else:
                assert g.denominator == 1 and abs(s - g) <= Fr(SUB, 2 ** 30), (sc.name, s, g)
    # the raster stage: every edge-function product below 2^52 over the whole box (so every difference is exact), the interpolation's sums exact
    S = [(round(gx), round(gy)) for gx, gy, _ in sc.pts]
    H, W = sc.size_hw
    for f in sc.faces:
        if not all(0 <= i < len(S) for i in f) or any(max(abs(S[i][0]), abs(S[i][1])) > MAX_SNAP for i in f):
            continue
        xs, ys = [S[i][0] for i in f], [S[i][1] for i in f]
        px = [sc.center[0], SUB * (W - 1) + sc.center[0]]
        py = [sc.center[1], SUB * (H - 1) + sc.center[1]]
        span = max(max(xs) - min(xs), max(ys) - min(ys))
        reach = max(abs(s - v) for ss, vs in ((px, xs), (py, ys)) for s in ss for v in vs)
        assert span * reach <= 2 ** 52, sc.name
        if sc.exact:
            iz = [1 / sc.pts[i][2] for i in f if sc.pts[i][2] > 0]
            if len(iz) == 3 and len(set(iz)) > 1:  # slanted: three terms of at most 2 span reach max(iz), in units of min(iz)
                assert 6 * span * reach * max(iz) / min(iz) <= 2 ** 53, sc.name


def scene(name, pts, faces, size_hw, *, cam=CAMERAS[0], center=CENTER, near=NEAR, far=FAR, dz=0) -> Scene:
    """The float32 arrays of a scene given in integers.  `dz` is added to t_z AFTER the vertices are placed: every camera depth becomes
    z + dz, which is no power of two, and the scene is marked inexact (see the module docstring)."""
    Rm, tv, (fx, k01, k02, fy, k12) = cam
    verts = []
    for gx, gy, z in pts:
        gx, gy, z = Fr(gx), Fr(gy), Fr(z)
        yc = (gy / SUB - k12) * z / fy
        xc = ((gx / SUB - k02) * z - k01 * yc) / fx
        d = (xc - tv[0], yc - tv[1], z - tv[2])
        verts.append([sum(Rm[r][c] * d[r] for r in range(3)) for c in range(3)])  # R^T (x - t)
    v32 = np.array([[float(c) for c in v] for v in verts], dtype=np.float32).reshape(-1, 3)
    assert all(Fr(float(a)) == b for row, v in zip(v32, verts) for a, b in zip(row, v)), f"{name}: a vertex is no float32"
    t32 = np.array([float(tv[0]), float(tv[1]), float(tv[2] + Fr(dz))], dtype=np.float32)
    assert [Fr(float(x)) for x in t32] == [Fr(tv[0]), Fr(tv[1]), tv[2] + Fr(dz)]
    K32 = np.array([[fx, k01, k02], [0, fy, k12], [0, 0, 1]], dtype=np.float32)
    assert all(Fr(float(a)) == Fr(b) for a, b in zip(K32[:2].reshape(-1), (fx, k01, k02, 0, fy, k12)))
    assert float(np.float32(near)) == near and float(np.float32(far)) == far and abs(center[0]) <= 64 * SUB and abs(center[1]) <= 64 * SUB
    sc = Scene(name, tuple((Fr(gx), Fr(gy), Fr(z) + Fr(dz)) for gx, gy, z in pts), np.asarray(faces, dtype=np.int32).reshape(-1, 3),
               tuple(size_hw), tuple(center), float(near), float(far), dz == 0, v32, np.array(Rm, dtype=np.float32), t32, K32)
    _verify(sc)
    return sc


class Ref(NamedTuple):
    depth: np.ndarray        # (H,W) float32
    face: np.ndarray         # (H,W) int32, -1 = miss
    mask: np.ndarray         # (H,W) bool
    info: int
    homo_z: np.ndarray       # (H,W,3) float32 for the default pix2k [[1,0,cx],[0,1,cy]]
    homo_z_pix2k: np.ndarray  # for PIX2K
    tie: np.ndarray          # (H,W) bool: the two smallest keys carry the same depth bits
    runner: np.ndarray       # (H,W) int32 face of the second smallest key, -1 = none


def snap(v, rounding="even") -> int:
    v = Fr(v)
    if rounding == "even":
        return round(v)  # Python rounds a Fraction's half to even
    if rounding == "half_up":
        return math.floor(v + Fr(1, 2))
    assert rounding == "trunc"
    return math.trunc(v)


def snapped(sc: Scene, rounding="even"):
    return [(snap(gx, rounding), snap(gy, rounding)) for gx, gy, _ in sc.pts]


def box(sc: Scene, S, f):
    """Pixel indices whose samples lie inside the vertices' bounding box, clamped to the map: (x0, x1, y0, y1), empty where x0 > x1 or y0 > y1."""
    H, W = sc.size_hw
    xs, ys = [S[i][0] for i in f], [S[i][1] for i in f]
    return (max(-((-(min(xs) - sc.center[0])) // SUB), 0), min((max(xs) - sc.center[0]) // SUB, W - 1),
            max(-((-(min(ys) - sc.center[1])) // SUB), 0), min((max(ys) - sc.center[1]) // SUB, H - 1))


def tile_counts(sc: Scene, fi: int) -> dict:
    """{(tile_x, tile_y): samples of face fi's box inside that 32x32 tile}: what the kernel's lane path / wave path switch compares with 64."""
    x0, x1, y0, y1 = box(sc, snapped(sc), sc.faces[fi])
    out = {}
    for ty in range(0, sc.size_hw[0], TILE):
        for tx in range(0, sc.size_hw[1], TILE):
            w, h = min(x1, tx + TILE - 1) - max(x0, tx) + 1, min(y1, ty + TILE - 1) - max(y0, ty) + 1
            if w > 0 and h > 0:
                out[(tx // TILE, ty // TILE)] = w * h
    return out


def _f32_of_exact(q: Fr) -> np.float32:
    """One rounding to fp32 of a product that fp64 holds exactly."""
    assert fits(q)
    return np.float32(float(q))


def _homo(depth, mask, M):
    H, W = depth.shape
    out = np.zeros((H, W, 3), dtype=np.float32)
    for y, x in zip(*np.nonzero(mask)):
        z = Fr(float(depth[y, x]))
        for c in range(2):
            out[y, x, c] = _f32_of_exact((M[c][0] * int(x) + M[c][1] * int(y) + M[c][2]) * z)
        out[y, x, 2] = depth[y, x]
    return out


def raster_int(sc: Scene, rounding="even") -> Ref:
    """include/lc_amd_render.h in integers.  `rounding` other than "even" is there for the tests that show what a scene is sensitive to."""
    H, W = sc.size_hw
    cxi, cyi = sc.center
    near32, far32 = np.float32(sc.near), np.float32(sc.far)
    S = snapped(sc, rounding)
    Z = [z for _, _, z in sc.pts]
    key1 = [[EMPTY] * W for _ in range(H)]
    key2 = [[EMPTY] * W for _ in range(H)]
    info = 0
    for fi, f in enumerate(sc.faces.tolist()):
        if not all(0 <= i < len(S) for i in f):
            continue  # an invalid vertex index: covers nothing, not counted
        if any(Z[i] <= Fr(float(near32)) or abs(S[i][0]) > MAX_SNAP or abs(S[i][1]) > MAX_SNAP for i in f):
            info += 1
            continue
        (ax, ay), (bx, by), (cx, cy) = (S[i] for i in f)
        za, zb, zc = (Z[i] for i in f)
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0:
            continue
        x0, x1, y0, y1 = box(sc, S, f)
        for y in range(y0, y1 + 1):
            py = SUB * y + cyi
            for x in range(x0, x1 + 1):
                px = SUB * x + cxi
                w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
                w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
                w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
                if not ((w0 >= 0 and w1 >= 0 and w2 >= 0) or (w0 <= 0 and w1 <= 0 and w2 <= 0)):
                    continue
                assert w0 + w1 + w2 == area
                z32 = np.float32(float(Fr(area) / (Fr(w0) / za + Fr(w1) / zb + Fr(w2) / zc)))  # once to fp64, then to fp32
                if not (near32 < z32 < far32):
                    continue
                key = (int(z32.view(np.uint32)) << 32) | fi
                if key < key1[y][x]:
                    key1[y][x], key = key, key1[y][x]
                key2[y][x] = min(key2[y][x], key)
    k1, k2 = np.array(key1, dtype=np.uint64).reshape(H, W), np.array(key2, dtype=np.uint64).reshape(H, W)
    mask = k1 != np.uint64(EMPTY)
    hi = lambda k: (k >> np.uint64(32)).astype(np.uint32)  # noqa: E731
    lo = lambda k: (k & np.uint64(0xFFFFFFFF)).astype(np.int64)  # noqa: E731
    depth = np.where(mask, hi(k1).view(np.float32), np.float32(0)).astype(np.float32)
    face = np.where(mask, lo(k1), -1).astype(np.int32)
    second = k2 != np.uint64(EMPTY)
    cx, cy = Fr(cxi, SUB), Fr(cyi, SUB)
    M = [[Fr(float(v)) for v in r] for r in PIX2K]
    return Ref(depth, face, mask, info, _homo(depth, mask, [[1, 0, cx], [0, 1, cy]]), _homo(depth, mask, M),
               second & (hi(k1) == hi(k2)), np.where(second, lo(k2), -1).astype(np.int32))


# ---- the scenes -------------------------------------------------------------------------------------------------------------------

def S(p, c=128):
    """Grid coordinate of pixel index p's sample."""
    return SUB * p + c


def quad(x0, y0, x1, y1, z=1, cw=False):
    """Four shared vertices, two faces whose common edge is the diagonal from (x0,y0) to (x1,y1)."""
    pts = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    return pts, ([(0, 2, 1), (0, 3, 2)] if cw else [(0, 1, 2), (0, 2, 3)])


def soup(tris):
    """Faces that share no vertex: tris is a list of three (gx, gy, z)."""
    return [p for t in tris for p in t], [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(tris))]


def tri_px(a, b, c, z=1, off=(0, 0)):
    """A face with its vertices on the samples of three pixels (default centre), moved by `off` grid units; z one depth or three."""
    z = (z, z, z) if not isinstance(z, tuple) else z
    return tuple((S(p[0]) + off[0], S(p[1]) + off[1], zi) for p, zi in zip((a, b, c), z))


def filler(k, x0, y0, width, z=4):
    """A small face around the sample of pixel (x0 + k % width, y0 + k // width): it covers that sample alone."""
    sx, sy = S(x0 + k % width), S(y0 + k // width)
    return ((sx - 64, sy - 64, z), (sx + 64, sy - 64, z), (sx, sy + 64, z))


def placed(n, at: dict, x0, y0, width):
    """n faces: those of `at` at their indices, fillers everywhere else."""
    return soup([at.get(k) or filler(k, x0, y0, width) for k in range(n)])


def reversed_faces(sc: Scene) -> Scene:
    return sc._replace(name=sc.name + "-rev", faces=sc.faces[::-1].copy())


# the tie faces: both at z = 1, overlapping; A and B have an 8x8 box (the lane path), AW and BW a 16x16 box (the wave path)
TIE_A, TIE_B = tri_px((2, 2), (9, 2), (2, 9)), tri_px((4, 3), (11, 3), (4, 10))
TIE_AW, TIE_BW = tri_px((2, 2), (17, 2), (2, 17)), tri_px((4, 3), (19, 3), (4, 18))
TIES = {  # name: (index and face of the first, of the second)
    "tie-same-wave-0-1": ((0, TIE_A), (1, TIE_B)),
    "tie-waves-0-64": ((0, TIE_A), (64, TIE_B)),
    "tie-waves-0-191": ((0, TIE_A), (191, TIE_B)),
    "tie-trips-0-256": ((0, TIE_A), (256, TIE_B)),
    "tie-trips-3-300": ((3, TIE_A), (300, TIE_B)),
    "tie-lane-path-0-wave-path-1": ((0, TIE_A), (1, TIE_BW)),
    "tie-wave-path-0-lane-path-65": ((0, TIE_AW), (65, tri_px((10, 4), (17, 4), (10, 11)))),
    "tie-wave-paths-0-64": ((0, TIE_AW), (64, TIE_BW)),
}
NEGBOX = (-257, -256, -255, -1, 0, 1)
SAMPLE_CENTERS = ((0, 0), (128, 128), (1, 255), (-64 * SUB, 64 * SUB), (64 * SUB, -64 * SUB))
WAVE_FOUR = {0: tri_px((1, 1), (30, 2), (3, 29)), 1: tri_px((5, 3), (28, 8), (10, 30)), 62: tri_px((12, 10), (25, 12), (14, 27), Fr(1, 2)),
             63: tri_px((0, 0), (31, 0), (0, 31), 2)}
BIG = tri_px((1, 1), (30, 2), (3, 29))


def _build():
    out = []
    cams = iter(CAMERAS * 1000)

    def add(name, mesh, size_hw, **kw):
        kw.setdefault("cam", next(cams))  # the cameras take turns
        out.append(scene(name, mesh[0], mesh[1], size_hw, **kw))
        return out[-1]

    # edges and vertices
    add("quad-on-samples", quad(S(3), S(2), S(10), S(9)), (16, 16))
    add("quad-on-samples-cw", quad(S(3), S(2), S(10), S(9), cw=True), (16, 16))
    for tag, (dx, dy) in (("x+1", (1, 0)), ("x-1", (-1, 0)), ("y+1", (0, 1)), ("y-1", (0, -1))):
        add(f"quad-shift-{tag}", quad(S(3) + dx, S(2) + dy, S(10) + dx, S(9) + dy), (16, 16))
    edge = add("shared-edge-nearer-wins", soup([tri_px((2, 2), (8, 2), (8, 10)), tri_px((8, 2), (13, 6), (8, 10), Fr(1, 2))]), (16, 16))
    out.append(reversed_faces(edge))
    # exact depth ties
    for name, ((i, a), (j, b)) in TIES.items():
        sc = add(name, placed(max(i, j) + 1, {i: a, j: b}, 0, 22, 40), (40, 40))
        out.append(reversed_faces(sc))
    # lane path / wave path switch
    add("switch-64-lane-path", soup([tri_px((3, 2), (10, 2), (10, 9))]), (16, 16))
    add("switch-65-wave-path", soup([tri_px((3, 2), (7, 2), (3, 14))]), (16, 16))
    add("switch-seam-64-and-65", soup([tri_px((24, 24), (36, 30), (30, 44))]), (48, 48))
    add("wave-path-single-face", soup([BIG]), (32, 32))
    add("wave-path-last-of-65", placed(65, {64: BIG}, 0, 33, 40), (40, 40))
    add("wave-path-lanes-0-1-62-63", placed(64, WAVE_FOUR, 0, 33, 40), (40, 40))
    add("wave-path-face-257", placed(258, {257: BIG}, 0, 33, 40), (40, 40))
    # tiles and borders
    add("seams-both", soup([tri_px((5, 7), (60, 20), (25, 58))]), (64, 64))
    add("map-33x47-vertices-outside", soup([tri_px((-20, -10), (70, 5), (10, 60)), tri_px((-5, 40), (20, -30), (60, 45), 2)]), (33, 47))
    add("map-1x1", soup([tri_px((-1, -1), (2, -1), (-1, 2))]), (1, 1))
    add("map-1x65", soup([tri_px((-2, -3), (70, -3), (30, 5))]), (1, 65))
    add("map-65x1", soup([tri_px((-3, -2), (-3, 70), (5, 30))]), (65, 1))
    for d in NEGBOX:  # the first face starts d grid units from sample 0 and reaches into the map; the second, in front of it, ends there
        e = 128 + d
        add(f"negbox-{d:+d}", soup([((e, e, 1), (e + 1500, e, 1), (e, e + 1500, 1)), ((e, e, Fr(1, 2)), (e - 1500, e, Fr(1, 2)), (e, e - 1500, Fr(1, 2)))]), (8, 8))
    far_pts = [(-MAX_SNAP, -MAX_SNAP, 1), (MAX_SNAP, -MAX_SNAP, 1), (0, MAX_SNAP, 1)]
    add("extent-2^25", (far_pts, [(0, 1, 2)]), (64, 64), cam=FAR_CAMERA)
    add("extent-2^25+1", ([far_pts[0], (MAX_SNAP + 1, -MAX_SNAP, 1), far_pts[2]], [(0, 1, 2)]), (64, 64), cam=FAR_CAMERA)
    # snapping: an edge at k + 1/2 (see test_render_grid.py for which way each goes)
    h = Fr(1, 2)
    add("snap-even-left", quad(S(3) + h, S(3) + h, S(9) + 40, S(9) + 40), (16, 16))
    add("snap-even-right", quad(S(3, 129) - 40, S(3, 129) - 40, S(9, 129) - h, S(9, 129) - h), (16, 16), center=(129, 129))
    add("snap-odd-right", quad(S(3) - 40, S(3) - 40, S(9) - h, S(9) - h), (16, 16))
    add("snap-odd-left", quad(S(3, 129) + h, S(3, 129) + h, S(9, 129) + 40, S(9, 129) + 40), (16, 16), center=(129, 129))
    add("snap-even-negative", quad(-898 + h, S(2) - 40, -898 + 2 * SUB + 40, S(5) + 40), (8, 64), center=(-16258, 128))
    # sample centres: three quads with corners on whole pixels, one per window the centres look at
    q = [((512 + ox, 768 + oy), (2304 + ox, 2816 + oy)) for ox, oy in ((0, 0), (-64 * SUB, 64 * SUB), (64 * SUB, -64 * SUB))]
    three = soup([t for (x0, y0), (x1, y1) in q for t in (((x0, y0, 1), (x1, y0, 1), (x1, y1, 1)), ((x0, y0, 1), (x1, y1, 1), (x0, y1, 1)))])
    cam = next(cams)
    for c in SAMPLE_CENTERS:
        add(f"centre-{c[0]}-{c[1]}", three, (16, 16), center=c, cam=cam)
    # near and far
    wide = (S(3) - 40, S(3) - 40, S(9) + 40, S(9) + 40)  # 7 x 7 samples
    add("far-at", quad(*wide, z=8), (16, 16), far=8.0)
    add("far-just-below", quad(*wide, z=8), (16, 16), far=float(np.nextafter(np.float32(8), np.float32(9))))
    add("near-rounds-onto-near", quad(*wide, z=Fr(1, 8)), (16, 16), cam=CAMERAS[0], dz=Fr(1, 2 ** 40))
    p, f = quad(*wide, z=Fr(1, 4))
    add("near-vertex-at-near", (p + [(S(1), S(1), Fr(1, 8)), (S(12), S(2), Fr(1, 4)), (S(5), S(13), Fr(1, 4))], f + [(4, 5, 6)]), (16, 16))
    # zero area, each in front of a quad that must show through
    back = quad(*wide, z=2)

    def front(pts, face):
        return back[0] + pts, back[1] + [tuple(4 + i for i in face)]

    add("zero-repeated-index", front([(S(2), S(2), 1), (S(10), S(3), 1), (S(4), S(11), 1)], (0, 1, 1)), (16, 16))
    add("zero-snapped-collinear", front([(900, 900, 1), (1900, 1900, 1), (2900, 2900 + Fr(1, 4), 1)], (0, 1, 2)), (16, 16))
    add("sliver-no-sample", front([(S(3) + 1, 700, 1), (S(3) + 2, 700, 1), (S(3) + 1, 3000, 1)], (0, 1, 2)), (16, 16))
    add("sliver-one-sample", front([(S(3), 800, 1), (S(3) + 1, 800, 1), (S(3), 1100, 1)], (0, 1, 2)), (16, 16))
    # slanted faces: depths 1/4, 1/2, 1 against 1, 1/2, 1/4
    d0, d1 = (Fr(1, 4), Fr(1, 2), 1), (1, Fr(1, 2), Fr(1, 4))
    add("slanted-wave-path", soup([tri_px((2, 3), (44, 6), (10, 45), d0, (37, -91)), tri_px((4, 2), (45, 9), (8, 44), d1, (-13, 55))]), (48, 48))
    add("slanted-lane-path", soup([tri_px((2, 2), (9, 3), (3, 9), d0, (11, -5)), tri_px((2, 3), (9, 2), (4, 9), d1, (-7, 9))]), (16, 16))
    assert len({s.name for s in out}) == len(out)
    return tuple(out)


SCENES = _build()
BY_NAME = {s.name: s for s in SCENES}


def groups() -> dict:
    """{what one call shares: the scenes' names}."""
    out = {}
    for s in SCENES:
        out.setdefault(s.group, []).append(s.name)
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Ref:
    """raster_int of a scene, computed once per process and shared (treat as read-only)."""
    return raster_int(BY_NAME[name])
