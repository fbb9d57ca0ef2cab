"""Procedural meshes, poses and cameras of the rasteriser's tests (TEST INFRASTRUCTURE ONLY): no assets.  tests/test_render_oracle.py
asserts for every case the two conditions tests/test_gpu_render.py relies on (vertex coordinates clear of the snapping boundaries, few
tie pixels); a case that violates one gets another pose, never a wider cap.  The rules these cases keep clear of -- samples on edges,
snapping halves, exact depth ties, near and far themselves -- are decided on the exact scenes of tests/render_grid.py."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import render_oracle

NEAR, FAR = 0.01, 6.5  # metres, as tools/gen_z.py:75-76
SIZES = ((64, 64), (128, 128), (33, 47))


def box(h=(0.25, 0.2, 0.15)):
    s = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32) * np.asarray(h, dtype=np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return s, np.asarray(f, dtype=np.int32)


def icosphere(subdiv=2, radius=0.1):
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


def torus(nu=16, nv=8, R=0.1, r=0.04):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack(((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)), -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return v.astype(np.float32), np.asarray(f, dtype=np.int32)


def sliver_fan(n=40, radius=0.15, width=0.004):
    """Long thin triangles from one centre vertex: most cover a handful of samples, many none."""
    v, f = [(0.0, 0.0, 0.0)], []
    for k in range(n):
        a = 2 * np.pi * k / n + 0.013
        v += [(radius * np.cos(a), radius * np.sin(a), 0.02 * np.sin(3 * a)), (radius * np.cos(a + width), radius * np.sin(a + width), 0.02 * np.sin(3 * a))]
        f.append((0, 2 * k + 1, 2 * k + 2))
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def prefix(mesh, n):
    return mesh[0], mesh[1][:n].copy()


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).astype(np.float32)


def camera(size_hw, rotated=False):
    H, W = size_hw
    f = 1.25 * max(H, W)
    K = np.array([[f, 0, W / 2 + 0.37], [0, 0.97 * f, H / 2 - 0.21], [0, 0, 1]], dtype=np.float32)
    if rotated:  # an in-plane rotation and a shear around the map centre: non-zero K01 and K10
        th = np.deg2rad(23.0)
        A = np.array([[np.cos(th), -np.sin(th) + 0.1, 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        c = np.array([W / 2, H / 2])
        A[:2, 2] = c - A[:2, :2] @ c
        K = (A @ K.astype(np.float64)).astype(np.float32)
    return K


def with_near_faces(R, t):
    """An icosphere in view plus three faces that reach behind the near plane under the pose (R, t): they must be dropped whole."""
    v, f = icosphere(1, 0.1)
    cam = np.array([[0.05, 0.0, 0.005], [0.0, 0.05, -0.2], [-0.05, 0.0, 0.009], [0.0, -0.05, 0.01]])  # camera space: z <= near
    extra = ((cam - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32)  # R^T (x - t)
    n = len(v)
    v = np.concatenate((v, extra), 0)
    f = np.concatenate((f, np.asarray([(0, 1, n), (2, n + 1, n + 2), (3, 4, n + 3)], dtype=np.int32)), 0)
    return v.astype(np.float32), f


class Pose(NamedTuple):
    R: np.ndarray
    t: np.ndarray


_T168, _T169 = torus(16, 8), torus(16, 9)
POSES = {
    "box": Pose(rot((1, 2, 0.5), 31.0), np.array([0.013, -0.021, 0.9], dtype=np.float32)),
    "ico": Pose(rot((0.3, 1, 0.2), 17.0), np.array([0.021, 0.012, 0.41], dtype=np.float32)),
    "torus": Pose(rot((1, 0.2, 0.1), 63.0), np.array([-0.011, 0.017, 0.47], dtype=np.float32)),
    "fan": Pose(rot((0.2, 1, 0.1), 24.0), np.array([0.004, -0.007, 0.33], dtype=np.float32)),
    "torus1": Pose(rot((1, 0.1, 0.3), 41.0), np.array([-0.08, 0.03, 0.3], dtype=np.float32)),
    "torus63": Pose(rot((1, 0.3, 0.1), 52.0), np.array([0.012, 0.009, 0.62], dtype=np.float32)),
    "torus64": Pose(rot((1, 0.3, 0.2), 47.0), np.array([0.007, -0.013, 0.9], dtype=np.float32)),
    "torus65": Pose(rot((1, 0.4, 0.1), 58.0), np.array([-0.009, 0.011, 1.5], dtype=np.float32)),
    "torus257": Pose(rot((1, 0.1, 0.2), 66.0), np.array([0.015, 0.006, 0.52], dtype=np.float32)),
    "near": Pose(rot((0.1, 1, 0.3), 12.0), np.array([0.01, 0.02, 0.5], dtype=np.float32)),
}
MESHES = {
    "box": box(), "ico": icosphere(2), "torus": _T168, "fan": sliver_fan(),
    "torus1": prefix(_T168, 1), "torus63": prefix(_T168, 63), "torus64": prefix(_T168, 64), "torus65": prefix(_T168, 65),
    "torus257": prefix(_T169, 257), "near": with_near_faces(*POSES["near"]),
}
OUT_OF_VIEW = Pose(rot((0, 1, 0), 5.0), np.array([5.0, 0.3, 0.5], dtype=np.float32))


class Case(NamedTuple):
    name: str
    mesh: str
    pose: Pose
    K: np.ndarray
    size_hw: tuple


def grid_cases():
    """Every mesh x every small size; 480x640 with the box and with the icosphere; the out-of-view pose; a rotated K."""
    out = [Case(f"{m}-{h}x{w}", m, POSES[m], camera((h, w)), (h, w)) for m in MESHES for (h, w) in SIZES]
    out += [Case(f"{m}-480x640", m, POSES[m], camera((480, 640)), (480, 640)) for m in ("box", "ico")]
    out.append(Case("torus-out-of-view", "torus", OUT_OF_VIEW, camera((64, 64)), (64, 64)))
    out += [Case(f"{m}-rotK-{h}x{w}", m, POSES[m], camera((h, w), rotated=True), (h, w)) for m in ("torus", "box") for (h, w) in ((64, 64), (33, 47))]
    return out


CASES = grid_cases()
MIXED = ("ico", "torus", None, "ico", "box")  # the rows of the B = 5 batch: a repeated mesh and the out-of-view row (None: torus)


@functools.lru_cache(maxsize=None)
def reference(name: str, center=(0.5, 0.5)) -> render_oracle.Ref:
    """The oracle's result of a case, computed once per process and shared (treat as read-only)."""
    c = next(c for c in CASES if c.name == name)
    v, f = MESHES[c.mesh]
    return render_oracle.render(v, f, c.pose.R, c.pose.t, c.K, c.size_hw, NEAR, FAR, center)
