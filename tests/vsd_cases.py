"""Procedural cases of the VSD tests (TEST INFRASTRUCTURE ONLY): no assets.  The meshes, poses, near / far and the plain camera are those of
tests/render_cases.py, the depth maps come from tests/render_oracle.render, and a scene's measured depth is the nearest of the objects
standing in it (a pose's ground-truth object, an occluder) and a back plane, with a rectangular patch set to 0 as missing measurement.

Every call of a case list has B <= 6 rows.  Unit: metres; delta = 15 mm; BOP's ten taus, normalised by the diameter, except where a case
says otherwise.  tests/test_vsd_oracle.py asserts for every case what tests/test_gpu_vsd.py relies on: the margin condition
(tests/vsd_oracle.py) and the cap on the render oracle's tie pixels; a case that violates one gets another pose or depth offset, never a
smaller bound."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import render_cases as rc
from tests import render_oracle as ro
from tests import vsd_oracle

DELTA = 0.015
BOP_TAUS = tuple(0.05 * k for k in range(1, 11))
MESH_NAMES = ("box", "ico", "torus")  # the order of the MeshSet the GPU tests build
DIAMETER = {"box": 2 * float(np.linalg.norm(rc.MESHES["box"][0][0])), "ico": 0.2, "torus": 0.28}
MARGIN = 2.0 ** -30
TIE_CAP = 0.01  # of union


def stress_camera(size_hw):
    """The "stress" camera of lc_amd.synth (stretch 1.15 / 0.87 and skew 0.08 of the focal length) without its in-plane rotation: the
    score's ray length reads an upper-triangular K."""
    H, W = size_hw
    f = 1.25 * max(H, W)
    return np.array([[1.15 * f, 0.08 * f, W / 2 + 0.37], [0, 0.87 * f, H / 2 - 0.21], [0, 0, 1]], dtype=np.float32)


def integer_camera(size_hw):
    """fx != fy, skew, and an integer-valued principal point: shifting it by a window origin is exact in fp32."""
    H, W = size_hw
    f = 1.25 * max(H, W)
    return np.array([[f, 0.03 * f, W // 2], [0, 0.97 * f, H // 2], [0, 0, 1]], dtype=np.float32)


def pose(mesh, dt=(0.0, 0.0, 0.0), axis=None, deg=0.0, base=None):
    """render_cases' pose of `mesh` (or `base`), turned by `deg` about `axis` and moved by `dt` in the camera frame."""
    p = rc.POSES[mesh] if base is None else base
    R = p.R if axis is None else (rc.rot(axis, deg).astype(np.float64) @ p.R.astype(np.float64)).astype(np.float32)
    return rc.Pose(R, (p.t.astype(np.float64) + np.asarray(dt, dtype=np.float64)).astype(np.float32))


def at(xyz, axis=(0.2, 1, 0.1), deg=20.0):
    return rc.Pose(rc.rot(axis, deg), np.asarray(xyz, dtype=np.float32))


class Row(NamedTuple):
    mesh: str
    est: rc.Pose
    gt: rc.Pose
    scene: int           # outside the scenes: the row is refused
    expect: Optional[str] = None  # "zero", "one", "union0", "refused"


class Scene(NamedTuple):
    objects: tuple       # ((mesh, pose), ...)
    plane: float         # the back plane's depth
    patch: Optional[tuple] = None  # (y0, y1, x0, x1) set to 0


class Case(NamedTuple):
    name: str
    size_hw: tuple
    K: np.ndarray
    rows: tuple
    scenes: tuple
    taus: tuple = BOP_TAUS
    normalised: bool = True
    center: tuple = (0.0, 0.0)


_ICO, _TORUS, _BOX = rc.POSES["ico"], rc.POSES["torus"], rc.POSES["box"]


def _cases():
    out = []
    # one scene, five poses: identical; est behind gt by less than every tau d (4 mm), between them (35 mm) and by more than every one
    # (120 mm) -- d = 0.2 m, tau d = 10 .. 100 mm; est in front of the scene; and a row whose scene does not exist
    s = (64, 64)
    ico_scene = Scene((("ico", _ICO),), 1.0)
    out.append(Case("ico-depths-64x64", s, rc.camera(s), (
        Row("ico", _ICO, _ICO, 0, "zero"),
        Row("ico", pose("ico", (0, 0, 0.004)), _ICO, 0),
        Row("ico", pose("ico", (0, 0, 0.035)), _ICO, 0),
        Row("ico", pose("ico", (0, 0, 0.12)), _ICO, 0, "one"),
        Row("ico", pose("ico", (0, 0, -0.05)), _ICO, 0),
        Row("ico", _ICO, _ICO, 1, "refused"),
    ), (ico_scene,)))
    # occlusion, skew, a width of 4 k + 3: a torus behind a box that fills the frame (union = 0); behind an icosphere that hides a part of
    # it, in a scene with a missing patch; disjoint silhouettes; a box estimate turned and moved
    s = (33, 47)
    far_l, far_r = at((-0.2, 0.01, 1.2)), at((0.2, -0.02, 1.2))
    out.append(Case("occlusion-stress-33x47", s, stress_camera(s), (
        Row("torus", pose("torus", (0.004, 0, 0.003)), _TORUS, 0, "union0"),
        Row("torus", pose("torus", (0.006, -0.004, 0.011), (0, 0, 1), 4.0), _TORUS, 1),
        Row("torus", far_r, far_l, 2, "one"),
        Row("box", pose("box", (0.02, 0.01, 0.06), (1, 0, 0), 6.0), _BOX, 3),
        Row("torus", _TORUS, _TORUS, -1, "refused"),
    ), (
        Scene((("torus", _TORUS), ("box", at((0.0, 0.0, 0.3), (1, 2, 0.5), 3.0))), 1.0),
        Scene((("torus", _TORUS), ("ico", at((0.06, 0.03, 0.3)))), 0.8, (3, 14, 20, 31)),
        Scene((("torus", far_l),), 2.0),
        Scene((("box", _BOX), ("ico", at((-0.1, 0.05, 0.5)))), 1.5, (20, 30, 5, 40)),
    )))
    # W = 4 k + 1 and T = 16: the row phase of depth_est turns with every row
    s = (20, 45)
    out.append(Case("torus-t16-20x45", s, stress_camera(s), (
        Row("torus", pose("torus", (0.003, 0.002, 0.021), (0, 1, 0), 3.0), _TORUS, 0),
        Row("ico", pose("ico", (0.0, 0.01, 0.017)), _ICO, 1),
        Row("torus", pose("torus", (0.0, 0.0, -0.04)), _TORUS, 0),
    ), (
        Scene((("torus", _TORUS),), 1.0, (0, 6, 0, 9)),
        Scene((("ico", _ICO), ("ico", at((0.07, 0.02, 0.27)))), 0.9),
    ), taus=tuple(0.03 * k for k in range(1, 17))))
    # one pixel, one absolute tau: the ray of the optical axis
    K1 = np.array([[50, 0, 0], [0, 50, 0], [0, 0, 1]], dtype=np.float32)
    c1 = at((0.0, 0.0, 0.41))
    out.append(Case("ico-1x1", (1, 1), K1, (
        Row("ico", at((0.0, 0.0, 0.44)), c1, 0, "one"),
        Row("ico", at((0.0, 0.0, 0.415)), c1, 0, "zero"),
    ), (Scene((("ico", c1),), 1.0),), taus=(0.02,), normalised=False))
    # windows: an integer-valued principal point, objects small enough for a 32 x 32 window of the 64 x 64 frame
    s = (64, 64)
    Kw = integer_camera(s)
    w_ico, w_tor, w_box = at((0.03, -0.02, 0.8)), at((-0.05, 0.04, 1.1), (1, 0.2, 0.1), 63.0), at((0.1, 0.1, 2.6), (1, 2, 0.5), 31.0)
    out.append(Case("window-64x64", s, Kw, (
        Row("ico", pose("ico", (0.01, 0.0, 0.02), base=w_ico), w_ico, 0),
        Row("torus", pose("torus", (-0.01, 0.01, 0.03), (0, 0, 1), 5.0, base=w_tor), w_tor, 0),
        Row("box", pose("box", (0.0, -0.02, 0.05), base=w_box), w_box, 0),
        Row("ico", pose("ico", (0.2, 0.15, 0.0), base=w_ico), w_ico, 1, "one"),
    ), (
        Scene((("ico", w_ico), ("torus", w_tor), ("box", w_box)), 3.0, (40, 50, 10, 30)),
        Scene((("ico", w_ico),), 3.0),
    )))
    return tuple(out)


CASES = _cases()
WINDOW_CASE, WINDOW_HW = "window-64x64", (32, 32)


def case(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def _key(p: rc.Pose):
    return p.R.tobytes(), p.t.tobytes()


@functools.lru_cache(maxsize=None)
def _render(mesh, Rb, tb, Kb, size_hw, center):
    v, f = rc.MESHES[mesh]
    R, t, K = np.frombuffer(Rb, np.float32).reshape(3, 3), np.frombuffer(tb, np.float32), np.frombuffer(Kb, np.float32).reshape(3, 3)
    return ro.render(v, f, R, t, K, size_hw, rc.NEAR, rc.FAR, center)


def render(c: Case, mesh: str, p: rc.Pose) -> ro.Ref:
    """The render oracle's result, computed once per process and shared (treat as read-only)."""
    return _render(mesh, *_key(p), c.K.tobytes(), c.size_hw, c.center)


class Batch(NamedTuple):
    """What one call takes, as numpy arrays, and the oracle's answer for its rows (None: refused)."""
    depth_est: np.ndarray    # (B,H,W) float32
    depth_gt: np.ndarray
    depth_test: np.ndarray   # (S,H,W) float32
    K: np.ndarray            # (B,3,3) float32
    scene_index: np.ndarray  # (B,) int32
    diameter: Optional[np.ndarray]
    mesh_index: np.ndarray   # (B,) int32 into MESH_NAMES
    R_est: np.ndarray
    t_est: np.ndarray
    R_gt: np.ndarray
    t_gt: np.ndarray
    refs: tuple
    ties: np.ndarray         # (B,) the render oracle's tie pixels of both renders


def scene_depth(c: Case, s: Scene) -> np.ndarray:
    d = np.full(c.size_hw, np.float32(s.plane), dtype=np.float32)
    for mesh, p in s.objects:
        r = render(c, mesh, p)
        d = np.where(r.mask & (r.depth < d), r.depth, d)
    if s.patch is not None:
        y0, y1, x0, x1 = s.patch
        d[y0:y1, x0:x1] = 0
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(name: str) -> Batch:
    c = case(name)
    est = [render(c, r.mesh, r.est) for r in c.rows]
    gt = [render(c, r.mesh, r.gt) for r in c.rows]
    test = np.stack([scene_depth(c, s) for s in c.scenes])
    diam = np.asarray([DIAMETER[r.mesh] for r in c.rows], dtype=np.float32) if c.normalised else None
    refs = tuple(None if not 0 <= r.scene < len(c.scenes) else
                 vsd_oracle.score(e.depth, g.depth, test[r.scene], c.K, DELTA, c.taus, None if diam is None else diam[b], (0, 0), c.center)
                 for b, (r, e, g) in enumerate(zip(c.rows, est, gt)))
    ties = np.asarray([int(ro.tie_pixels(e, ro.z_tolerance(e)).sum()) + int(ro.tie_pixels(g, ro.z_tolerance(g)).sum()) for e, g in zip(est, gt)])
    return Batch(np.stack([e.depth for e in est]), np.stack([g.depth for g in gt]), test, np.repeat(c.K[None], len(c.rows), 0),
                 np.asarray([r.scene for r in c.rows], dtype=np.int32), diam, np.asarray([MESH_NAMES.index(r.mesh) for r in c.rows], dtype=np.int32),
                 np.stack([r.est.R for r in c.rows]), np.stack([r.est.t for r in c.rows]), np.stack([r.gt.R for r in c.rows]),
                 np.stack([r.gt.t for r in c.rows]), refs, ties)


def expected(name: str):
    """(counts (B,T+3) int32, errors (B,T) float32) of a call: -1 and NaN on the refused rows."""
    c, b = case(name), batch(name)
    T = len(c.taus)
    counts = np.stack([np.full(T + 3, -1, np.int32) if r is None else r.counts for r in b.refs])
    errors = np.stack([np.full(T, np.nan, np.float32) if r is None else r.errors for r in b.refs])
    return counts, errors


def silhouette_box(name: str, rows):
    """(x0, y0, x1, y1), inclusive: the box of every pixel that `rows`' estimate or ground truth hits."""
    b = batch(name)
    hit = np.zeros(b.depth_est.shape[1:], dtype=bool)
    for r in rows:
        hit |= (b.depth_est[r] > 0) | (b.depth_gt[r] > 0)
    ys, xs = np.nonzero(hit.any(1))[0], np.nonzero(hit.any(0))[0]
    return int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])
