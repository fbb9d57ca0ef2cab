"""Procedural cases of the VSD tests (TEST INFRASTRUCTURE ONLY): no assets.  The meshes, poses, near / far and the plain camera are those of
tests/render_cases.py, the depth maps come from tests/render_oracle.render, and a scene's measured depth is the nearest of the objects
standing in it (a pose's ground-truth object, an occluder) and a back plane, with a rectangular patch set to 0 as missing measurement.

Every call of a case list has B <= 6 rows.  Unit: metres; delta = 15 mm; BOP's ten taus, normalised by the diameter, except where a case
says otherwise.  tests/test_vsd_oracle.py asserts for every case what tests/test_gpu_vsd.py relies on: the margin condition
(tests/vsd_oracle.py) and the cap on the render oracle's tie pixels; a case that violates one gets another pose or depth offset, never a
smaller bound.

STRIP_CASES, further down, are not rasterised and are no members of CASES: synthetic maps sized from the kernel's kStripPixels (read from
lc_vsd.hip) so that a pose spans two to five strips, windows that span a strip boundary, single-pixel probes on every strip edge, and one
17 x 17 case whose comparisons sit exactly on delta and tau d, with -1, -0.0 and NaN among its depths."""
from __future__ import annotations

import functools
import os
import re
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


# ---- synthetic maps: the launch shape (strips of whole rows) and the comparisons on their thresholds ----
# Nothing below is rasterised and nothing below is a member of CASES (whose members also go through the numpy rasteriser in the chain
# tests).  The maps are made the way tests/gtinfo_cases.py makes its own: seeded blobs of hits on a depth grid of 1/64, a scene of grid
# values with noise of the size of delta on half of its pixels, a missing patch, a skewed camera with fx != fy.

KERNEL_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lc_amd", "csrc", "vsd", "lc_vsd.hip")


@functools.lru_cache(maxsize=None)
def strip_pixels() -> int:
    """The kernel's strip size, read from its source: the cases are sized from it, so they follow it when it changes."""
    with open(KERNEL_SOURCE) as f:
        m = re.findall(r"constexpr int kStripPixels = (\d+);", f.read())
    assert len(m) == 1, f"kStripPixels not found in {KERNEL_SOURCE}"
    return int(m[0])


def rps(w: int) -> int:
    """The kernel's rows per strip of maps w wide."""
    return 1 if w >= strip_pixels() else strip_pixels() // w


def strips_of(h: int, w: int):
    """(number of strips, rows of the last one)."""
    n = -(-h // rps(w))
    return n, h - (n - 1) * rps(w)


class StripCase(NamedTuple):
    """One call of vsd_from_depth as numpy arrays."""
    name: str
    depth_est: np.ndarray            # (B,h,w) float32
    depth_gt: np.ndarray
    depth_test: np.ndarray           # (S,H,W) float32
    K: np.ndarray                    # (B,3,3) float32
    scene_index: np.ndarray          # (B,) int32; outside [0,S): refused
    diameter: Optional[np.ndarray]   # (B,) float32
    origins: Optional[np.ndarray]    # (B,2) int32 (x0,y0); a window that reaches outside the frame: refused
    delta: float
    taus: tuple
    center: tuple = (0.0, 0.0)
    claim: Optional[tuple] = None    # (strips, rows of the last strip) the case was built to have

    @property
    def window_hw(self):
        return self.depth_est.shape[1:]

    @property
    def frame_hw(self):
        return self.depth_test.shape[1:]

    def origin(self, b):
        return (0, 0) if self.origins is None else (int(self.origins[b, 0]), int(self.origins[b, 1]))

    def refused(self, b):
        (h, w), (H, W), (x0, y0) = self.window_hw, self.frame_hw, self.origin(b)
        return not (0 <= self.scene_index[b] < len(self.depth_test) and 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H)

    def rows(self, rows):
        """The same call with the poses `rows` (a slice or a list)."""
        pick = lambda a: None if a is None else np.ascontiguousarray(a[rows])  # noqa: E731
        return self._replace(depth_est=pick(self.depth_est), depth_gt=pick(self.depth_gt), K=pick(self.K), scene_index=pick(self.scene_index),
                             diameter=pick(self.diameter), origins=pick(self.origins))


def squat_camera(size_hw):
    """The stress camera's stretch and skew with a focal length of 6.5 pixels along y: on a map of three or five rows, 4096 pixels wide, the
    ray length still changes by several per cent from one row to the next."""
    H, W = size_hw
    f = 1.25 * W
    return np.array([[1.15 * f, 0.08 * f, W / 2 + 0.37], [0, 6.5, H / 2 - 0.21], [0, 0, 1]], dtype=np.float32)


STRIP_DIAMETER = 0.2
# 0.08125 x 0.2 = 1.04 / 64: where est and gt lie one grid step apart, the ray length (1 to about 1.1 over a map) decides that cost
RAY_TAU = 0.08125
STRIP_TAUS = BOP_TAUS[:9] + (RAY_TAU,)
STRIP_TAUS_16 = tuple(0.03 * k for k in range(1, 16)) + (RAY_TAU,)
STRIP_TAUS_1 = (RAY_TAU,)


def _blob_pair(rng, h, w, rows=None, cols=None):
    """(est, gt) of one pose: two elliptic blobs of hits, a few pixels apart, that fill the rows [rows) from the first to the last and are
    clipped to [rows) x [cols).  gt lies on 60 .. 65 / 64, est on 58 .. 69 / 64: |est - gt| is 0 to 9 grid steps."""
    r0, r1 = rows or (0, h)
    c0, c1 = cols or (0, w)
    hh, ww = r1 - r0, c1 - c0
    yy, xx = np.mgrid[0:h, 0:w]
    box = (yy >= r0) & (yy < r1) & (xx >= c0) & (xx < c1)
    cy, cx = r0 + rng.uniform(0.4, 0.6) * hh, c0 + rng.uniform(0.4, 0.6) * ww
    ry, rx = max(rng.uniform(0.75, 0.9) * hh, 1.5), max(rng.uniform(0.3, 0.45) * ww, 1.5)
    dy, dx = rng.uniform(-0.08, 0.08) * hh, rng.uniform(-0.08, 0.08) * ww
    in_g = box & (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)
    in_e = box & (((yy - cy - dy) / ry) ** 2 + ((xx - cx - dx) / rx) ** 2 <= 1.0)
    gt = np.where(in_g, rng.integers(60, 66, size=(h, w)).astype(np.float32) / np.float32(64), np.float32(0))
    est = np.where(in_e, rng.integers(58, 70, size=(h, w)).astype(np.float32) / np.float32(64), np.float32(0))
    return est.astype(np.float32), gt.astype(np.float32)


def _noisy_scene(rng, H, W, delta):
    """Grid values 58 .. 67 / 64 around the blobs' depths; on half of the pixels noise of up to 2 delta on top; a missing patch."""
    grid = rng.integers(58, 68, size=(H, W)).astype(np.float64) / 64
    noise = np.where(rng.random((H, W)) < 0.5, rng.uniform(-2 * delta, 2 * delta, size=(H, W)), 0.0)
    d = (grid + noise).astype(np.float32)
    d[3 * H // 8:max(5 * H // 8, 3 * H // 8 + 1), W // 4:W // 2] = 0
    return d


def _synthetic(name, seed, size_hw, scenes, n_scenes, taus, K, claim):
    rng = np.random.default_rng(seed)
    h, w = size_hw
    B = len(scenes)
    pairs = [_blob_pair(rng, h, w) for _ in range(B)]
    test = np.stack([_noisy_scene(rng, h, w, DELTA) for _ in range(n_scenes)])
    return StripCase(name, np.stack([e for e, _ in pairs]), np.stack([g for _, g in pairs]), test, np.repeat(K[None], B, 0),
                     np.asarray(scenes, dtype=np.int32), np.full(B, STRIP_DIAMETER, dtype=np.float32), None, DELTA, taus, (0.0, 0.0), claim)


WINDOW_STRIP_CASE = "strip-window"
WINDOW_STRIP_FRAME = (200, 83)    # W = 4 k + 3: the 16-byte phase of the scene's row turns with every row
WINDOW_STRIP_HW = (150, 41)       # two strips where a strip is 4096 pixels
WINDOW_STRIP_HELD = (0, 1)        # the rows whose window holds both silhouettes clear of its border


def _window_case(seed=31):
    """Six poses in windows of one frame: hits in the last strip only; hits on the two rows where the first strip meets the second and
    nowhere else; a window outside the frame (refused); hits cut by the window's bottom side; a scene_index past the scenes (refused); hits
    cut by the window's top side."""
    rng = np.random.default_rng(seed)
    (H, W), (h, w) = WINDOW_STRIP_FRAME, WINDOW_STRIP_HW
    n, last = strips_of(h, w)
    r0 = (n - 1) * rps(w)  # the last strip's first row
    assert n >= 2 and 2 <= r0 and last >= 3, "the window case needs a window of at least two strips"
    inside = (1, w - 1)
    pairs = [_blob_pair(rng, h, w, (r0, h - 1), inside), _blob_pair(rng, h, w, (r0 - 1, r0 + 1), inside), _blob_pair(rng, h, w),
             _blob_pair(rng, h, w, (r0 // 2, h), inside), _blob_pair(rng, h, w), _blob_pair(rng, h, w, (0, r0 + last // 2), inside)]
    origins = np.asarray([[3, 7], [8, 20], [W - w + 1, 5], [13, 1], [2, 9], [22, H - h - 1]], dtype=np.int32)
    scenes = np.asarray([0, 1, 0, 1, 2, 0], dtype=np.int32)
    test = np.stack([_noisy_scene(rng, H, W, DELTA) for _ in range(2)])
    return StripCase(WINDOW_STRIP_CASE, np.stack([e for e, _ in pairs]), np.stack([g for _, g in pairs]), test,
                     np.repeat(stress_camera((H, W))[None], 6, 0), scenes, np.full(6, STRIP_DIAMETER, dtype=np.float32), origins, DELTA, STRIP_TAUS,
                     (0.0, 0.0), (n, last))


def full_frame_of(c: StripCase, rows) -> StripCase:
    """The poses `rows` of a window case as a call without windows: each window's maps set into a frame of zeros."""
    H, W = c.frame_hw
    h, w = c.window_hw
    est, gt = np.zeros((len(rows), H, W), np.float32), np.zeros((len(rows), H, W), np.float32)
    for i, b in enumerate(rows):
        x0, y0 = c.origin(b)
        est[i, y0:y0 + h, x0:x0 + w], gt[i, y0:y0 + h, x0:x0 + w] = c.depth_est[b], c.depth_gt[b]
    return c.rows(list(rows))._replace(name=c.name + "-full-frame", depth_est=est, depth_gt=gt, origins=None, claim=strips_of(H, W))


TIE_CASE = "ties-17x17"
TIE_DELTA, TIE_TAUS, TIE_DIAMETER = 3 / 64, (3 / 8, 3 / 4), 0.5
# (y, x, comparison) of the pixels whose ray length is exact -- 1 at the principal point, 3/2 at (+-2, +-4) and (+-4, +-2) from it, 3 at
# (+-8, +-8) -- and the comparison that sits on its threshold there: "gt" dist_gt - dist_test = delta, "est" dist_est - dist_test = delta,
# "cost" |dist_gt - dist_est| = tau_0 d
TIE_PIXELS = ((8, 8, "gt"), (12, 10, "gt"), (12, 6, "est"), (4, 10, "cost"), (4, 6, "gt"), (10, 12, "est"), (10, 4, "cost"), (6, 12, "est"),
              (6, 4, "cost"), (0, 0, "gt"), (0, 16, "est"), (16, 0, "cost"), (16, 16, "cost"))
TIE_POSES = (0, 1, 2)  # the tie; the deciding depth one fp32 step up; one step down
VALUE_POSE = 3
ODD_VALUES = (-1.0, -0.0, float("nan"))
# (y, x, est, gt, test) of the value pose, `None` standing for each of ODD_VALUES in turn along x
VALUE_PIXELS = ((1, 2, None, 1.0, 1.0), (2, 2, 1.0, None, 1.0), (3, 10, None, None, 1.0), (5, 8, 1.0, 1.0, None), (7, 1, None, 0.0, 0.0),
                (9, 9, 0.0, None, 0.0), (11, 12, 1.0, 0.0, None), (13, 5, None, 1.0, None))


def _tie_case():
    """K00 = K11 = 4, no skew, principal point (8, 8), pixel centre (0, 0): n = sqrt(dx^2 + dy^2 + 16) / 4.  delta = 3/64 and
    tau_0 d = 3/16, so at a pixel of ray length n the depths 1 and 1 + 3 / (64 n), or 1 and 1 + 3 / (16 n), are dyadic numbers whose
    distances differ by exactly the threshold.  A "cost" pixel's scene is missing at n = 3/2 and far behind (4) elsewhere."""
    H = W = 17
    K = np.array([[4, 0, 8], [0, 4, 8], [0, 0, 1]], dtype=np.float32)
    n_exact = {0: 1.0, 20: 1.5, 128: 3.0}
    est, gt = np.zeros((4, H, W), np.float32), np.zeros((4, H, W), np.float32)
    test = np.ones((1, H, W), np.float32)
    for y, x, kind in TIE_PIXELS:
        n = n_exact[(y - 8) ** 2 + (x - 8) ** 2]
        step = np.float32((3 / 16 if kind == "cost" else 3 / 64) / n)
        at = np.float32(1) + step
        assert float(at) == 1 + float(step) and float(step) * n in (3 / 16, 3 / 64)  # dyadic: nothing is rounded
        values = (at, np.nextafter(at, np.float32(2)), np.nextafter(at, np.float32(0)))
        for pose, v in zip(TIE_POSES, values):
            if kind == "gt":
                gt[pose, y, x] = v
            elif kind == "est":
                est[pose, y, x] = v
            else:
                gt[pose, y, x], est[pose, y, x] = 1.0, v
        if kind == "cost":
            test[0, y, x] = 0.0 if n == 1.5 else 4.0
    for y, x, *triple in VALUE_PIXELS:
        for i, odd in enumerate(ODD_VALUES):
            e, g, t = (np.float32(odd if v is None else v) for v in triple)
            est[VALUE_POSE, y, x + i], gt[VALUE_POSE, y, x + i] = e, g
            assert test[0, y, x + i] == 1.0  # no pixel is used twice
            test[0, y, x + i] = t
    return StripCase(TIE_CASE, est, gt, test, np.repeat(K[None], 4, 0), np.zeros(4, np.int32), np.full(4, TIE_DIAMETER, np.float32), None, TIE_DELTA,
                     TIE_TAUS, (0.0, 0.0), (1, H))


@functools.lru_cache(maxsize=None)
def strip_cases():
    sp = strip_pixels()
    t47, w64 = (2 * rps(47) + 5, 47), (rps(64) + 1, 64)
    out = [
        # three strips with a ragged last one; three poses on three scenes, T = 16
        _synthetic("strip-ragged-w47", 21, t47, (2, 0, 1), 3, STRIP_TAUS_16, stress_camera(t47), (3, 5)),
        # the last strip is one row; three poses on three scenes and one more on the first, T = 1
        _synthetic("strip-one-row-w64", 22, w64, (1, 2, 0, 1), 3, STRIP_TAUS_1, stress_camera(w64), (2, 1)),
        # the widths at which rows_per_strip changes: two rows per strip, then one; and the branch w >= kStripPixels from both sides
        _synthetic("strip-half", 23, (5, sp // 2), (0, 1), 2, STRIP_TAUS, squat_camera((5, sp // 2)), (3, 1)),
        _synthetic("strip-half-plus-1", 24, (3, sp // 2 + 1), (0, 0), 1, STRIP_TAUS, squat_camera((3, sp // 2 + 1)), (3, 1)),
        _synthetic("strip-whole-minus-1", 25, (3, sp - 1), (0, 0), 1, STRIP_TAUS, squat_camera((3, sp - 1)), (3, 1)),
        _synthetic("strip-whole", 26, (3, sp), (1, 0), 2, STRIP_TAUS, squat_camera((3, sp)), (3, 1)),
        _synthetic("strip-whole-plus-1", 27, (5, sp + 1), (0, 0), 1, STRIP_TAUS, squat_camera((5, sp + 1)), (5, 1)),
        _window_case(),
        _tie_case(),
    ]
    return tuple(out)


STRIP_CASES = strip_cases()
STRIP_NAMES = tuple(c.name for c in STRIP_CASES)
MULTI_STRIP_CASE = "strip-ragged-w47"


def strip_case(name: str) -> StripCase:
    return next(c for c in STRIP_CASES if c.name == name)


def as_call(name: str) -> StripCase:
    """A member of CASES in the form of a StripCase: what test_score_equals_the_oracle passes to vsd_from_depth."""
    c, b = case(name), batch(name)
    return StripCase(name, b.depth_est, b.depth_gt, b.depth_test, b.K, b.scene_index, b.diameter, None, DELTA, c.taus, c.center, None)


def score_call(c: StripCase):
    """(counts (B,T+3) int32, errors (B,T) float32, refs): the oracle's answer to a call, -1 / NaN / None on its refused rows."""
    T = len(c.taus)
    refs = tuple(None if c.refused(b) else
                 vsd_oracle.score(c.depth_est[b], c.depth_gt[b], c.depth_test[c.scene_index[b]], c.K[b], c.delta, c.taus,
                                  None if c.diameter is None else c.diameter[b], c.origin(b), c.center) for b in range(len(c.depth_est)))
    counts = np.stack([np.full(T + 3, -1, np.int32) if r is None else r.counts for r in refs])
    errors = np.stack([np.full(T, np.nan, np.float32) if r is None else r.errors for r in refs])
    return counts, errors, refs


@functools.lru_cache(maxsize=None)
def strip_expected(name: str):
    """`score_call` of a strip case, computed once per process and shared (treat as read-only)."""
    return score_call(strip_case(name))


PROBE_SHAPES = ((2 * rps(47) + 5, 47), (5, strip_pixels() // 2), (3, strip_pixels() + 1))


def probe_pixels(h, w):
    """The first and the last row of every strip (the map's last row among them), each at columns 0 and w - 1."""
    n, _ = strips_of(h, w)
    rows = sorted({r for s in range(n) for r in (s * rps(w), min(h, (s + 1) * rps(w)) - 1)} | {h - 1})
    return [(y, x) for y in rows for x in (0, w - 1)]


def probe_calls(h, w):
    """Calls of up to six poses, each pose with ONE hit pixel (est = gt = 1, on a scene that measures 1 everywhere): union = inter = 1,
    edge = 0, no cost, error 0.  -> [(StripCase, [(y, x), ...])]"""
    px = probe_pixels(h, w)
    out = []
    for i in range(0, len(px), 6):
        part = px[i:i + 6]
        maps = np.zeros((len(part), h, w), np.float32)
        for b, (y, x) in enumerate(part):
            maps[b, y, x] = 1.0
        K = np.repeat((stress_camera if h > 8 else squat_camera)((h, w))[None], len(part), 0)
        out.append((StripCase(f"probe-{h}x{w}-{i // 6}", maps, maps.copy(), np.ones((1, h, w), np.float32), K, np.zeros(len(part), np.int32),
                              np.full(len(part), STRIP_DIAMETER, np.float32), None, DELTA, STRIP_TAUS_1, (0.0, 0.0), strips_of(h, w)), part))
    return out
