"""Cases of the annotation tests (TEST INFRASTRUCTURE ONLY): no assets, every map made by a seeded numpy generator or written out by hand.

A render is an elliptic silhouette that may reach over the window's sides, with depths on a 1/16 grid (so that two instances tie at many
pixels when a scene is composed from them) and a sprinkle of what a render should never hold but a caller's map may: 0, negative values,
NaN and +inf inside the silhouette.  A scene's depth is part grid values (ties with the render), part uniform noise (differences of every
size around delta) and a sprinkle of 0, negative values, NaN and +inf.  Every call has B <= 6 rows and S <= 3 scenes.  The shapes are the
smallest at which each path of the kernel is taken: windows of one pixel, one row and one column, widths of 4k and 4k +- 1, origins in each
of the four 16-byte phases of the frame row, negative origins, windows larger than the frame and wholly outside it, BOP's 3H x 3W form, and
one case sized from the kernel's tile (lc_amd.gtinfo.TILE_W, TILE_H): three tiles in each direction with a ragged last one.

tests/test_gtinfo_oracle.py asserts for every case what tests/test_gpu_gtinfo.py relies on: the margin condition of tests/gtinfo_oracle.py."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import gtinfo_oracle as oracle

DELTA = 0.015
MARGIN = 2.0 ** -30


class Case(NamedTuple):
    name: str
    frame_hw: tuple
    window_hw: tuple
    origins: Optional[np.ndarray]  # (B,2) int32 (x0, y0), or None: full-frame maps
    scene_index: np.ndarray        # (B,) int32; outside [0,S): the row is refused
    K: np.ndarray                  # (B,3,3) float32
    delta: float
    center: tuple
    depth_gt: np.ndarray           # (B,h,w) float32
    depth_test: np.ndarray         # (S,H,W) float32


def stress_camera(frame_hw):
    """Stretch, skew and a principal point off the pixel grid: no ray length is 1."""
    H, W = frame_hw
    f = 1.25 * max(H, W, 8)
    return np.array([[1.15 * f, 0.08 * f, W / 2 + 0.37], [0, 0.87 * f, H / 2 - 0.21], [0, 0, 1]], dtype=np.float32)


def whole_camera(frame_hw, fx=50.0):
    """Integer fx and a whole principal point: n = 1 exactly at pixel (W // 2, H // 2) with pixel centre (0,0)."""
    H, W = frame_hw
    return np.array([[fx, 0, W // 2], [0, fx + 3, H // 2], [0, 0, 1]], dtype=np.float32)


def silhouette(rng, h, w, empty=False):
    d = np.zeros((h, w), dtype=np.float32)
    if empty:
        return d
    cy, cx = rng.uniform(-0.1, 1.1) * h, rng.uniform(-0.1, 1.1) * w
    ry, rx = max(rng.uniform(0.25, 0.8) * h, 1.0), max(rng.uniform(0.25, 0.8) * w, 1.0)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    z = rng.integers(8, 24, size=(h, w)).astype(np.float32) / np.float32(16)
    d[inside] = z[inside]
    odd = inside & (rng.random((h, w)) < 0.08)
    d[odd] = rng.choice(np.asarray([0.0, -0.5, np.nan, np.inf], dtype=np.float32), size=int(odd.sum()))
    return d


def scene(rng, H, W):
    grid = rng.integers(8, 24, size=(H, W)).astype(np.float32) / np.float32(16)
    noise = rng.uniform(0.4, 1.6, size=(H, W)).astype(np.float32)
    d = np.where(rng.random((H, W)) < 0.5, grid, noise).astype(np.float32)
    odd = rng.random((H, W)) < 0.15
    d[odd] = rng.choice(np.asarray([0.0, -1.0, np.nan, np.inf], dtype=np.float32), size=int(odd.sum()))
    return d


def _random(name, seed, frame_hw, window_hw=None, origins=None, scenes=(0,), n_scenes=1, empty=(), K=None, center=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    H, W = frame_hw
    h, w = window_hw or frame_hw
    B = len(scenes)
    K = stress_camera(frame_hw) if K is None else K
    gt = np.stack([silhouette(rng, h, w, empty=b in empty) for b in range(B)])
    test = np.stack([scene(rng, H, W) for _ in range(n_scenes)])
    return Case(name, frame_hw, (h, w), None if origins is None else np.asarray(origins, dtype=np.int32).reshape(B, 2),
                np.asarray(scenes, dtype=np.int32), np.repeat(K[None], B, 0), DELTA, center, gt, test)


def tile_sizes():
    from lc_amd import gtinfo

    return gtinfo.TILE_H, gtinfo.TILE_W


def _hand_cases():
    out = []
    H, W = 7, 9
    # values: one scene whose depth is 1 but for four special pixels; renders 1.005 deep (visible, 5 mm behind) but for their own specials
    test = np.ones((1, H, W), dtype=np.float32)
    test[0, 1, 1], test[0, 1, 2], test[0, 1, 3], test[0, 1, 4] = 0.0, -2.0, np.nan, np.inf
    test[0, 5, :] = 0.9  # a row in front of everything: occluded by 105 mm
    full = np.full((H, W), 1.005, dtype=np.float32)
    odd = full.copy()
    odd[2, 2], odd[2, 3], odd[2, 4], odd[3, 3] = np.nan, -1.0, 0.0, np.inf
    gt = np.stack([np.zeros((H, W), np.float32), full, odd])
    out.append(Case("values-7x9", (H, W), (H, W), None, np.zeros(3, np.int32), np.repeat(stress_camera((H, W))[None], 3, 0), DELTA, (0.0, 0.0), gt, test))
    # the threshold itself, where n = 1: pixel (4,3) of the whole camera.  d_test = 1, delta = 0.25: d_gt = 1.25 is visible (the difference
    # equals delta), the next fp32 above 1.25 is not; the same pair one pixel aside, where n > 1, lies clear of the threshold on both sides
    Kw = whole_camera((H, W))
    test = np.ones((1, H, W), dtype=np.float32)
    at, above = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    at[3, 4], above[3, 4] = 1.25, np.nextafter(np.float32(1.25), np.float32(2))
    at[3, 5], above[3, 5] = 1.2, 1.3
    out.append(Case("threshold-7x9", (H, W), (H, W), None, np.zeros(2, np.int32), np.repeat(Kw[None], 2, 0), 0.25, (0.0, 0.0), np.stack([at, above]), test))
    # edge: a 5 x 6 window at (2,1); one hit in the interior, one on each side, the four corners (each counts once), a full border
    h, w = 5, 6
    test = np.full((1, H, W), 2.0, dtype=np.float32)
    rows = []
    for pix in ([(2, 3)], [(0, 2)], [(4, 3)], [(1, 0)], [(3, 5)], [(0, 0), (0, 5), (4, 0), (4, 5)]):
        m = np.zeros((h, w), np.float32)
        for y, x in pix:
            m[y, x] = 1.0
        rows.append(m)
    out.append(Case("edge-5x6", (H, W), (h, w), np.asarray([[2, 1]] * 6, np.int32), np.zeros(6, np.int32), np.repeat(stress_camera((H, W))[None], 6, 0), DELTA,
                    (0.0, 0.0), np.stack(rows), test))
    ring = np.ones((h, w), np.float32)
    ring[1:-1, 1:-1] = 0
    out.append(Case("ring-5x6", (H, W), (h, w), np.asarray([[2, 1]], np.int32), np.zeros(1, np.int32), stress_camera((H, W))[None], DELTA, (0.0, 0.0), ring[None], test))
    # extreme boxes: a hit at each frame corner, full frame and through a 3H x 3W window
    corners = np.zeros((H, W), np.float32)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1.0
    big = np.zeros((3 * H, 3 * W), np.float32)
    big[H:2 * H, W:2 * W] = corners
    big[0, 0] = big[-1, -1] = 1.0  # and at the window's own corners, far outside the frame
    out.append(Case("corners-7x9", (H, W), (H, W), None, np.zeros(1, np.int32), stress_camera((H, W))[None], DELTA, (0.0, 0.0), corners[None], test))
    out.append(Case("corners-3x-7x9", (H, W), (3 * H, 3 * W), np.asarray([[-W, -H]], np.int32), np.zeros(1, np.int32), stress_camera((H, W))[None], DELTA, (0.0, 0.0),
                    big[None], test))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    th, tw = tile_sizes()
    out = [
        _random("full-7x9", 1, (7, 9), scenes=(0, 1, 1, 0), n_scenes=2),
        _random("full-16x20", 2, (16, 20), scenes=(0, 1, 2, 2, 1, 0), n_scenes=3, center=(0.5, 0.5)),
        _random("full-33x37", 3, (33, 37), scenes=(2, 0, -1, 1, 3), n_scenes=3, empty=(0,)),  # an empty render, two refused rows
        _random("win-1x1", 4, (7, 9), (1, 1), [[0, 0], [8, 6], [4, 3], [-1, 2], [9, 0], [3, 7]], scenes=(0,) * 6),
        _random("win-1x5", 5, (7, 9), (1, 5), [[0, 0], [4, 6], [-2, 3], [6, 2], [1, -1]], scenes=(0, 1, 0, 1, 0), n_scenes=2),
        _random("win-6x1", 6, (7, 9), (6, 1), [[0, 0], [8, 1], [3, -2], [5, 4], [-1, 0]], scenes=(0,) * 5),
        # widths 4k - 1, 4k, 4k + 1; x0 = 0, 1, 2, 3 puts the frame row in each of the four 16-byte phases, -1 and -2 reach out on the left
        _random("win-5x7", 7, (16, 20), (5, 7), [[0, 0], [1, 3], [2, 11], [3, 5], [-1, 2], [-2, 12]], scenes=(0, 1, 0, 1, 0, 1), n_scenes=2),
        _random("win-5x8", 8, (16, 20), (5, 8), [[0, 1], [1, 0], [2, 4], [3, 11], [-3, -2], [14, 13]], scenes=(0, 1, 2, 0, 1, 2), n_scenes=3),
        _random("win-5x9", 9, (16, 20), (5, 9), [[0, 2], [1, 9], [2, 0], [3, 3], [-4, 11], [12, -1]], scenes=(0,) * 6),
        _random("larger-20x25", 10, (7, 9), (20, 25), [[-8, -6], [-3, -2], [0, 0], [-16, -13]], scenes=(0, 1, 0, 5), n_scenes=2),
        # wholly outside: right of, left of, below and above the frame; px_count_all still counts
        _random("outside-4x6", 11, (7, 9), (4, 6), [[11, 1], [-10, 0], [0, 7], [2, -4]], scenes=(0,) * 4),
        _random("bop3x-7x9", 12, (7, 9), (21, 27), [[-9, -7]] * 3, scenes=(0, 0, 1), n_scenes=2, K=whole_camera((7, 9))),
        _random("bop3x-16x20", 13, (16, 20), (48, 60), [[-20, -16]] * 2, scenes=(0, 0)),
        _random("tiles", 14, (2 * th + 5, 2 * tw + 37), None, [[0, 0], [-5, 3]], scenes=(0, 0)),
        _random("far-origin", 15, (7, 9), (4, 6), [[1, 1], [oracle.MAX_ORIGIN + 1, 0], [0, -oracle.MAX_ORIGIN - 1], [oracle.MAX_ORIGIN, 2]], scenes=(0,) * 4),
    ]
    return tuple(out + _hand_cases())


def names():
    return [c.name for c in cases()]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(info (B,12) int32, mask_visib (B,h,w) uint8, margin): the oracle's answer, computed once per process and shared (read-only)."""
    c = case(name)
    return oracle.records(c.depth_gt, c.depth_test, c.K, c.delta, c.scene_index, c.origins, c.center)


@functools.lru_cache(maxsize=None)
def expected_compose(name: str) -> oracle.Composed:
    """The same rows as the instances of their scenes."""
    c = case(name)
    return oracle.compose(c.depth_gt, c.scene_index, c.frame_hw, len(c.depth_test), c.origins)
