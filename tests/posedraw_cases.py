"""The drawn scene poses' case list (TEST INFRASTRUCTURE ONLY), shared by tests/test_posedraw_host.py and tests/test_gpu_posedraw.py: built so
that the host contract alone (`posedraw.draw_scene_poses_host`) reaches every branch -- tests/test_posedraw_host.py asserts that it does
-- and the device is then compared with it bit for bit.  Lengths are metres; the cameras are lc_amd.synth's `bop` (fx != fy) and `stress`
(fx != fy and skew) of tests/camera_cases.py, without the in-plane rotation (the contract reads K00, K01, K02, K11, K12).

    one              S = 1, M = 1
    s3-m1/-m2/-m64   S = 3 with M = 1, 2 and 64 (a full wave of slots), radii small enough that every slot is placed at try 0
    crowded          M = 8, large radii in a narrow depth range and a small box: retries, slots without room, and a small object placed
                     behind a slot that found none
    refusals         empty slots between filled ones, unknown meshes on both sides, a sphere that reaches the near plane, a camera that
                     is not finite and one with K11 = 0 (per-scene cameras)
    mixed-radii      five radii over two decades
    flat-z           z_min == z_max
    big-box          a centre_box larger than the frame
    ids              scene ids that are not contiguous, a negative one, and one repeated in two batch positions
    seed-high        seeds with a non-zero upper half
    cam-bop/-stress  the two cameras (every other case uses `stress`)
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from lc_amd import synth
from lc_amd.posedraw import PoseDrawConfig, draw_scene_poses_host
from tests import camera_cases

FRAME = (480, 640)
NEAR = 0.01


class Case(NamedTuple):
    name: str
    cfg: PoseDrawConfig
    seed: int
    scene_ids: np.ndarray   # (S,) int32
    mesh_index: np.ndarray  # (S,M) int32
    radius: np.ndarray      # (n_meshes,) float32
    cam_K: np.ndarray       # (3,3) or (S,3,3) float32


def camera(name: str, f=600.0) -> np.ndarray:
    """(3,3) float32: lc_amd.synth's camera `name` at focal length f around the frame's centre, no in-plane rotation."""
    assert name in camera_cases.CAMERAS
    K = synth.crop_camera(torch.tensor([f], dtype=torch.float64), torch.zeros(1, dtype=torch.float64), FRAME[1] / 2, FRAME[0] / 2, name)
    return K[0].numpy().astype(np.float32)


FRAME_BOX = (0.0, 0.0, float(FRAME[1]), float(FRAME[0]))
ROOMY = PoseDrawConfig(z_range=(0.5, 1.5), centre_box=FRAME_BOX, gap=0.002, near=NEAR)
SMALL_RADII = np.array([0.001, 0.0015, 0.002], dtype=np.float32)


def _ids(S, first=0):
    return np.arange(first, first + S, dtype=np.int32)


def _round_robin(S, M, n):
    return ((np.arange(S)[:, None] * M + np.arange(M)[None]) % n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    stress = camera("stress")
    if name == "one":
        return Case(name, ROOMY, 1, _ids(1), np.zeros((1, 1), np.int32), np.array([0.05], np.float32), stress)
    if name in ("s3-m1", "s3-m2", "s3-m64"):
        M = int(name.split("m")[1])
        return Case(name, ROOMY, 20 + M, _ids(3, 7), _round_robin(3, M, 3), SMALL_RADII, stress)
    if name == "crowded":
        cfg = PoseDrawConfig(z_range=(0.5, 0.56), centre_box=(260.0, 180.0, 380.0, 300.0), gap=0.004, near=NEAR)
        mi = np.array([[0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 1, 0, 1], [0, 1, 0, 0, 0, 0, 1, 1]], np.int32)
        return Case(name, cfg, 77, _ids(3), mi, np.array([0.035, 0.004], np.float32), stress)
    if name == "refusals":
        bad_K, flat_K = stress.copy(), stress.copy()
        bad_K[0, 2] = np.inf
        flat_K[1, 1] = 0.0
        nan_K = stress.copy()
        nan_K[2, 0] = np.nan  # an entry the contract never reads otherwise
        mi = np.array([[0, -1, 1, 7, -5, 2], [-1, -1, 0, 1, -1, 0], [0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0], [0, 0, 1, 1, 2, -1]], np.int32)
        return Case(name, ROOMY, 5, _ids(5), mi, np.array([0.03, 0.02, 0.49], np.float32), np.stack((stress, stress, bad_K, flat_K, nan_K)))  # 0.5 - 0.49 == near
    if name == "mixed-radii":
        cfg = PoseDrawConfig(z_range=(0.6, 0.9), centre_box=(200.0, 150.0, 440.0, 330.0), gap=0.01, near=NEAR)
        return Case(name, cfg, 31, _ids(2), _round_robin(2, 5, 5), np.array([0.002, 0.02, 0.08, 0.2, 0.0005], np.float32), stress)
    if name == "flat-z":
        cfg = PoseDrawConfig(z_range=(0.75, 0.75), centre_box=FRAME_BOX, gap=0.0, near=NEAR)
        return Case(name, cfg, 9, _ids(2), _round_robin(2, 6, 2), np.array([0.05, 0.08], np.float32), stress)
    if name == "big-box":
        cfg = PoseDrawConfig(z_range=(0.5, 1.0), centre_box=(-200.0, -100.0, 900.0, 650.0), gap=0.0, near=NEAR)
        return Case(name, cfg, 13, _ids(2), _round_robin(2, 8, 2), np.array([0.05, 0.08], np.float32), stress)
    if name == "ids":
        return Case(name, ROOMY, 3, np.array([5, 1000000, -3, 5, 2 ** 31 - 1], np.int32), _round_robin(1, 4, 3).repeat(5, 0), np.array([0.05, 0.08, 0.03], np.float32), stress)
    if name == "seed-high":
        return Case(name, ROOMY, 2 ** 63 + 12345, _ids(2), _round_robin(2, 3, 3), np.array([0.05, 0.08, 0.03], np.float32), stress)
    if name in ("cam-bop", "cam-stress"):
        return Case(name, ROOMY, 7 * 2 ** 32 + 1, _ids(2, 40), _round_robin(2, 4, 3), np.array([0.05, 0.08, 0.03], np.float32), camera(name[4:], 550.0))
    raise KeyError(name)


NAMES = ("one", "s3-m1", "s3-m2", "s3-m64", "crowded", "refusals", "mixed-radii", "flat-z", "big-box", "ids", "seed-high", "cam-bop", "cam-stress")


@functools.lru_cache(maxsize=None)
def reference(name: str, seed_offset: int = 0):
    """(ScenePoses, fp64 positions) of the host contract at the case's seed + seed_offset: computed once per process, shared, read-only."""
    c = build(name)
    return draw_scene_poses_host(c.cfg, (c.seed + seed_offset) % 2 ** 64, c.scene_ids, c.mesh_index, c.radius, c.cam_K, return_fp64=True)
