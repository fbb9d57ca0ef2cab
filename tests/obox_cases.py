"""The meshes of the oriented-box tests and their oracle results, computed once per (mesh, mode, levels) and shared: tests/test_obox_host.py
checks the conditions the GPU cases rely on, tests/test_gpu_obox.py holds the kernels to the results."""
import functools
import math

import numpy as np

from tests import obox_oracle as oracle

TILE, SPLIT = 256, 1024  # LC_OBOX_TILE, LC_OBOX_SPLIT (tests/test_obox_host.py holds them to the header)
# one wave's edge, the LDS tile's edge, the vertex split's edge (1025: two workgroups share a mesh), and three chunks with a ragged last tile
SIZES = (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT + 300)
BOX_HALF = (0.031, 0.052, 0.11)
# rotation vectors in degrees that lie on no grid point of any level
OFF_GRID = ((13.7, -4.1, 22.3), (3.3, 41.9, -17.2), (-28.6, 9.4, 5.5), (0.0, 0.0, 33.3))


def rotation(rotvec_deg):
    r = np.radians(np.asarray(rotvec_deg, np.float64))
    a = float(np.linalg.norm(r))
    if a == 0:
        return np.eye(3)
    k = r / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


@functools.lru_cache(maxsize=None)
def cloud(V, seed=0):
    """V vertices of a Gaussian cloud three times as long as wide, turned off the axes (a search that has something to find), off-centre."""
    rng = np.random.default_rng(1000 * seed + V)
    v = rng.standard_normal((V, 3)) * (0.02, 0.045, 0.07)
    v = v @ rotation((25.0, -40.0, 31.0)).T + (0.01, -0.02, 0.005)
    v = v.astype(np.float32)
    v.setflags(write=False)
    return v


def box_corners(half=BOX_HALF):
    return np.array([[sx * half[0], sy * half[1], sz * half[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def turned_box(rotvec_deg, half=BOX_HALF):
    """The eight corners of a box turned by a rotation vector, rounded to fp32."""
    return (box_corners(half) @ rotation(rotvec_deg).T).astype(np.float32)


def tie_cube():
    """A cube turned by 45 degrees about z, its corners rounded to fp32: the set is mirror-symmetric in y, so the level-0 candidates that turn
    it back by +45 and by -45 degrees about z see mirrored point sets and score the same bits."""
    r = np.float32(math.sqrt(2.0))
    return np.array([[sx * r, 0, sz] for sx in (-1, 1) for sz in (-1, 1)] + [[0, sy * r, sz] for sy in (-1, 1) for sz in (-1, 1)], np.float32)


def flat(V=40):
    v = np.array(cloud(V, seed=3))
    v[:, 1] = np.float32(0.25)
    return v


@functools.lru_cache(maxsize=None)
def mesh(name):
    kind, _, arg = name.partition(":")
    if kind == "cloud":
        return cloud(int(arg))
    if kind == "offgrid":
        return turned_box(OFF_GRID[int(arg)])
    v = {"tie-cube": tie_cube, "flat": flat}[kind]()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(name, axis=None, levels=oracle.DEFAULT_LEVELS):
    """The oracle's result for one mesh alone (every field has a leading axis of 1)."""
    return oracle.oriented_box_host([mesh(name)], axis, levels)


FIELDS = ("xform", "noc_scale", "volume", "aabb_volume", "path", "info")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
