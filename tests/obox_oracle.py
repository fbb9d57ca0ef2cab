"""The oriented model box of include/lc_amd_obox.h, restated in numpy: the tables, the candidates in fp64 operation by operation, the fp32
score, the winner rule, the final pass.  `oriented_box_host` is what tests/test_gpu_obox.py holds the kernels to, bit for bit; the host
tests check the properties of the definition on it.  Nothing here imports lc_amd."""
import math
from typing import NamedTuple

import numpy as np

STEP0 = math.pi / 20.0  # 9 degrees
GRID_RADIUS = 7
AXIS_LEVEL0_COUNT = 10
DEFAULT_LEVELS = 6
F32 = np.float32


class Box(NamedTuple):
    xform: np.ndarray        # (n,4,4) float32
    noc_scale: np.ndarray    # (n,3) float32
    volume: np.ndarray       # (n,) float32
    aabb_volume: np.ndarray  # (n,) float32
    path: np.ndarray         # (n,levels+1) int32
    info: np.ndarray         # (n,) int32
    scores: list             # per mesh, per level: the (n_cand,) float32 scores (the oracle's own; the library does not return them)


def _n2(p):
    return p[0] * p[0] + p[1] * p[1] + p[2] * p[2]


def level_vectors(axis, level):
    """The integer rotation vectors of a level's table, in the table's order."""
    if axis is None:
        if level == 0:
            span = range(-GRID_RADIUS, GRID_RADIUS + 1)
            pts = [(i, j, k) for i in span for j in span for k in span if i * i + j * j + k * k <= GRID_RADIUS ** 2]
        else:
            pts = [(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)]
        return sorted(pts, key=lambda p: (_n2(p), p))
    unit = [1 if a == axis else 0 for a in range(3)]
    if level == 0:
        return [tuple(s * u for u in unit) for s in range(AXIS_LEVEL0_COUNT)]
    return sorted([tuple(s * u for u in unit) for s in range(-2, 3)], key=lambda p: (_n2(p), p))


def level_quats(axis, level):
    s = STEP0 / 2.0 ** level
    out = []
    for p in level_vectors(axis, level):
        n2 = _n2(p)
        if n2 == 0:
            out.append((1.0, 0.0, 0.0, 0.0))
            continue
        root = math.sqrt(float(n2))
        h = (s * root) * 0.5
        f = math.sin(h) / root
        out.append((math.cos(h), p[0] * f, p[1] * f, p[2] * f))
    return np.asarray(out, np.float64)


def candidate_quat(b, d, c):
    """Candidate c: the base as it is, or normalise(d (x) b).  Python floats are IEEE fp64, one rounding per operation."""
    bw, bx, by, bz = (float(x) for x in b)
    if c == 0:
        return (bw, bx, by, bz)
    dw, dx, dy, dz = (float(x) for x in d)
    pw = ((dw * bw - dx * bx) - dy * by) - dz * bz
    px = ((dw * bx + dx * bw) + dy * bz) - dz * by
    py = ((dw * by - dx * bz) + dy * bw) + dz * bx
    pz = ((dw * bz + dx * by) - dy * bx) + dz * bw
    n = math.sqrt(((pw * pw + px * px) + py * py) + pz * pz)
    return (pw / n, px / n, py / n, pz / n)


def quat_matrix(q):
    """(3,3) float32: the fp64 formula, each entry rounded once."""
    w, x, y, z = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    return np.asarray(R, np.float64).astype(F32)


def extents(R, v):
    """lo, hi (..., 3) float32 of p = R v for matrices R (..., 3, 3) and vertices v (V, 3): every product and sum rounded on its own (numpy
    evaluates an array expression operation by operation), a zero of either sign as +0."""
    R, v = np.asarray(R, F32), np.asarray(v, F32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        p = (R[..., 0, None] * x + R[..., 1, None] * y) + R[..., 2, None] * z  # (..., 3, V)
        lo, hi = np.fmin.reduce(p, axis=-1) + F32(0), np.fmax.reduce(p, axis=-1) + F32(0)
    return lo.astype(F32), hi.astype(F32)


def score(R, v):
    lo, hi = extents(R, v)
    with np.errstate(all="ignore"):
        e = hi - lo
        return ((e[..., 0] * e[..., 1]) * e[..., 2]).astype(F32)


def level_matrices(base, axis, level):
    table = level_quats(axis, level)
    quats = [candidate_quat(base, table[c], c) for c in range(len(table))]
    return quats, np.stack([quat_matrix(q) for q in quats])


def winner(scores):
    """Lowest score, ties to the lowest index: the minimum of (score bits << 32 | index), as the library takes it."""
    keys = (np.asarray(scores, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(scores), dtype=np.uint64)
    return int(keys.min() & np.uint64(0xFFFFFFFF))


def oriented_box_one(v, axis=None, levels=DEFAULT_LEVELS):
    v = np.asarray(v, F32).reshape(-1, 3)
    base, path, per_level = (1.0, 0.0, 0.0, 0.0), [], []
    volume = aabb = F32(0)
    for level in range(levels + 1):
        quats, mats = level_matrices(base, axis, level)
        s = np.concatenate([score(mats[a:a + 256], v) for a in range(0, len(mats), 256)])
        k = winner(s)
        base, volume = quats[k], s[k]
        if level == 0:
            aabb = s[0]
        path.append(k)
        per_level.append(s)
    R = quat_matrix(base)
    lo, hi = extents(R, v)
    with np.errstate(all="ignore"):
        c = (lo + hi) * F32(0.5)
        scale = np.fmax(hi - c, c - lo)
    X = np.zeros((4, 4), F32)
    X[:3, :3], X[:3, 3], X[3, 3] = R, -c, 1
    return X, scale.astype(F32), F32(volume), F32(aabb), np.asarray(path, np.int32), np.int32(0 if np.isfinite(v).all() else 1), per_level


def oriented_box_host(meshes, axis=None, levels=DEFAULT_LEVELS) -> Box:
    """`meshes`: a list of (V,3) vertex arrays (or (verts, faces) pairs)."""
    rows = [oriented_box_one(m[0] if isinstance(m, tuple) else m, axis, levels) for m in meshes]
    return Box(*(np.stack([r[k] for r in rows]) for k in range(6)), [r[6] for r in rows])


def transformed(X, v):
    """fl(R v - c) in fp32 as the enclosure inequality states it: p by the score's rule, then one subtraction of c = -t."""
    X, v = np.asarray(X, F32), np.asarray(v, F32)
    R, c = X[:3, :3], -X[:3, 3]
    p = (R[:, 0, None] * v[:, 0] + R[:, 1, None] * v[:, 1]) + R[:, 2, None] * v[:, 2]
    return (p - c[:, None]).T
