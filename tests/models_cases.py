"""The numpy restatement of lc_amd.models' definitions (include/lc_amd_models.h, `lc_model_prepare_f32`) and the case list of its tests.

numpy's elementwise float32 operations round one at a time, so every value below is the definition's own: the GPU tests compare
bit for bit.
"""
from types import SimpleNamespace

import numpy as np

f32 = np.float32


def d2(a, b):
    """((ax-bx)^2 + (ay-by)^2) + (az-bz)^2 in float32, every operation rounded on its own; a, b (...,3) broadcast."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def extents(v):
    v = np.asarray(v, f32)
    return v.min(0), v.max(0)


def diameter(v, rows=512):
    """(diameter float32, (i, j)): the largest d2 over i < j, ties to the smallest i, then the smallest j; sqrt correctly rounded."""
    v = np.asarray(v, f32)
    V = len(v)
    if V == 1:
        return f32(0), (0, 0)
    best, pair = f32(-1), (0, 0)
    col = np.arange(V)
    for i0 in range(0, V, rows):
        blk = d2(v[i0:i0 + rows, None, :], v[None, :, :])
        blk = np.where(col[None, :] > np.arange(i0, min(V, i0 + rows))[:, None], blk, f32(-1))
        k = int(blk.argmax())  # first occurrence in row-major order: smallest i, then smallest j
        i, j = divmod(k, V)
        if blk[i, j] > best:   # strictly: an earlier block's pair keeps a tie
            best, pair = blk[i, j], (i0 + i, j)
    return np.sqrt(best, dtype=f32), pair


def fps(v, count):
    """(index (count,) int32, points (count,3) float32): seeded at the box centre, argmax ties to the smallest index."""
    v = np.asarray(v, f32)
    if count > len(v):
        raise ValueError("count > V")
    lo, hi = extents(v)
    c = (lo + hi) * f32(0.5)
    mind = d2(v, c)
    idx = np.empty(count, np.int32)
    for n in range(count):
        k = int(mind.argmax())  # first maximum
        idx[n] = k
        mind = np.minimum(mind, d2(v, v[k]))
    return idx, v[idx]


def prepare_oracle(meshes, fps_count=0, *, want_diameter=True):
    """`lc_amd.models.prepare` on the host: `meshes` has `.host` = [(verts, faces)] -- returns numpy arrays in a ModelInfo-shaped object."""
    lo, hi, dia, pair, pts, index = [], [], [], [], [], []
    for v, _ in meshes.host:
        a, b = extents(v)
        lo.append(a)
        hi.append(b)
        if want_diameter:
            d, p = diameter(v)
            dia.append(d)
            pair.append(p)
        if fps_count:
            i, q = fps(v, fps_count)
            index.append(i)
            pts.append(q)
    from lc_amd.models import ModelInfo

    return ModelInfo(np.stack(lo), np.stack(hi), np.asarray(dia, f32) if want_diameter else None, np.asarray(pair, np.int32) if want_diameter else None,
                     np.stack(pts) if fps_count else None, np.stack(index) if fps_count else None)


def host_set(meshes, obj_ids=None):
    """What prepare_oracle reads, standing in for a MeshSet where there is no device."""
    meshes = [(np.asarray(v, f32), f) for v, f in meshes]
    return SimpleNamespace(host=meshes, obj_ids=list(range(len(meshes))) if obj_ids is None else list(obj_ids), n_meshes=len(meshes))


def cloud(V, seed, scale=0.1, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((V, 3)) * scale + offset).astype(f32)


def cube_with_duplicates():
    """The eight corners of a cube, every corner three times, shuffled by a fixed permutation: four diagonals of the same length (and
    nine index pairs for each), eight equidistant first picks -- every tie rule fires."""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32) * f32(0.5)
    v = np.concatenate([c, c, c])
    return v[np.random.default_rng(3).permutation(len(v))]


def collinear(V=97):
    t = np.linspace(-1, 1, V).astype(f32)
    return np.stack([t * f32(0.3), t * f32(-0.2), t * f32(0.7)], -1).astype(f32)


FACES0 = np.zeros((0, 3), np.int32)


def named_cases(tile, resident):
    """name -> (verts, fps counts, want_diameter): the sizes around every boundary of the kernels.  `tile` / `resident` are
    lc_amd.models.DIAM_TILE / FPS_RESIDENT.  The two meshes around the resident limit skip the diameter (its kernels do not know
    that limit, and their oracle is 7e7 pairs each)."""
    cases = {}
    for V in (1, 2, 3, 63, 64, 65):
        cases[f"V{V}"] = (cloud(V, 100 + V), (1, min(16, V), V), True)
    for name, V in (("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1), ("2tiles+1", 2 * tile + 1), ("rows", 1100)):
        cases[name] = (cloud(V, 200 + V), (16,), True)
    cases["resident"] = (cloud(resident, 7), (16,), False)
    cases["resident+1"] = (cloud(resident + 1, 8), (16,), False)
    cases["cube_duplicates"] = (cube_with_duplicates(), (24,), True)
    cases["collinear"] = (collinear(), (16,), True)
    cases["mm_offset"] = (cloud(300, 9, scale=40.0, offset=1.0e4), (16,), True)
    return cases
