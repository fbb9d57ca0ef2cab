"""The symmetry deviation of include/lc_amd_symfind.h, restated in numpy: the query transformed in fp64 operation by operation and rounded
once to fp32, d2 in fp32 with every operation rounded on its own (numpy's elementwise float32 arithmetic), the min with its lowest j, the
max with its lowest query position, the NaN rule, the refusals.  `deviation` is what tests/test_gpu_symfind.py holds the kernels to, bit
for bit; `mistake=` restates one wrong kernel (never what the device is compared with: tests/test_symfind_host.py shows that each one
changes the answer on some case); `scorer` is the `score(jobs)` of lc_amd.symfind's tools on the host."""
from types import SimpleNamespace

import numpy as np

f32, f64 = np.float32, np.float64
TILE, QUERIES, WALK_THREADS, WAVE = 256, 256, 128, 64  # LC_SYMFIND_TILE, LC_SYMFIND_QUERIES, kWalkThreads and the wavefront of lc_symfind.hip

MISTAKES = ("min_le", "max_ge", "highest_tile", "highest_group", "max_before_min", "fp32_transform", "fma", "position_as_index")


def transform(row, v, fp32=False):
    """p[r] = fp32(((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r]) of the vertices v (n,3) float32 under the row-major 3 x 4 `row`."""
    T = f32 if fp32 else f64
    m = np.asarray(row, f64).reshape(3, 4).astype(T)
    x, y, z = (np.asarray(v, f32)[:, c].astype(T) for c in range(3))
    return np.stack([(((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]).astype(f32) for r in range(3)], -1)


def d2(p, v, fma=False):
    """d2 of every p (n,3) against every v (V,3): (n,V) float32."""
    dx, dy, dz = (p[:, None, c] - v[None, :, c] for c in range(3))
    if fma:  # fma(dz, dz, fma(dy, dy, dx*dx)): the products exact in fp64, one rounding per fused step
        xx = dx * dx
        xy = (dy.astype(f64) * dy.astype(f64) + xx.astype(f64)).astype(f32)
        return (dz.astype(f64) * dz.astype(f64) + xy.astype(f64)).astype(f32)
    return (dx * dx + dy * dy) + dz * dz


def _argmin_rows(D, last=False):
    """(n (rows,), j (rows,)) of the d2 matrix D: the minimum of the entries that are no NaN (+inf without one), the lowest (last: highest)
    j that has it, 0 if none has."""
    Dn = np.where(np.isnan(D), f32(np.inf), D)
    n = Dn.min(1) if D.shape[1] else np.full(len(D), f32(np.inf))
    hit = D == n[:, None]
    j = np.where(hit.any(1), (D.shape[1] - 1 - hit[:, ::-1].argmax(1)) if last else hit.argmax(1), 0)
    return n.astype(f32), j.astype(np.int64)


def deviation_row(verts, row, queries=None, mistake=None):
    """(dev2 float32, arg_query, arg_target, skipped) of one transform of one mesh; queries: vertex indices or None for all, in order.  (-1, -1,
    -1) without a vertex or a counted query.  `mistake`: one of MISTAKES, the answer of a wrong kernel with this file's tile sizes."""
    if mistake is not None and mistake not in MISTAKES:
        raise ValueError(mistake)
    v = np.ascontiguousarray(verts, f32).reshape(-1, 3)
    V = len(v)
    if V == 0:  # an empty mesh comes first: its query list is not looked at
        return f32(-1), -1, -1, False
    q = np.arange(V, dtype=np.int64) if queries is None else np.asarray(queries, np.int64).reshape(-1)
    if mistake == "position_as_index":
        q = np.arange(len(q), dtype=np.int64)  # the place in the list taken for the vertex
    valid = (q >= 0) & (q < V)
    skipped = bool((~valid).any())
    pos = np.flatnonzero(valid)
    if len(pos) == 0:
        return f32(-1), -1, -1, skipped
    D = d2(transform(row, v[q[pos]], fp32=mistake == "fp32_transform"), v, fma=mistake == "fma")
    if mistake == "max_before_min":  # every target tile's own max of its mins, merged by max
        n = np.stack([_argmin_rows(D[:, t:t + TILE])[0] for t in range(0, V, TILE)], 1).max(1)
        j = np.zeros(len(pos), np.int64)
    elif mistake == "highest_tile":  # ties across target tiles go to the later tile, inside a tile to the lowest j
        parts = [_argmin_rows(D[:, t:t + TILE]) for t in range(0, V, TILE)]
        n = np.stack([p[0] for p in parts], 1)
        best = n.min(1)
        t = n.shape[1] - 1 - (n == best[:, None])[:, ::-1].argmax(1)
        n, j = best, np.array([parts[tt][1][i] + tt * TILE for i, tt in enumerate(t)])
        j = np.where((D == n[:, None]).any(1), j, 0)
    else:
        n, j = _argmin_rows(D, last=mistake == "min_le")
    top = n.max()
    tied = np.flatnonzero(n == top)
    if mistake == "max_ge":
        w = tied[-1]
    elif mistake == "highest_group":  # ties across workgroups (query tiles) go to the later one, inside to the lowest position
        w = min(tied.tolist(), key=lambda a: (-(pos[a] // QUERIES), pos[a]))
    else:
        w = tied[0]
    return f32(top), int(q[pos[w]]), int(j[w]), skipped


def deviation(meshes, table, mesh_index, row_off, row_k, query_idx=None, query_off=None, query_n=None, *, max_k=None, max_queries=None, mistake=None):
    """lc_amd.symfind.deviation on the host: meshes = [verts (V,3)]; -> SimpleNamespace(dev2, arg_query, arg_target (G,max_k), dev, info)."""
    table = np.asarray(table, f64).reshape(-1, 12)
    G = len(mesh_index)
    max_k = max(min(int(max(row_k)) if max_k is None else max_k, len(table)), 1)
    if query_idx is not None:
        query_idx = np.asarray(query_idx, np.int64).reshape(-1)
        max_queries = max(min(int(max(query_n)) if max_queries is None else max_queries, len(query_idx)), 1)
    dev2, aq, at, info = np.full((G, max_k), -1, f32), np.full((G, max_k), -1, np.int32), np.full((G, max_k), -1, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        mi, ro, rk = int(mesh_index[g]), int(row_off[g]), int(row_k[g])
        bad = not 0 <= mi < len(meshes) or ro < 0 or not 0 <= rk <= max_k or ro + rk > len(table)
        q = None
        if not bad and query_idx is not None:
            qo, qn = int(query_off[g]), int(query_n[g])
            bad = qo < 0 or not 0 <= qn <= max_queries or qo + qn > len(query_idx)
            q = None if bad else query_idx[qo:qo + qn]
        if bad:
            info[g] = -1
            continue
        for k in range(rk):
            dev2[g, k], aq[g, k], at[g, k], skipped = deviation_row(meshes[mi], table[ro + k], q, mistake)
            if skipped:
                info[g] = 1
    with np.errstate(invalid="ignore"):
        return SimpleNamespace(dev2=dev2, arg_query=aq, arg_target=at, dev=np.sqrt(dev2.astype(f64)), info=info)


def dev2_rows_fast(verts, rows, queries=None, near=8):
    """dev2 (K,) float32 of many rows of one mesh, for the tools' shapes: the `near` nearest vertices by a k-d tree in float64 are the only
    targets whose fp32 d2 is evaluated.  Equal to deviation_row's dev2 wherever the fp32 minimum is among them (finite coordinates, no
    more than `near` vertices within rounding of the nearest); tests/test_symfind_host.py holds it to the definition on its shapes."""
    from scipy.spatial import cKDTree

    v = np.ascontiguousarray(verts, f32).reshape(-1, 3)
    q = v if queries is None else v[np.asarray(queries, np.int64)]
    tree, near = cKDTree(v.astype(f64)), min(near, len(v))
    out = np.empty(len(rows), f32)
    for k, row in enumerate(np.asarray(rows, f64).reshape(-1, 12)):
        p = transform(row, q)
        idx = tree.query(p.astype(f64), k=near)[1].reshape(len(p), near)
        dx, dy, dz = (p[:, None, c] - v[idx, c] for c in range(3))
        out[k] = ((dx * dx + dy * dy) + dz * dz).min(1).max()
    return out


def scorer(meshes, fast=True):
    """The `score(jobs)` of lc_amd.symfind.check_symmetries / propose_symmetries on the host: meshes = [verts]."""
    def score(jobs):
        out = []
        for m, rows, q in jobs:
            rows = np.asarray(rows, f64).reshape(-1, 12)
            d = dev2_rows_fast(meshes[m], rows, q) if fast else np.array([deviation_row(meshes[m], r, q)[0] for r in rows], f32)
            out.append(np.sqrt(d.astype(f64)))
        return out

    return score
