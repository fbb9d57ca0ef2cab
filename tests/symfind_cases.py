"""The cases of the symmetry-deviation tests, shared by tests/test_symfind_host.py (which checks the conditions they rely on against the numpy
oracle) and tests/test_gpu_symfind.py (which holds the kernels to the oracle bit for bit): calls of `deviation` at the edges of the target
tile T and the query tile Q, lattice meshes with planted exact ties for every merge level, and the shapes of the two tools with the eps
each is judged at."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from lc_amd.symmetry import rodrigues
from tests import models_cases
from tests import symfind_oracle as oracle

f32, f64 = np.float32, np.float64
T, Q = oracle.TILE, oracle.QUERIES
IDENTITY = np.eye(3, 4).reshape(12)
STEP = 2.0 ** -models_cases.LATTICE_BITS


def random_rows(K, seed, shift=0.02):
    """K rows: the identity, then rotations about random axes by random angles with small translations."""
    rng = np.random.default_rng(seed)
    rows = [IDENTITY]
    for _ in range(K - 1):
        a = rng.standard_normal(3)
        R = rodrigues(a / np.linalg.norm(a), rng.uniform(-math.pi, math.pi))
        rows.append(np.concatenate((R, rng.standard_normal((3, 1)) * shift), 1).reshape(12))
    return np.stack(rows)


class Call(SimpleNamespace):
    """meshes [verts], table (Ktot,12), mesh_index, row_off, row_k, and query_idx / query_off / query_n (all None: every vertex)."""

    def args(self):
        return (self.table, self.mesh_index, self.row_off, self.row_k, self.query_idx, self.query_off, self.query_n)


def call(meshes, jobs):
    """jobs = [(mesh, rows (K,12), query list or None)]: a table of the rows back to back; query lists for all jobs if any has one."""
    ks = [len(r) for _, r, _ in jobs]
    lists = None
    if any(q is not None for _, _, q in jobs):
        lists = [np.arange(len(meshes[m]), dtype=np.int32) if q is None else np.asarray(q, np.int32) for m, _, q in jobs]
    starts = lambda n: np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int32)
    return Call(meshes=meshes, table=np.concatenate([r for _, r, _ in jobs]), mesh_index=np.array([m for m, _, _ in jobs], np.int32), row_off=starts(ks),
                row_k=np.array(ks, np.int32), query_idx=None if lists is None else np.concatenate(lists),
                query_off=None if lists is None else starts([len(l) for l in lists]), query_n=None if lists is None else np.array([len(l) for l in lists], np.int32))


SIZES = (1, 2, T - 1, T, T + 1, 2 * T + 1)
QUERY_COUNTS = (Q - 1, Q, Q + 1)
cloud = models_cases.cloud


def planted(V, seed, plants, n_queries):
    """A lattice mesh with exact planted ties, and the query list and row that meet them.  The row is the translation by 16 steps along x.
    `plants` = [(query position, [target indices])], at most three: plant m's query vertex sits 100 steps out on axis m, lands at
    100 e_m + 16 e_x, and its targets sit 8 steps from there along +-e_(m+1) (a third and fourth along +-e_(m+2)): d2 = 64 steps^2 each, an
    exact tie, nearer than the query's own vertex (256).  The other vertices are lattice points within 24 steps of the origin, in pairs
    (a, a + 16 e_x); the other queries are drawn from the a's (with repeats) and land exactly on their partners: their minima are 0 and the
    planted ones the strict maximum.  All coordinates are integers below 2^8 in steps of 2^-8: every difference, square and sum is exact."""
    v = np.zeros((V, 3), f32)
    rng = np.random.default_rng(seed + 1)
    taken = {j for _, ts in plants for j in ts}
    free = [i for i in range(V) if i not in taken]
    rest = free[len(plants):]
    a = models_cases.lattice(-(-len(rest) // 2), seed, 24) / f32(STEP)
    v[rest[0::2]] = a
    v[rest[1::2]] = a[:len(rest) // 2] + np.array([16, 0, 0], f32)
    queries = rng.choice(rest[0:2 * (len(rest) // 2):2], size=n_queries).astype(np.int32)
    for m, (pos, targets) in enumerate(plants):
        qi = free[m]
        v[qi] = 0
        v[qi, m] = 100
        land = v[qi] + np.array([16, 0, 0], f32)
        for n, j in enumerate(targets):
            v[j] = land
            v[j, (m + 1 + n // 2) % 3] += 8 * (1 - 2 * (n % 2))
        queries[pos] = qi
    row = np.concatenate((np.eye(3), [[16 * STEP], [0], [0]]), 1).reshape(12)
    return (v * f32(STEP)).astype(f32), queries, row


# name -> (V, plants, number of queries, the mistakes of the oracle that must change the answer, what the case forces)
TIED = {
    "targets-one-thread": (T + 40, [(2, [7, 7 + 256])], 20, ("min_le", "highest_tile"), "two tied targets 256 apart: one thread of the finish, two tiles of the walk"),
    "targets-waves": (T - 1, [(0, [3, 70])], 9, ("min_le",), "two tied targets of one tile in different waves"),
    "targets-tiles": (2 * T + 1, [(4, [T + 9, 2 * T])], 30, ("min_le", "highest_tile"), "two tied targets in the second and the third tile"),
    "targets-four": (T + 1, [(1, [200, 100, T, 50])], 5, ("min_le", "highest_tile"), "four tied targets, the lowest neither first nor last in plant order"),
    "queries-wave": (T, [(3, [10, 20]), (40, [30, 41])], 60, ("max_ge",), "two queries with equal minima in one wave"),
    "queries-slots": (2 * T, [(128 + 3, [10, 20]), (3, [30, 41])], 200, ("max_ge",), "equal minima in the two slots of one lane"),
    "queries-waves": (2 * T, [(70, [10, 20]), (5, [30, 41]), (127, [50, 51])], 128, ("max_ge",), "equal minima across the waves of a workgroup"),
    "queries-groups": (2 * T + 1, [(Q + 20, [10, 20]), (10, [30, 41]), (2 * Q + 1, [50, 51])], 2 * Q + 2, ("max_ge", "highest_group"), "equal minima across three workgroups"),
}


@functools.lru_cache(None)
def tied(name):
    V, plants, nq, mistakes, forces = TIED[name]
    v, queries, row = planted(V, 40 + sorted(TIED).index(name), plants, nq)
    return SimpleNamespace(call=call([v], [(0, np.stack([IDENTITY, row]), queries)]), plants=plants, mistakes=mistakes, forces=forces)


def lattice_box(nx=3, ny=4, nz=2):
    """A centred box of lattice points with odd coordinates (no zero): -(2n-1)..(2n-1) steps in twos along each axis."""
    ax = lambda n: np.arange(-(2 * n - 1), 2 * n, 2)
    g = np.stack(np.meshgrid(ax(nx), ax(ny), ax(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g[np.random.default_rng(5).permutation(len(g))] * STEP).astype(f32)


def half_turn_rows():
    """The half turns about x, y, z through the origin as `rodrigues` gives them: sin(pi) = 1.2e-16 stands in four entries of each."""
    return np.stack([np.concatenate((rodrigues(np.eye(3)[a], math.pi), np.zeros((3, 1))), 1).reshape(12) for a in range(3)])


@functools.lru_cache(None)
def named(name):
    """The calls of the kernel tests by name."""
    if name.startswith("size:"):
        V = int(name[5:])
        return call([cloud(V, 300 + V)], [(0, random_rows(3, V), None)])
    if name.startswith("queries:"):
        n = int(name[8:])
        return call([cloud(2 * T + 1, 77)], [(0, random_rows(3, n), np.random.default_rng(n).permutation(2 * T + 1)[:n])])
    if name == "identity":
        return call([cloud(T + 1, 78)], [(0, IDENTITY[None], None)])
    if name in ("jobs", "jobs-shuffled"):
        meshes = [cloud(65, 1), cloud(2 * T + 1, 2), cloud(T, 3), cloud(1, 4)]
        rng = np.random.default_rng(9)
        jobs = [(1, random_rows(5, 11), rng.permutation(2 * T + 1)[:Q + 1]), (0, random_rows(2, 12), None), (2, random_rows(1, 13), np.arange(T)[::-1]),
                (3, random_rows(3, 14), [0, 0, 0]), (1, random_rows(4, 15), None), (2, random_rows(7, 16), rng.integers(0, T, 2 * Q + 5))]
        if name == "jobs-shuffled":
            jobs = [jobs[i] for i in JOB_SHUFFLE]
        return call(meshes, jobs)
    if name == "repeats-descending":
        q = np.concatenate((np.arange(T + 1)[::-1], [5, 5, 5, T, T]))
        return call([cloud(T + 1, 79)], [(0, random_rows(3, 17), q)])
    if name == "all-identical":
        v = np.tile(np.array([3, -5, 7], f32) * f32(STEP), (300, 1))
        shift = np.concatenate((np.eye(3), [[4 * STEP], [0], [-3 * STEP]]), 1).reshape(12)
        return call([v], [(0, np.stack([IDENTITY, shift]), None)])
    if name == "half-turns":
        return call([lattice_box()], [(0, half_turn_rows(), None)])
    raise KeyError(name)


JOB_SHUFFLE = (4, 2, 5, 0, 3, 1)
NAMES = tuple(f"size:{V}" for V in SIZES) + tuple(f"queries:{n}" for n in QUERY_COUNTS) + ("identity", "jobs", "jobs-shuffled", "repeats-descending",
                                                                                          "all-identical", "half-turns")


@functools.lru_cache(None)
def reference(name):
    """The oracle's answer of a named or tied call, computed once."""
    c = tied(name).call if name in TIED else named(name)
    return oracle.deviation(c.meshes, *c.args())


FIELDS = ("dev2", "arg_query", "arg_target", "info")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the tools' shapes (coordinates in mm) ----

def _box_surface(hx, hy, hz, n):
    """The points of an n x n grid on each face of the box of half-extents (hx, hy, hz): symmetric under every symmetry of the box."""
    u = np.linspace(-1.0, 1.0, n)
    a, b = (m.reshape(-1) for m in np.meshgrid(u, u, indexing="ij"))
    pts = []
    for axis in range(3):
        for s in (-1.0, 1.0):
            p = np.empty((len(a), 3))
            p[:, axis] = s
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a, b
            pts.append(p)
    pts = np.unique(np.concatenate(pts).round(12), axis=0) * np.array([hx, hy, hz])
    return pts[np.random.default_rng(21).permutation(len(pts))]


def _revolution(profile, meridians=48):
    """The surface of revolution of the (radius, height) profile about z, sampled on `meridians` meridians."""
    phi = 2.0 * math.pi * np.arange(meridians) / meridians
    pts = [(r * math.cos(p), r * math.sin(p), h) for r, h in profile for p in (phi if r > 0 else phi[:1])]
    pts = np.asarray(pts)
    return pts[np.random.default_rng(22).permutation(len(pts))]


def _scalene(V=400):
    rng = np.random.default_rng(23)
    return rng.standard_normal((V, 3)) * np.array([20.0, 35.0, 55.0]) + rng.standard_normal((V, 1)) * np.array([9.0, -4.0, 6.0])


GENERIC_TURN = rodrigues(np.array([2.0, -1.0, 3.0]) / math.sqrt(14.0), 0.83)
GENERIC_SHIFT = np.array([31.0, -17.0, 12.0])
_FLIP_PROFILE = [(12.0 + 18.0 * math.cos(t), 40.0 * math.sin(t)) for t in np.linspace(-1.2, 1.2, 13)]
_CONE_PROFILE = [(3.0 + 1.6 * i, -35.0 + 5.5 * i) for i in range(14)]

# name -> (vertices fp64, frame kind, eps, expected discrete count, expected continuous count, expected closed, expected truncated)
TOOL_SHAPES = {
    "cuboid": (lambda: _box_surface(30.0, 45.0, 65.0, 9), "model", 0.5, 3, 0, True, False),
    "square-prism": (lambda: _box_surface(30.0, 30.0, 65.0, 9), "model", 0.5, 7, 0, True, False),
    "cube": (lambda: _box_surface(40.0, 40.0, 40.0, 9), "model", 0.5, 23, 0, True, False),
    "revolution-flip": (lambda: _revolution(_FLIP_PROFILE), "model", 2.35, 2, 1, True, False),
    "revolution-cone": (lambda: _revolution(_CONE_PROFILE), "model", 1.8, 0, 1, True, False),
    "scalene": (lambda: _scalene(), "model", 0.5, 0, 0, True, False),
    "square-prism-turned": (lambda: _box_surface(30.0, 30.0, 65.0, 9) @ GENERIC_TURN.T + GENERIC_SHIFT, "obox", 0.5, 7, 0, True, False),
    # a cuboid tilted by a quarter of a degree about the diagonal of its xy plane, in the model frame, with an eps between the deviations of the
    # half turns about x and y (0.44, 0.49) and that of their product, the half turn about z (0.73): the closure is not closed
    "cuboid-tilted": (lambda: _box_surface(30.0, 45.0, 65.0, 9) @ rodrigues(np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0), math.radians(0.25)).T, "model", 0.6, 2, 0, False, False),
}


@functools.lru_cache(None)
def tool_mesh(name):
    return TOOL_SHAPES[name][0]().astype(f32)


def spoil_turn(entry, degrees=20.0):
    """A copy of a models_info entry whose first discrete symmetry is turned by `degrees` about a generic axis."""
    out = dict(entry)
    m = np.asarray(entry["symmetries_discrete"][0], f64).reshape(4, 4).copy()
    m[:3, :3] = rodrigues(np.array([1.0, 2.0, 2.0]) / 3.0, math.radians(degrees)) @ m[:3, :3]
    out["symmetries_discrete"] = [m.reshape(16).tolist()] + [list(s) for s in entry["symmetries_discrete"][1:]]
    return out


def spoil_axis(entry, degrees=20.0):
    """A copy of a models_info entry whose continuous axis is tilted by `degrees`."""
    out = dict(entry)
    c = dict(entry["symmetries_continuous"][0])
    a = np.asarray(c["axis"], f64)
    other = np.eye(3)[int(np.argmin(np.abs(a)))]
    c["axis"] = (rodrigues(np.cross(a, other) / np.linalg.norm(np.cross(a, other)), math.radians(degrees)) @ a).tolist()
    out["symmetries_continuous"] = [c]
    return out
