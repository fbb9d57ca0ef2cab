"""The numpy restatement of lc_amd.models' definitions (include/lc_amd_models.h, `lc_model_prepare_f32`) and the case list of its tests.

numpy's elementwise float32 operations round one at a time, so every value below is the definition's own: the GPU tests compare
bit for bit.

Two case lists.  `named_cases`: Gaussian clouds at the sizes around every boundary of the kernels (no ties at all), a cube and a line.
`tied_cases`: points on an integer lattice, where equal distances are equal bits, with the tied vertices planted so that one merge
level of the kernels after the other has to break a tie: inside a tile, between tiles in tile order, in the reducer's second
round, across the selection's waves and slots.  `diameter` and `fps` take a `mistake=` that restates one wrong merge; it is never
what the device is compared with, only the proof (tests/test_models_host.py) that a tied case tells that mistake from the definition.
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


DIAMETER_MISTAKES = ("first_partial", "last_partial", "j_then_i", "largest_j", "lane_before_slot", "reduce_largest_j", "one_round")
FPS_MISTAKES = ("largest_index", "thread_before_slot", "wave_order_reversed")
WAVE, POINT_THREADS, REDUCE_THREADS = 64, 1024, 256  # the wavefront, kPointThreads and kReduceThreads of lc_models.hip


def diameter_tiled(v, tile, mistake=None):
    """The diameter along the kernels' own merge levels, so that a wrong merge can be stated: per tile (ib <= jb, tile number
    t = jb (jb + 1) / 2 + ib) every i keeps its best (d2, j) while j ascends, the tile keeps the best (d2, smallest il), and the partials
    are merged under (d2, smallest i, smallest j).  `mistake=None` is `diameter` (the host tests hold it to that); a name restates
    one wrong kernel:
        largest_j         `>=` in the walk: the last j of a tie survives in the tile
        lane_before_slot  the tile orders its i's by (il % (tile/2), il // (tile/2)): the lane before the lane's slot
        j_then_i          the smallest j wins before the smallest i, in the tile and among the partials
        first_partial / last_partial   tied partials are settled by their tile number t
        reduce_largest_j  among partials of equal (d2, i) the largest j wins
        one_round         the reducer reads its first REDUCE_THREADS partials only"""
    if mistake is not None and mistake not in DIAMETER_MISTAKES:
        raise ValueError(mistake)
    v = np.asarray(v, f32)
    V = len(v)
    if V == 1:
        return f32(0), (0, 0)
    half, parts = tile // 2, []
    for jb in range(-(-V // tile)):
        for ib in range(jb + 1):
            i0, j0 = ib * tile, jb * tile
            blk = d2(v[i0:i0 + tile, None, :], v[None, j0:j0 + tile, :])
            if ib == jb:
                blk = np.where(np.arange(blk.shape[1])[None, :] > np.arange(blk.shape[0])[:, None], blk, f32(-1))
            best = blk.max(1)
            bj = blk.shape[1] - 1 - blk[:, ::-1].argmax(1) if mistake == "largest_j" else blk.argmax(1)
            if best.max() < 0:
                continue  # a diagonal tile of one vertex holds no pair
            rank = {"lane_before_slot": lambda a: (a % half, a // half), "j_then_i": lambda a: (bj[a], a)}.get(mistake, lambda a: a)
            a = min(np.flatnonzero(best == best.max()).tolist(), key=rank)
            parts.append((jb * (jb + 1) // 2 + ib, best[a], i0 + a, j0 + int(bj[a])))
    if mistake == "one_round":
        parts = [p for p in parts if p[0] < REDUCE_THREADS]
    top = max(p[1] for p in parts)
    order = {"first_partial": lambda p: p[0], "last_partial": lambda p: -p[0], "j_then_i": lambda p: (p[3], p[2]),
             "reduce_largest_j": lambda p: (p[2], -p[3])}.get(mistake, lambda p: (p[2], p[3]))
    _, d, i, j = min((p for p in parts if p[1] == top), key=order)
    return np.sqrt(d, dtype=f32), (i, j)


def diameter(v, rows=512, *, mistake=None, tile=256):
    """(diameter float32, (i, j)): the largest d2 over i < j, ties to the smallest i, then the smallest j; sqrt correctly rounded.
    A `mistake` (DIAMETER_MISTAKES) answers as a wrong kernel of tile edge `tile` would: see diameter_tiled."""
    if mistake is not None:
        return diameter_tiled(v, tile, mistake)
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


def maximal_pairs(v, rows=512):
    """(largest d2, every (i, j), i < j, that has it, in (i, j) order)."""
    v = np.asarray(v, f32)
    col, top, pairs = np.arange(len(v)), f32(-1), []
    for i0 in range(0, len(v), rows):
        blk = d2(v[i0:i0 + rows, None, :], v[None, :, :])
        blk = np.where(col[None, :] > np.arange(i0, i0 + len(blk))[:, None], blk, f32(-1))
        if blk.max() > top:
            top, pairs = blk.max(), []
        if blk.max() == top:
            pairs += [(i0 + int(a), int(b)) for a, b in zip(*np.nonzero(blk == top))]
    return top, pairs


def _pick(mind, mistake):
    """The index a pick takes from the distances: the first maximum, or what a wrong merge of the kernel's levels (vertex i lives in
    thread i % POINT_THREADS, slot i // POINT_THREADS, and that thread in wave (i // WAVE) % (POINT_THREADS / WAVE)) would take:
        largest_index        the last maximum
        thread_before_slot   ties ordered by (thread, slot)
        wave_order_reversed  the last wave that holds a maximum wins, inside it the smallest index"""
    if mistake is None:
        return int(mind.argmax())
    tied = np.flatnonzero(mind == mind.max())
    if mistake == "largest_index":
        return int(tied[-1])
    if mistake == "thread_before_slot":
        return int(min(tied.tolist(), key=lambda i: (i % POINT_THREADS, i // POINT_THREADS)))
    if mistake == "wave_order_reversed":
        return int(min(tied.tolist(), key=lambda i: (-((i // WAVE) % (POINT_THREADS // WAVE)), i)))
    raise ValueError(mistake)


def fps(v, count, *, mistake=None, ties=None):
    """(index (count,) int32, points (count,3) float32): seeded at the box centre, argmax ties to the smallest index.  A `mistake`
    (FPS_MISTAKES, see _pick) answers as a wrong kernel would; a list `ties` receives every pick's tied maxima."""
    v = np.asarray(v, f32)
    if count > len(v):
        raise ValueError("count > V")
    lo, hi = extents(v)
    c = (lo + hi) * f32(0.5)
    mind = d2(v, c)
    idx = np.empty(count, np.int32)
    for n in range(count):
        k = _pick(mind, mistake)  # None: the first maximum
        if ties is not None:
            ties.append(np.flatnonzero(mind == mind.max()))
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
    nine index pairs for each), eight equidistant first picks.  With 24 vertices every one of these ties is settled inside one
    wavefront, one tile, one register slot and one partial: the merges above that are `tied_cases`' to force."""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32) * f32(0.5)
    v = np.concatenate([c, c, c])
    return v[np.random.default_rng(3).permutation(len(v))]


def collinear(V=97):
    t = np.linspace(-1, 1, V).astype(f32)
    return np.stack([t * f32(0.3), t * f32(-0.2), t * f32(0.7)], -1).astype(f32)


FACES0 = np.zeros((0, 3), np.int32)


def named_cases(tile, resident):
    """name -> (verts, fps counts, want_diameter): the sizes around every boundary of the kernels.  `tile` / `resident` are
    lc_amd.models.DIAM_TILE / FPS_RESIDENT.  The two meshes around the resident limit take the diameter too (3.4e7 pairs each, under a
    second of numpy): 33 tile rows, 561 partials, three rounds of the reducer's loop."""
    cases = {}
    for V in (1, 2, 3, 63, 64, 65):
        cases[f"V{V}"] = (cloud(V, 100 + V), (1, min(16, V), V), True)
    for name, V in (("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1), ("2tiles+1", 2 * tile + 1), ("rows", 1100)):
        cases[name] = (cloud(V, 200 + V), (16,), True)
    cases["resident"] = (cloud(resident, 7), (16,), True)
    cases["resident+1"] = (cloud(resident + 1, 8), (16,), True)
    cases["cube_duplicates"] = (cube_with_duplicates(), (24,), True)
    cases["collinear"] = (collinear(), (16,), True)
    cases["mm_offset"] = (cloud(300, 9, scale=40.0, offset=1.0e4), (16,), True)
    return cases


# ---- inputs whose ties are exact and placed: every merge level of the kernels is asked to break one ----

LATTICE_BITS = 8    # a lattice step is 2^-8
PLANT_STEPS = 32    # planted vertices sit 32 steps out on an axis, outside every interior this file draws


def lattice(V, seed, r, k=LATTICE_BITS):
    """V integer points (drawn with repeats) inside the ball of radius r lattice steps, scaled by 2^-k.  With r <= 32 every difference,
    square and sum of a d2 is an integer below 2^24 in lattice units: exact in fp32 under any evaluation order, so equal distances
    are equal bits."""
    rng = np.random.default_rng(seed)
    pts = np.empty((0, 3), np.int64)
    while len(pts) < V:
        p = rng.integers(-r, r + 1, size=(2 * V + 16, 3))
        pts = np.concatenate([pts, p[(p * p).sum(1) <= r * r]])
    return (pts[:V] * 2.0 ** -k).astype(f32)


def plant(v, families, k=LATTICE_BITS, steps=PLANT_STEPS):
    """A copy of v with, for every family (axis a, P, Q), the vertices P at +A e_a and Q at -A e_a, A = steps * 2^-k.  Inside a family
    every (P, Q) pair has d2 = 4 A^2, across families 2 A^2, against an interior of radius r < steps at most (A + r 2^-k)^2 < 4 A^2:
    the families share the maximum, and indices alone decide."""
    v = np.array(v, f32)
    A = f32(steps * 2.0 ** -k)
    for a, P, Q in families:
        for idx, s in ((P, A), (Q, -A)):
            v[list(idx)] = 0
            v[list(idx), a] = s
    return v


def tile_number(i, j, tile):
    ib, jb = i // tile, j // tile
    return jb * (jb + 1) // 2 + ib


class TiedCase(SimpleNamespace):
    """verts, fps_count, forces (the merge level the case is for), pair (the diameter's pair by construction, or None),
    mistakes (names of DIAMETER_MISTAKES / FPS_MISTAKES that must change the oracle's answer on it),
    spans(pairs) -> bool on the maximal pairs (None: no claim), fps_spans (of "waves", "slots": what some pick's tied maxima must span)."""


TIED_NAMES = ("lane-slots", "waves", "same-i-many-j", "tile-order", "reduce-two-rounds", "reduce-max-in-second-round", "all-identical",
              "fps-ties-resident", "fps-ties-streaming")


def tied_cases(tile, resident):
    """name -> TiedCase.  `tile` / `resident` are lc_amd.models.DIAM_TILE / FPS_RESIDENT; a tile's workgroup has tile / 2 threads, each
    with the i-vertices il = lane and il = tile / 2 + lane."""
    h, cases = tile // 2, {}

    def add(name, verts, forces, mistakes, pair=None, spans=None, fps_count=16, fps_spans=()):
        cases[name] = TiedCase(verts=verts, fps_count=fps_count, forces=forces, mistakes=tuple(mistakes), pair=pair, spans=spans, fps_spans=tuple(fps_spans))

    i_of = lambda pairs: sorted({i for i, _ in pairs})
    t_of = lambda pairs: sorted({tile_number(i, j, tile) for i, j in pairs})

    add("lane-slots", plant(lattice(tile, 31, 24), [(0, [5], [h + 72]), (1, [h + 2], [h + 52]), (2, [h + 5], [h + 62])]),
        "one tile: a lane's two slots (il = 5 and tile/2 + 5) and the key's il field across lanes (il = tile/2 + 2 is lane 2)",
        ("lane_before_slot", "j_then_i"), pair=(5, h + 72), spans=lambda pairs: i_of(pairs) == [5, h + 2, h + 5] and len(pairs) == 3)
    add("waves", plant(lattice(tile, 32, 24), [(0, [3], [h + 72]), (1, [WAVE + 6], [h + 22])]),
        "one tile: the workgroup's two waves, the i of the second wave with the smaller j", ("j_then_i",), pair=(3, h + 72),
        spans=lambda pairs: pairs == [(3, h + 72), (WAVE + 6, h + 22)] and (WAVE + 6) // WAVE == 1 and WAVE + 6 < h)
    add("same-i-many-j", plant(lattice(2 * tile + 40, 33, 24), [(0, [7], [tile + 20, tile + 90, 2 * tile + 5])]),
        "one i: two tied j inside a tile (the walk's strict >), a third in a later tile (the reducer's j)",
        ("largest_j", "last_partial", "reduce_largest_j"), pair=(7, tile + 20),
        spans=lambda pairs: pairs == [(7, tile + 20), (7, tile + 90), (7, 2 * tile + 5)] and t_of(pairs) == [1, 3])
    add("tile-order", plant(lattice(4 * tile + 76, 34, 24), [(0, [tile + 44], [tile + 144]), (1, [10], [3 * tile + 232, 2 * tile + 188]),
                                                               (2, [tile + 244], [4 * tile + 26])]),
        "five tile rows: the winning partial is neither the first nor the last of the tied ones in tile order",
        ("first_partial", "last_partial", "j_then_i", "reduce_largest_j"), pair=(10, 2 * tile + 188),
        spans=lambda pairs: len(pairs) == 4 and min(t_of(pairs)) < tile_number(10, 2 * tile + 188, tile) < max(t_of(pairs)))
    big = 23 * tile + 1  # 24 tile rows, 300 partials: the reducer's threads 0..43 read a second one
    add("reduce-two-rounds", plant(lattice(big, 35, 24), [(1, [10], [5 * tile + 30, 22 * tile + 40]), (0, [11 * tile + 20], [11 * tile + 100]),
                                                            (2, [7 * tile + 3], [23 * tile])]),
        "300 partials: the winner's j across two threads, a tied partial inside tile row 11, one in the reducer's second round",
        ("last_partial", "reduce_largest_j"), pair=(10, 5 * tile + 30),
        spans=lambda pairs: len(pairs) == 4 and max(t_of(pairs)) >= REDUCE_THREADS
        and len({tile_number(10, j, tile) % REDUCE_THREADS for j in (5 * tile + 30, 22 * tile + 40)}) == 2)
    add("reduce-max-in-second-round", plant(lattice(big, 36, 24), [(0, [20 * tile + 17], [22 * tile + 100])], steps=72),
        "300 partials: a strictly larger d2 arrives in a thread's second round", ("one_round",), pair=(20 * tile + 17, 22 * tile + 100),
        spans=lambda pairs: len(pairs) == 1 and t_of(pairs)[0] >= REDUCE_THREADS)
    add("all-identical", np.tile(np.array([3, -5, 7], f32) * f32(2.0 ** -LATTICE_BITS), (300, 1)),
        "every pair and every vertex tied: d2 = 0, pair (0, 1), index 0 at every pick",
        ("last_partial", "largest_j", "reduce_largest_j", "largest_index", "wave_order_reversed"), pair=(0, 1), fps_count=40, fps_spans=("waves",))
    add("fps-ties-resident", lattice(2500, 37, 6), "resident selection: tied maxima across the 16 waves and across the three register slots in use",
        FPS_MISTAKES, fps_count=64, fps_spans=("waves", "slots"))
    add("fps-ties-streaming", lattice(resident + 300, 38, 6), "streaming selection: tied maxima across waves and across a thread's strided visits; "
        "over a thousand maximal pairs spread over every tile row",FPS_MISTAKES + tuple(m for m in DIAMETER_MISTAKES if m != "one_round"), fps_count=64, fps_spans=("waves", "slots"))
    return cases
