"""tests/render_grid.py without a GPU: its integer reference against the numpy oracle (two independent statements of
include/lc_amd_render.h) on every scene, against hand counts, and the reason each scene is there, asserted from the reference."""
import numpy as np
import pytest

from tests import render_grid as rg
from tests import render_oracle as ro

NAMES = [s.name for s in rg.SCENES]
ONE = np.float32(1).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rect(shape, xs, ys):
    m = np.zeros(shape, dtype=bool)
    m[ys[0]:ys[1] + 1, xs[0]:xs[1] + 1] = True
    return m


@pytest.mark.parametrize("name", NAMES)
def test_integer_reference_equals_the_numpy_oracle(name):
    sc, ref = rg.BY_NAME[name], rg.reference(name)
    o = ro.render(sc.verts, sc.faces, sc.R, sc.t, sc.K, sc.size_hw, sc.near, sc.far, sc.center_px)
    assert np.array_equal(_bits(ref.depth), _bits(o.depth))
    assert np.array_equal(ref.face, o.face)
    assert np.array_equal(ref.mask, o.mask) and ref.info == o.info
    assert np.array_equal(ref.mask, ref.face >= 0) and np.array_equal(ref.mask, ref.depth > 0)
    # the exact scenes sit ON the snapping grid (margin 0.5 grid units) or on a half (margin 0): nothing the older cases allow
    assert sc.exact == (name != "near-rounds-onto-near")


def test_scene_limits():
    assert all(max(s.size_hw) <= 96 and len(s.faces) <= 400 for s in rg.SCENES)
    assert sum(len(v) for v in rg.groups().values()) == len(rg.SCENES)


def test_homo_z_is_one_rounding_of_the_exact_product():
    ref, sc = rg.reference("slanted-wave-path"), rg.BY_NAME["slanted-wave-path"]
    ys, xs = np.nonzero(ref.mask)
    z = ref.depth[ys, xs].astype(np.float64)
    M = rg.PIX2K.astype(np.float64)
    # fp64 holds (24-bit z) x (a few bits of p) exactly, so numpy's product rounded to fp32 is the one rounding
    assert np.array_equal(ref.homo_z[ys, xs, 0], ((xs + 0.5) * z).astype(np.float32)) and np.array_equal(ref.homo_z[ys, xs, 2], ref.depth[ys, xs])
    assert np.array_equal(ref.homo_z_pix2k[ys, xs, 1], ((M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) * z).astype(np.float32))
    assert not ref.homo_z[~ref.mask].any() and len(set(_bits(ref.depth[ref.mask]).tolist())) > 100


# ---- hand counts ------------------------------------------------------------------------------------------------------------------

def test_quad_on_samples_and_its_four_shifts():
    """Corners on the samples of pixels (3,2) and (10,9): 8 x 8 pixels, edges and vertices included; the diagonal's 8 samples are hit by
    both faces and go to face 0, which so has 8 + 7 + ... + 1 = 36 pixels.  One grid unit to the right loses column 3 and keeps column
    10 (its samples are now inside by one unit); likewise for the other three."""
    for name in ("quad-on-samples", "quad-on-samples-cw"):
        ref = rg.reference(name)
        assert np.array_equal(ref.mask, _rect((16, 16), (3, 10), (2, 9))) and (_bits(ref.depth[ref.mask]) == ONE).all() and ref.info == 0
        assert (ref.face == 0).sum() == 36 and (ref.face == 1).sum() == 28
        d = np.arange(8)
        assert (ref.face[2 + d, 3 + d] == 0).all() and ref.tie[2 + d, 3 + d].all() and ref.tie.sum() == 8 and (ref.runner[2 + d, 3 + d] == 1).all()
    up, lo = rg.reference("quad-on-samples").face, rg.reference("quad-on-samples-cw").face
    assert np.array_equal(up, lo)  # the winding changes nothing
    for tag, xs, ys in (("x+1", (4, 10), (2, 9)), ("x-1", (3, 9), (2, 9)), ("y+1", (3, 10), (3, 9)), ("y-1", (3, 10), (2, 8))):
        ref = rg.reference(f"quad-shift-{tag}")
        assert np.array_equal(ref.mask, _rect((16, 16), xs, ys)) and ref.mask.sum() == 56 and not ref.tie.any()


def test_64_and_65_sample_faces():
    """Right triangles on samples: legs of 7 and 7 steps hold 8 + 7 + ... + 1 = 36 samples in an 8 x 8 box; legs of 4 and 12 steps hold the
    (i, j) with 3 i + j <= 12, 13 + 10 + 7 + 4 + 1 = 35, in a 5 x 13 box."""
    a, b = rg.reference("switch-64-lane-path"), rg.reference("switch-65-wave-path")
    assert rg.tile_counts(rg.BY_NAME["switch-64-lane-path"], 0) == {(0, 0): 64} and a.mask.sum() == 36
    assert rg.tile_counts(rg.BY_NAME["switch-65-wave-path"], 0) == {(0, 0): 65} and b.mask.sum() == 35
    assert [int(n) for n in b.mask[2:15, 3:8].sum(0)] == [13, 10, 7, 4, 1] and [int(n) for n in a.mask[2:10, 3:11].sum(1)] == list(range(8, 0, -1))


def test_largest_coordinate():
    sc, ref = rg.BY_NAME["extent-2^25"], rg.reference("extent-2^25")
    assert sorted(abs(c) for c in sum(rg.snapped(sc), ())) == [0] + [2 ** 25] * 5
    assert ref.mask.all() and (_bits(ref.depth) == ONE).all() and (ref.face == 0).all() and ref.info == 0
    sc, ref = rg.BY_NAME["extent-2^25+1"], rg.reference("extent-2^25+1")
    assert max(abs(c) for c in sum(rg.snapped(sc), ())) == 2 ** 25 + 1
    assert not ref.mask.any() and ref.info == 1


def test_near_and_far():
    """The quad spans the samples of pixels 3..9 in both directions: 49 pixels where it is drawn at all."""
    full = _rect((16, 16), (3, 9), (3, 9))
    at, below = rg.reference("far-at"), rg.reference("far-just-below")
    assert rg.BY_NAME["far-at"].far == 8.0 and not at.mask.any() and at.info == 0
    assert np.float32(rg.BY_NAME["far-just-below"].far) == np.nextafter(np.float32(8), np.float32(9))
    assert np.array_equal(below.mask, full) and (_bits(below.depth[full]) == np.float32(8).view(np.uint32)).all() and below.info == 0
    sc, onto = rg.BY_NAME["near-rounds-onto-near"], rg.reference("near-rounds-onto-near")
    z = {p[2] for p in sc.pts}
    assert len(z) == 1 and float(min(z)) > sc.near and np.float32(float(min(z))) == np.float32(sc.near)  # passes the setup's fp64 test, rounds onto near
    assert float(sc.t[2]) == 2.0 ** -40 and (sc.verts[:, 2] == sc.near).all()
    assert not onto.mask.any() and onto.info == 0
    sc, vert = rg.BY_NAME["near-vertex-at-near"], rg.reference("near-vertex-at-near")
    assert [float(sc.pts[i][2]) == sc.near for i in sc.faces[2]] == [True, False, False]
    assert np.array_equal(vert.mask, full) and vert.info == 1 and (vert.face[full] <= 1).all() and (vert.depth[full] == 0.25).all()


def test_half_even_snapping():
    """An edge at k + 1/2 grid units.  k even goes down to k, where floor(x + 1/2) goes up: the left edge on sample column 3 keeps it (7 x 7
    against 6 x 6), the right edge one unit below column 9's (odd) sample stays below it (6 x 6 against 7 x 7).  k odd goes up to k + 1, where
    a truncation stays: the mirror images.  Below zero floor(x + 1/2) still goes up: -897.5 to -897, half-even to -898, column 60's sample."""
    for name, even, half_up, trunc in (("snap-even-left", 49, 36, 49), ("snap-even-right", 36, 49, 36), ("snap-odd-right", 49, 49, 36),
                                       ("snap-odd-left", 36, 36, 49), ("snap-even-negative", 12, 8, 8)):
        sc = rg.BY_NAME[name]
        halves = [g for p in sc.pts for g in p[:2] if g.denominator == 2]
        assert halves and all((int(g - rg.Fr(1, 2)) % 2 == 0) == ("even" in name) for g in halves)
        got = [int(rg.raster_int(sc, r).mask.sum()) for r in ("even", "half_up", "trunc")]
        assert got == [even, half_up, trunc], name
    a, b = rg.reference("snap-even-left").mask, rg.raster_int(rg.BY_NAME["snap-even-left"], "half_up").mask
    assert np.array_equal(a, _rect((16, 16), (3, 9), (3, 9))) and np.array_equal(b, _rect((16, 16), (4, 9), (4, 9)))  # exactly column 3 and row 3
    a, b = rg.reference("snap-even-right").mask, rg.raster_int(rg.BY_NAME["snap-even-right"], "half_up").mask
    assert np.array_equal(a, _rect((16, 16), (3, 8), (3, 8))) and np.array_equal(b, _rect((16, 16), (3, 9), (3, 9)))
    a, b = rg.reference("snap-even-negative").mask, rg.raster_int(rg.BY_NAME["snap-even-negative"], "half_up").mask
    assert np.array_equal(a, _rect((8, 64), (60, 62), (2, 5))) and np.array_equal(b, _rect((8, 64), (61, 62), (2, 5)))


def test_sample_centres():
    """Quads with corners on the whole pixels (2,3) and (9,11), and the same 64 px to either side: whole-pixel samples see 8 x 9 with the
    edges, half-pixel samples 7 x 8, and (1/256, 255/256) keeps column 2 (one unit inside) and loses row 2 (one unit outside): 7 x 8."""
    want = {(0, 0): ((2, 9), (3, 11), {0, 1}), (128, 128): ((2, 8), (3, 10), {0, 1}), (1, 255): ((2, 8), (3, 10), {0, 1}),
            (-16384, 16384): ((2, 9), (3, 11), {2, 3}), (16384, -16384): ((2, 9), (3, 11), {4, 5})}
    assert set(want) == set(rg.SAMPLE_CENTERS)
    for c, (xs, ys, faces) in want.items():
        ref = rg.reference(f"centre-{c[0]}-{c[1]}")
        assert np.array_equal(ref.mask, _rect((16, 16), xs, ys)) and set(ref.face[ref.mask].tolist()) == faces


# ---- the reason each scene is there --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rg.TIES))
def test_tie_scenes_tie_and_reverse(name):
    (i, _), (j, _) = rg.TIES[name]
    sc, ref, rev = rg.BY_NAME[name], rg.reference(name), rg.reference(name + "-rev")
    n = len(sc.faces)
    assert i < j == n - 1 and ref.tie.sum() >= 15
    assert (ref.face[ref.tie] == i).all() and (ref.runner[ref.tie] == j).all()  # equal depth bits: the lower index wins
    assert (ref.face == j).any() and (ref.face == i).sum() > ref.tie.sum()  # and each face has pixels of its own
    path = lambda f: "wave" if max(rg.tile_counts(sc, f).values()) > rg.COOP else "lane"  # noqa: E731
    assert [path(i), path(j)] == [("wave" if "wave-path" in w else "lane") for w in _paths(name)]
    assert all(rg.tile_counts(sc, f) and max(rg.tile_counts(sc, f).values()) == 1 for f in range(n) if f not in (i, j))
    # the faces in reverse order: the same bits, the same faces mapped back, except that the tie pixels go to the other face
    assert np.array_equal(_bits(ref.depth), _bits(rev.depth)) and np.array_equal(ref.tie, rev.tie) and ref.info == rev.info
    back = np.where(rev.face >= 0, n - 1 - rev.face, -1)
    assert np.array_equal(back[~ref.tie], ref.face[~ref.tie]) and (back[ref.tie] == j).all()


def _paths(name):
    """("lane-path" | "wave-path") of the two tie faces, from the scene's name; plain names are two lane-path faces."""
    if "path" not in name:
        return ("lane-path", "lane-path")
    if "wave-paths" in name:
        return ("wave-path", "wave-path")
    return ("lane-path", "wave-path") if name.index("lane-path") < name.index("wave-path") else ("wave-path", "lane-path")


def test_shared_edge_goes_to_the_nearer_face():
    ref, rev = rg.reference("shared-edge-nearer-wins"), rg.reference("shared-edge-nearer-wins-rev")
    ys = np.arange(2, 11)
    assert (ref.face[ys, 8] == 1).all() and (ref.runner[ys, 8] == 0).all() and (ref.depth[ys, 8] == 0.5).all() and not ref.tie.any()
    assert (ref.face == 0).any() and np.array_equal(_bits(ref.depth), _bits(rev.depth)) and np.array_equal(np.where(rev.face >= 0, 1 - rev.face, -1), ref.face)


def test_switch_scenes_have_the_stated_box_in_tile_counts():
    assert rg.tile_counts(rg.BY_NAME["switch-seam-64-and-65"], 0) == {(0, 0): 64, (1, 0): 40, (0, 1): 104, (1, 1): 65}
    ref = rg.reference("switch-seam-64-and-65")
    assert all(ref.mask[y:y + 32, x:x + 32].any() for y in (0, 32) for x in (0, 32))  # the face is seen in all four tiles
    for name, big in (("wave-path-single-face", [0]), ("wave-path-last-of-65", [64]), ("wave-path-lanes-0-1-62-63", [0, 1, 62, 63]),
                      ("wave-path-face-257", [257])):
        sc, ref = rg.BY_NAME[name], rg.reference(name)
        assert len(sc.faces) == {"wave-path-single-face": 1, "wave-path-last-of-65": 65, "wave-path-lanes-0-1-62-63": 64, "wave-path-face-257": 258}[name]
        for f in range(len(sc.faces)):
            counts = rg.tile_counts(sc, f)
            assert (counts[(0, 0)] > rg.COOP) if f in big else (max(counts.values()) == 1)
            assert (ref.face == f).any()  # every face, filler or large, is seen
    four = rg.reference("wave-path-lanes-0-1-62-63")
    assert len({tuple(rg.box(rg.BY_NAME["wave-path-lanes-0-1-62-63"], rg.snapped(rg.BY_NAME["wave-path-lanes-0-1-62-63"]), rg.BY_NAME["wave-path-lanes-0-1-62-63"].faces[f]))
                for f in (0, 1, 62, 63)}) == 4  # four different boxes
    assert four.tie.any() and (four.runner >= 0).sum() > 300  # they overlap, two of them at the same depth
    for name in ("seams-both", "map-33x47-vertices-outside", "slanted-wave-path"):
        assert max(rg.tile_counts(rg.BY_NAME[name], 0).values()) > rg.COOP and len(rg.tile_counts(rg.BY_NAME[name], 0)) == 4
    assert rg.tile_counts(rg.BY_NAME["slanted-lane-path"], 0)[(0, 0)] <= rg.COOP and rg.tile_counts(rg.BY_NAME["slanted-lane-path"], 1)[(0, 0)] <= rg.COOP


def test_border_scenes():
    sc = rg.BY_NAME["map-33x47-vertices-outside"]
    H, W = sc.size_hw
    S = rg.snapped(sc)
    xs, ys = [p[0] for p in S], [p[1] for p in S]
    assert min(xs) < 128 and max(xs) > rg.S(W - 1) and min(ys) < 128 and max(ys) > rg.S(H - 1)  # vertices beyond every side
    ref = rg.reference(sc.name)
    assert ref.mask[0].any() and ref.mask[-1].any() and ref.mask[:, 0].any() and ref.mask[:, -1].any() and not ref.mask.all()
    for name, n in (("map-1x1", 1), ("map-1x65", 46), ("map-65x1", 46)):
        assert rg.reference(name).mask.sum() == n
    assert np.array_equal(rg.reference("map-1x65").mask.T, rg.reference("map-65x1").mask)
    # 256 (i + j) - 2 d <= 1500 over the samples i, j >= 0 (from 1 where the face starts one unit past sample 0)
    counts = {-257: 10, -256: 10, -255: 10, -1: 21, 0: 21, 1: 10}
    for d in rg.NEGBOX:
        sc, ref = rg.BY_NAME[f"negbox-{d:+d}"], rg.reference(f"negbox-{d:+d}")
        S = rg.snapped(sc)
        assert min(p[0] for p in S[:3]) - sc.center[0] == d == max(p[0] for p in S[3:]) - sc.center[0]
        assert min(p[1] for p in S[:3]) - sc.center[1] == d == max(p[1] for p in S[3:]) - sc.center[1]
        assert (ref.face == 0).sum() + (ref.runner == 0).sum() == counts[d]
        # the face that ends d units from sample 0 reaches it from d = 0 on, and nothing else
        assert (ref.face == 1).sum() == (1 if d >= 0 else 0) and (d < 0 or ref.face[0, 0] == 1)


def test_zero_area_scenes():
    full = _rect((16, 16), (3, 9), (3, 9))
    for name in ("zero-repeated-index", "zero-snapped-collinear", "sliver-no-sample", "sliver-one-sample"):
        sc, ref = rg.BY_NAME[name], rg.reference(name)
        S = [rg.snapped(sc)[i] for i in sc.faces[2]]
        area = (S[1][0] - S[0][0]) * (S[2][1] - S[0][1]) - (S[1][1] - S[0][1]) * (S[2][0] - S[0][0])
        assert (area == 0) == name.startswith("zero") and np.array_equal(ref.mask, full) and ref.info == 0
        assert (ref.face == 2).sum() == (1 if name == "sliver-one-sample" else 0)
    sc = rg.BY_NAME["zero-snapped-collinear"]
    assert len({tuple(sc.verts[i]) for i in sc.faces[2]}) == 3 and len(set(sc.faces[2])) == 3 and len(set(rg.BY_NAME["zero-repeated-index"].faces[2])) == 2
    one = rg.reference("sliver-one-sample")
    assert one.face[3, 3] == 2 and one.depth[3, 3] == 1 and one.runner[3, 3] in (0, 1)
    for name in ("sliver-no-sample", "sliver-one-sample"):
        xs = [p[0] for p in (rg.snapped(rg.BY_NAME[name])[i] for i in rg.BY_NAME[name].faces[2])]
        assert max(xs) - min(xs) == 1


def test_slanted_faces_change_the_winner_inside_the_overlap():
    for name in ("slanted-wave-path", "slanted-lane-path"):
        sc, ref = rg.BY_NAME[name], rg.reference(name)
        assert sorted(float(sc.pts[i][2]) for i in sc.faces[0]) == [0.25, 0.5, 1.0] == sorted(float(sc.pts[i][2]) for i in sc.faces[1])
        both = ref.runner >= 0
        assert (ref.face[both] == 0).sum() >= 3 and (ref.face[both] == 1).sum() >= 3
        assert max(abs(c) for p in rg.snapped(sc) for c in p) < 2 ** 20
