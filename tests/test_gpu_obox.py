"""lc_amd.obox on the GPU: every output EQUAL to the numpy oracle's (tests/obox_oracle.py), bit for bit and `path` included -- at one
wave's, the LDS tile's and the vertex split's edges, with several meshes of unequal size side by side, in both modes and about all three
axes, at 0, 1 and the default number of levels, with a planted NaN, on a case whose lowest level-0 score is shared by two candidates, on
boxes turned off the grid, on a second call and under a captured graph replayed twice.  The level-0 tables hold 1419 and 10 candidates and
the later ones 125 and 5: none is a multiple of 64.  tests/test_obox_host.py checks the conditions these cases rely on."""
import numpy as np
import pytest
import torch

from tests import obox_cases as cases

pytestmark = pytest.mark.gpu
FACES0 = np.zeros((0, 3), np.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def _set(dev, names):
    from lc_amd.render import MeshSet

    return MeshSet([(cases.mesh(n), FACES0) for n in names], dev)


def _host(box):
    return {f: getattr(box, f).cpu().numpy() for f in cases.FIELDS}


def _check(got, names, axis=None, levels=6):
    for k, name in enumerate(names):
        want = cases.reference(name, axis, levels)
        for f in cases.FIELDS:
            assert cases.same_bits(got[f][k], getattr(want, f)[0]), (name, axis, levels, f, got[f][k], getattr(want, f)[0])


@pytest.mark.parametrize("V", cases.SIZES)
def test_one_mesh_of_every_size_equals_the_oracle(dev, V):
    from lc_amd import obox

    name = f"cloud:{V}"
    got = _host(obox.oriented_box(_set(dev, [name])))
    print(V, got["path"][0].tolist(), float(got["volume"][0]), float(got["aabb_volume"][0]))
    _check(got, [name])


NAMES = ("cloud:1025", "cloud:1", "tie-cube", "cloud:65", f"cloud:{2 * cases.SPLIT + 300}", "flat", "cloud:3", "offgrid:0", "cloud:256")


def test_unequal_meshes_side_by_side_equal_each_mesh_alone(dev):
    from lc_amd import obox

    together = _host(obox.oriented_box(_set(dev, NAMES)))
    _check(together, NAMES)
    for k in (0, 2, 4):  # and the device's own answer for a mesh alone, whose offset, chunk count and grid differ
        alone = _host(obox.oriented_box(_set(dev, [NAMES[k]])))
        for f in cases.FIELDS:
            assert cases.same_bits(alone[f][0], together[f][k]), (NAMES[k], f)


@pytest.mark.parametrize("axis", [0, 1, 2, "z"])
def test_about_one_axis(dev, axis):
    from lc_amd import obox

    names = ("cloud:65", "cloud:1025", "offgrid:3", "tie-cube")
    got = _host(obox.oriented_box(_set(dev, names), axis=axis))
    a = "xyz".index(axis) if isinstance(axis, str) else axis
    _check(got, names, a)
    unit = np.eye(3, dtype=np.float32)[a]
    assert all(np.array_equal(X[a, :3], unit) and np.array_equal(X[:3, a], unit) for X in got["xform"])


@pytest.mark.parametrize("levels", [0, 1])
def test_fewer_levels(dev, levels):
    from lc_amd import obox

    names = ("cloud:257", "cloud:1025", "tie-cube")
    for axis in (None, 1):
        got = _host(obox.oriented_box(_set(dev, names), axis=axis, levels=levels))
        assert got["path"].shape == (3, levels + 1)
        _check(got, names, axis, levels)


def test_the_tie_at_the_lowest_score_goes_to_the_lower_index(dev):
    from lc_amd import obox
    from tests import obox_oracle as oracle

    want = cases.reference("tie-cube", None, 0)
    s = want.scores[0][0]
    tied = np.nonzero(s == s.min())[0]
    assert len(tied) == 2  # (tests/test_obox_host.py says which two)
    got = _host(obox.oriented_box(_set(dev, ["tie-cube"]), levels=0))
    assert got["path"][0, 0] == tied[0] and cases.same_bits(got["volume"][0], s.min())
    _check(got, ["tie-cube"], None, 0)
    assert oracle.winner(s) == tied[0]


def test_boxes_turned_off_the_grid_equal_the_oracle(dev):
    from lc_amd import obox

    names = [f"offgrid:{i}" for i in range(len(cases.OFF_GRID))]
    got = _host(obox.oriented_box(_set(dev, names)))
    _check(got, names)
    true = np.prod(np.asarray(cases.BOX_HALF, np.float64) * 2)
    print("volume over true:", (got["volume"] / true).tolist())  # (the figures of profiles/obox/offgrid_ratio.json: equality above says so)


def test_a_planted_nan_raises_info_and_leaves_the_other_meshes_alone(dev):
    from lc_amd import obox

    names = ("cloud:65", "cloud:1025", "cloud:257")
    ms = _set(dev, names)
    clean = _host(obox.oriented_box(ms))
    ms.verts[65 + 1024, 1] = float("nan")  # the last vertex of the second mesh: its second chunk
    got = _host(obox.oriented_box(ms))
    assert got["info"].tolist() == [0, 1, 0]
    for k in (0, 2):
        for f in cases.FIELDS:
            assert cases.same_bits(got[f][k], clean[f][k]), (k, f)
    _check({f: got[f][[0, 2]] for f in cases.FIELDS}, [names[0], names[2]])
    assert (got["path"][1] >= 0).all() and (got["path"][1, 0] < 1419) and (got["path"][1, 1:] < 125).all()
    ms.verts[65 + 1024, 1] = float("inf")
    assert obox.oriented_box(ms).info.tolist() == [0, 1, 0]


def test_a_second_call_and_a_replayed_graph_give_the_same_bits(dev):
    from lc_amd import obox

    ms = _set(dev, NAMES)
    first = _host(obox.oriented_box(ms))
    second = _host(obox.oriented_box(ms))
    _check(first, NAMES)
    assert all(cases.same_bits(first[f], second[f]) for f in cases.FIELDS)
    for axis in (None, 2):
        eager = _host(obox.oriented_box(ms, axis=axis))  # (also the warm-up: the mode's table is on the device before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            box = obox.oriented_box(ms, axis=axis)
        for _ in range(2):
            for t in box:
                t.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            replayed = _host(box)
            assert all(cases.same_bits(eager[f], replayed[f]) for f in cases.FIELDS), axis
