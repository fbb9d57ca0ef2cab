"""The depth rasteriser (lc_amd.render, lc_amd/csrc/render/lc_render.hip) on the GPU against the integer reference of
tests/render_grid.py, on scenes whose every intermediate is exact: depth bits, face, mask, info and homo_z bits are EQUAL on every pixel --
no tolerance, no excluded pixel.  What each scene is there for is asserted in tests/test_render_grid.py.  The device-side bounds checks,
which MeshSet keeps away from the wrapper, go through the C entry point with buffers in which a missing check would read and write
only memory this test allocated: a regression is a wrong picture, not a fault."""
import numpy as np
import pytest
import torch

from tests import render_grid as rg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = [s.name for s in rg.SCENES]
GROUPS = rg.groups()


@pytest.fixture(scope="module")
def meshes():
    from lc_amd.render import MeshSet

    return MeshSet([(s.verts, s.faces) for s in rg.SCENES], DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _render(meshes, names, pix2k=None):
    """One call over the scenes `names` of one group, a row each."""
    from lc_amd.render import render_depth

    scs = [rg.BY_NAME[n] for n in names]
    sc = scs[0]
    assert all(s.group == sc.group for s in scs)
    idx = torch.tensor([NAMES.index(n) for n in names], dtype=torch.int32, device=DEV)
    R, t, K = (_dev(np.stack(x)) for x in zip(*[(s.R, s.t, s.K) for s in scs]))
    M = None if pix2k is None else _dev(np.stack([pix2k] * len(scs)))
    return render_depth(meshes, idx, R, t, K, sc.size_hw, near=sc.near, far=sc.far, pixel_center=sc.center_px, want_face=True, want_homo=True, pix2k=M)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_row(out, b, ref, homo, what):
    depth, mask, face, hz = (x[b].cpu().numpy() for x in (out.depth, out.mask, out.face, out.homo_z))
    assert np.array_equal(_bits(depth), _bits(ref.depth)), f"{what}: depth bits differ on {(_bits(depth) != _bits(ref.depth)).sum()} pixels"
    assert np.array_equal(face, ref.face), f"{what}: face differs on {(face != ref.face).sum()} pixels"
    assert np.array_equal(mask, ref.mask), what
    assert int(out.info[b]) == ref.info, what
    assert np.array_equal(_bits(hz), _bits(homo)), f"{what}: homo_z bits differ on {(_bits(hz) != _bits(homo)).any(-1).sum()} pixels"


@pytest.mark.parametrize("name", NAMES)
def test_scene_equals_the_integer_reference(meshes, name):
    ref = rg.reference(name)
    _assert_row(_render(meshes, [name]), 0, ref, ref.homo_z, name)
    _assert_row(_render(meshes, [name], rg.PIX2K), 0, ref, ref.homo_z_pix2k, name + " (pix2k)")


@pytest.mark.parametrize("group", list(GROUPS), ids=[f"{k[0][0]}x{k[0][1]}-c{k[1][0]},{k[1][1]}-far{k[3]!r}" for k in GROUPS])
def test_batched_rows_equal_their_single_row_calls(meshes, group):
    names = GROUPS[group]
    single = [_render(meshes, [n]) for n in names]
    for order in (names, names[::-1]):
        out = _render(meshes, order)
        for b, n in enumerate(order):
            ref = rg.reference(n)
            _assert_row(out, b, ref, ref.homo_z, f"{n} as row {b} of {len(order)}")
            for got, want in zip(out, single[names.index(n)]):
                assert torch.equal(got[b], want[0])


# ---- the device-side bounds checks, through the C entry point ---------------------------------------------------------------------

WIDE = (rg.S(3) - 40, rg.S(3) - 40, rg.S(9) + 40, rg.S(9) + 40)
H = rg.Fr(1, 2)
A_PTS = [(rg.S(1), rg.S(12), H), (rg.S(5), rg.S(14), H), (rg.S(12), rg.S(1), H)]   # the mesh in front of B in memory: index -1 of B is its last vertex
B_PTS, B_FACES = rg.quad(*WIDE)                                                     # the mesh under test: 4 vertices
C_PTS = [(rg.S(1), rg.S(14), H), (rg.S(14), rg.S(13), H), (rg.S(13), rg.S(15), H)]  # the mesh behind it: index n_vert of B is its first vertex
ALL = rg.scene("bounds", A_PTS + B_PTS + C_PTS, [(0, 1, 2)], (16, 16), cam=rg.CAMERAS[1])  # one camera, one set of float32 vertices
FACES = np.array(B_FACES + [(-1, 1, 2), (0, 4, 2), (0, 1, 2), (0, 1, 2)], dtype=np.int32)  # B's four faces, then two of A's size: six allocated
TABLE = np.array([(0, 3, 4, 1),   # 0: A, its face stored behind B's
                  (3, 4, 0, 4),   # 1: B with the two faces of invalid indices
                  (3, 4, 0, 2),   # 2: B, valid faces only
                  (3, 4, 2, 4)],  # 3: B's vertices with faces 2..5
                 dtype=np.int32)
REF_A = rg.raster_int(ALL._replace(pts=ALL.pts[:3], faces=FACES[4:5]))
REF_B = rg.raster_int(ALL._replace(pts=ALL.pts[3:7], faces=FACES[:4]))
REF_B2 = rg.raster_int(ALL._replace(pts=ALL.pts[3:7], faces=FACES[:2]))


def _direct(idx, *, total_verts=10, total_faces=6, max_faces=4):
    """lc_render_depth_f32 on the buffers above; the workspace holds four records per row whatever max_faces says."""
    from lc_amd import _lib, render

    lib = render.load()
    B = len(idx)
    verts, faces, table, mi = _dev(ALL.verts), _dev(FACES), _dev(TABLE), torch.tensor(idx, dtype=torch.int32, device=DEV)
    R, t, K = (_dev(np.stack([a] * B)) for a in (ALL.R, ALL.t, ALL.K))
    Hh, Ww = ALL.size_hw
    depth = torch.full((B, Hh, Ww), 7.0, device=DEV)
    face = torch.full((B, Hh, Ww), 7, device=DEV, dtype=torch.int32)
    mask = torch.full((B, Hh, Ww), 7, device=DEV, dtype=torch.uint8)
    homo = torch.full((B, Hh, Ww, 3), 7.0, device=DEV)
    info = torch.full((B,), 7, device=DEV, dtype=torch.int32)
    ws = torch.zeros(B * 4 * render.RECORD_BYTES, device=DEV, dtype=torch.uint8)
    assert int(lib.lc_render_workspace_bytes(B, max_faces)) <= ws.numel()
    rc = lib.lc_render_depth_f32(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(table), _lib.ptr(mi), len(TABLE), total_verts, total_faces, max_faces,
                                 _lib.ptr(R), _lib.ptr(t), _lib.ptr(K), None, B, Hh, Ww, ALL.near, ALL.far, *ALL.center_px, _lib.ptr(depth),
                                 _lib.ptr(face), _lib.ptr(mask), _lib.ptr(homo), _lib.ptr(info), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    assert rc == 0, lib.lc_amd_render_last_error()
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (depth, face, mask, homo, info)]


def _assert_direct(got, b, ref):
    depth, face, mask, homo, info = got
    if ref is None:  # a refused table entry: the miss values and info = -1
        assert not depth[b].any() and (face[b] == -1).all() and not mask[b].any() and not homo[b].any() and info[b] == -1
        return
    assert np.array_equal(_bits(depth[b]), _bits(ref.depth)) and np.array_equal(face[b], ref.face) and np.array_equal(mask[b], ref.mask.astype(np.uint8))
    assert np.array_equal(_bits(homo[b]), _bits(ref.homo_z)) and info[b] == ref.info


def test_invalid_vertex_indices_cover_nothing():
    """Faces (-1, 1, 2) and (0, n_vert, 2): not drawn, not counted, and the two valid faces as without them.  Were an index honoured, it
    would name the neighbouring mesh's vertex, in front of the quad and inside the map -- a different picture (asserted here in integers)."""
    assert np.array_equal(REF_B.depth, REF_B2.depth) and np.array_equal(REF_B.face, REF_B2.face) and REF_B.info == 0 and REF_B.mask.sum() == 49
    honoured = rg.raster_int(ALL._replace(faces=np.array([(3, 4, 5), (3, 5, 6), (2, 4, 5), (3, 7, 5)], dtype=np.int32)))
    assert (honoured.face == 2).any() and (honoured.face == 3).any()
    got = _direct([1, 2, 0])
    for b, ref in enumerate((REF_B, REF_B2, REF_A)):
        _assert_direct(got, b, ref)


@pytest.mark.parametrize("what", ["n_face > max_faces", "vertex range passes total_verts", "face range passes total_faces"])
def test_refused_table_entries(what):
    """Row 0 names the refused entry, row 1 an entry that is fine under the same sizes and must come out as ever."""
    if what == "n_face > max_faces":
        got, good = _direct([1, 2], max_faces=2), REF_B2            # 4 faces against max_faces = 2
    elif what == "vertex range passes total_verts":
        got, good = _direct([2, 0], total_verts=6), REF_A           # vertices 3..6 against 6 in all
    else:
        got, good = _direct([3, 2], total_faces=5), REF_B2          # faces 2..5 against 5 in all
    _assert_direct(got, 0, None)
    _assert_direct(got, 1, good)
    assert good.mask.any()
