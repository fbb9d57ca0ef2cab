"""lc_amd.models on the MI355X: every output bit-equal to the numpy restatement of its definitions (tests/models_cases.py) at the sizes
around every boundary of the kernels -- the diameter's tile edge (models.DIAM_TILE), the register-resident limit of the farthest-point
selection (models.FPS_RESIDENT), with the diameter on both sides of it -- and on `tied_cases`: exact lattice inputs whose ties are placed
so that each merge level is asked to break one (a lane's two slots, the two waves of a tile, the tile's key, the partials in tile
order, the reducer's second round and its j across threads; the selection's 16 waves and its register slots or strided visits),
singly and as one set.  tests/test_models_host.py shows that each of these inputs tells the planted wrong merges from the definition.
Not reached: the reducer's in-thread `k == bk && r.z < bjv`, which needs two tiles of one tile row 256 tile numbers apart, that is a
mesh of more than 256 tile rows (65537 vertices, 2e9 pairs for the oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import models_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def models():
    from lc_amd import models as m

    return m


@pytest.fixture(scope="module")
def cases(models):
    return mc.named_cases(models.DIAM_TILE, models.FPS_RESIDENT)


@pytest.fixture(scope="module")
def oracle(cases):
    """name -> (lo, hi, diameter or None, pair or None, fps index and points at the case's largest count): computed once, shared, read only."""
    out = {}
    for name, (v, counts, want_d) in cases.items():
        lo, hi = mc.extents(v)
        d, pair = mc.diameter(v) if want_d else (None, None)
        idx, pts = mc.fps(v, max(counts))
        out[name] = (lo, hi, d, pair, idx, pts)
    return out


TIED_PICKS = 64  # the largest fps_count of a tied case: the set takes it for every row, a case alone its own (a prefix)


@pytest.fixture(scope="module")
def tied(models):
    return mc.tied_cases(models.DIAM_TILE, models.FPS_RESIDENT)


@pytest.fixture(scope="module")
def tied_oracle(tied):
    """name -> (lo, hi, diameter, pair, fps index and points at TIED_PICKS picks): computed once, shared, read only."""
    assert all(c.fps_count <= TIED_PICKS <= len(c.verts) for c in tied.values())
    return {name: (*mc.extents(c.verts), *mc.diameter(c.verts), *mc.fps(c.verts, TIED_PICKS)) for name, c in tied.items()}


def _mesh_set(*verts):
    from lc_amd.render import MeshSet

    return MeshSet([(v, mc.FACES0) for v in verts], DEV)


def _same(t, ref):
    ref = np.asarray(ref)
    got = t.detach().cpu().numpy()
    return got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


CASE_NAMES = ["V1", "V2", "V3", "V63", "V64", "V65", "tile-1", "tile", "tile+1", "2tiles+1", "rows", "resident", "resident+1", "cube_duplicates",
              "collinear", "mm_offset"]


def test_case_names_follow_the_exported_constants(models, cases):
    assert sorted(CASE_NAMES) == sorted(cases)
    T, R = models.DIAM_TILE, models.FPS_RESIDENT
    assert [len(cases[n][0]) for n in ("tile-1", "tile", "tile+1", "2tiles+1", "resident", "resident+1")] == [T - 1, T, T + 1, 2 * T + 1, R, R + 1]
    assert len(cases["rows"][0]) > 4 * T  # several tile rows


@pytest.mark.parametrize("name", CASE_NAMES)
def test_single_mesh_equals_the_oracle_bit_for_bit(models, cases, oracle, name):
    v, counts, want_d = cases[name]
    lo, hi, d, pair, idx, pts = oracle[name]
    ms = _mesh_set(v)
    for c in counts:
        info = models.prepare(ms, c, want_diameter=want_d)
        assert _same(info.lo, lo[None]) and _same(info.hi, hi[None])
        if want_d:
            assert _same(info.diameter, np.asarray([d], np.float32)), (info.diameter.item(), float(d))
            assert info.pair.cpu().tolist() == [list(pair)]
        else:
            assert info.diameter is None and info.pair is None
        assert info.fps_index.cpu().numpy().tolist() == [idx[:c].tolist()]  # also: the c-point result is a prefix of the largest one
        assert _same(info.fps, pts[None, :c])


def _assert_row(info, k, ref, count):
    lo, hi, d, pair, idx, pts = ref
    assert _same(info.lo[k], lo) and _same(info.hi[k], hi)
    assert _same(info.diameter[k:k + 1], np.asarray([d], np.float32)), (info.diameter[k].item(), float(d))
    assert info.pair[k].cpu().tolist() == list(pair)
    assert info.fps_index[k].cpu().tolist() == idx[:count].tolist()
    assert _same(info.fps[k], pts[:count])


def test_tied_case_names_follow_the_exported_constants(models, tied):
    assert tuple(tied) == mc.TIED_NAMES
    T, R = models.DIAM_TILE, models.FPS_RESIDENT
    assert [len(tied[n].verts) for n in ("lane-slots", "waves", "tile-order", "reduce-two-rounds", "fps-ties-streaming")] == [T, T, 4 * T + 76, 23 * T + 1, R + 300]
    assert 2 * 1024 < len(tied["fps-ties-resident"].verts) < 3 * 1024 <= R  # three register slots, the last partly filled


@pytest.mark.parametrize("name", mc.TIED_NAMES)
def test_tied_case_equals_the_oracle_bit_for_bit(models, tied, tied_oracle, name):
    """Exact ties placed at one merge level each (`forces`): the definition's smallest (i, j) and smallest index, not a merge's own order."""
    c = tied[name]
    info = models.prepare(_mesh_set(c.verts), c.fps_count)
    print(name, c.forces, "pair", info.pair.cpu().tolist()[0], "first picks", info.fps_index[0, :4].cpu().tolist())
    _assert_row(info, 0, tied_oracle[name], c.fps_count)
    if c.pair is not None:
        assert tuple(info.pair.cpu().tolist()[0]) == c.pair


def test_tied_cases_as_one_shuffled_set(models, tied, tied_oracle):
    """All tied cases in one call, in a fixed shuffled order (vertex offsets, partial slots and, for the streaming one, a distance
    row that is not the first): each row is its single-mesh result and the oracle's."""
    names = [mc.TIED_NAMES[k] for k in np.random.default_rng(5).permutation(len(mc.TIED_NAMES))]
    assert names != list(mc.TIED_NAMES) and names.index("fps-ties-streaming") > 0
    info = models.prepare(_mesh_set(*(tied[n].verts for n in names)), TIED_PICKS)
    for k, n in enumerate(names):
        single = models.prepare(_mesh_set(tied[n].verts), TIED_PICKS)
        assert all(torch.equal(a[k:k + 1], b) for a, b in zip(info, single)), n
        _assert_row(info, k, tied_oracle[n], TIED_PICKS)


def test_tie_rules_on_the_cube(models, cases, oracle):
    """36 index pairs share the largest distance and eight corners the first pick: the smallest (i, j) and the lowest index win."""
    v = cases["cube_duplicates"][0]
    info = models.prepare(_mesh_set(v), 24)
    sq = mc.d2(v[:, None], v[None])
    cand = [(a, b) for a in range(len(v)) for b in range(a + 1, len(v)) if sq[a, b] == sq.max()]
    assert len(cand) == 36 and tuple(info.pair.cpu().tolist()[0]) == min(cand)
    first = mc.d2(v, (v.min(0) + v.max(0)) * np.float32(0.5))
    assert (first == first.max()).sum() == len(v) and info.fps_index[0, 0].item() == 0
    assert info.fps_index.cpu().tolist()[0] == oracle["cube_duplicates"][4].tolist()


def test_a_set_of_meshes_equals_the_single_mesh_calls(models, cases, oracle):
    """Three meshes of different sizes in one call (vertex offsets, a grid of several meshes whose tile counts differ), one of them
    past the resident limit: each row is the single-mesh result."""
    names = ("rows", "V3", "resident+1", "tile+1")
    info = models.prepare(_mesh_set(*(cases[n][0] for n in names)), 3)
    for k, n in enumerate(names):
        lo, hi, d, pair, idx, pts = oracle[n]
        assert _same(info.lo[k], lo) and _same(info.hi[k], hi)
        assert _same(info.fps[k], pts[:3]) and info.fps_index[k].cpu().tolist() == idx[:3].tolist()
        assert _same(info.diameter[k:k + 1], np.asarray([d], np.float32)) and info.pair[k].cpu().tolist() == list(pair), n
    assert names[2] == "resident+1" and oracle["resident+1"][2] is not None  # row 2: 33 tile rows among smaller meshes, against the oracle above
    single = models.prepare(_mesh_set(cases["resident+1"][0]), 3)  # and against the mesh alone
    assert torch.equal(info.diameter[2:3], single.diameter) and torch.equal(info.pair[2:3], single.pair)


def test_fps_counts_and_prefixes(models):
    v = mc.cloud(700, 21)
    ms = _mesh_set(v)
    idx, pts = mc.fps(v, 256)
    big, small = models.prepare(ms, 256, want_diameter=False), models.prepare(ms, 16, want_diameter=False)
    assert big.fps_index.cpu().tolist() == [idx.tolist()] and _same(big.fps, pts[None])
    assert torch.equal(big.fps[:, :16], small.fps) and torch.equal(big.fps_index[:, :16], small.fps_index)
    one = models.prepare(ms, 1, want_diameter=False)
    assert torch.equal(one.fps, big.fps[:, :1])
    w = mc.cloud(300, 22)
    full = models.prepare(_mesh_set(w), 300, want_diameter=False)  # count = V: every vertex once
    assert sorted(full.fps_index.cpu().tolist()[0]) == list(range(300)) and full.fps_index.cpu().tolist()[0] == mc.fps(w, 300)[0].tolist()


def test_streaming_form_prefix_and_counts(models, cases):
    """Past the resident limit the distances live in the workspace: 40 picks against the oracle, and their first 16 against the 16-pick call."""
    v = cases["resident+1"][0]
    ms = _mesh_set(v)
    idx, pts = mc.fps(v, 40)
    a, b = models.prepare(ms, 40, want_diameter=False), models.prepare(ms, 16, want_diameter=False)
    assert a.fps_index.cpu().tolist() == [idx.tolist()] and _same(a.fps, pts[None])
    assert torch.equal(a.fps[:, :16], b.fps)


def test_two_streaming_meshes_around_a_resident_one(models, cases, oracle, tied, tied_oracle):
    """Two streaming rows of different lengths, so that the second one's distances start at its own row of the workspace
    (`mind + m * mind_stride`), at one pick -- the distances are never written -- and at 40: each row is its single-mesh oracle result."""
    R = models.FPS_RESIDENT
    a, b, c = cases["resident+1"][0], cases["V65"][0], tied["fps-ties-streaming"].verts
    assert (len(a), len(b), len(c)) == (R + 1, 65, R + 300)
    idx_a, pts_a = mc.fps(a, 40)
    refs = (oracle["resident+1"][:4] + (idx_a, pts_a), oracle["V65"], tied_oracle["fps-ties-streaming"])
    ms = _mesh_set(a, b, c)
    for count in (1, 40):
        info = models.prepare(ms, count)
        for k, ref in enumerate(refs):
            _assert_row(info, k, ref[:4] + (ref[4][:count], ref[5][:count]), count)


def test_streaming_form_takes_every_vertex_once(models, cases):
    """fps_count = V past the resident limit: a permutation of the vertices, the oracle's."""
    v = cases["resident+1"][0]
    idx, pts = mc.fps(v, len(v))
    full = models.prepare(_mesh_set(v), len(v), want_diameter=False)
    got = full.fps_index.cpu().numpy()[0]
    assert np.array_equal(np.sort(got), np.arange(len(v))) and np.array_equal(got, idx) and _same(full.fps, pts[None])


def test_each_part_is_skipped_through_its_null_output(models, cases, oracle):
    v = cases["rows"][0]
    lo, hi, d, pair, idx, pts = oracle["rows"]
    ms = _mesh_set(v)
    only_ext = models.prepare(ms, 0, want_diameter=False)
    assert only_ext.diameter is None and only_ext.fps is None and _same(only_ext.lo, lo[None]) and _same(only_ext.hi, hi[None])
    only_dia = models.prepare(ms, 0, want_diameter=True, want_extents=False)
    assert only_dia.lo is None and only_dia.fps is None and _same(only_dia.diameter, np.asarray([d], np.float32)) and only_dia.pair.cpu().tolist() == [list(pair)]
    only_fps = models.prepare(ms, 16, want_diameter=False, want_extents=False)
    assert only_fps.lo is None and only_fps.diameter is None and _same(only_fps.fps, pts[None, :16])
    # single pointers of a part through the C entry point: the other one is still written
    from lc_amd import _lib

    lib = models.load()
    dia = torch.full((1,), -1.0, device=DEV)
    idx_t = torch.full((1, 16), -1, device=DEV, dtype=torch.int32)
    hi_t = torch.full((1, 3), 7.0, device=DEV)
    n = lib.lc_model_workspace_bytes(1, len(v), 16)
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    rc = lib.lc_model_prepare_f32(_lib.ptr(ms.verts), _lib.ptr(ms.table), ms.table_host.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, len(v), 16, None,
                                  _lib.ptr(hi_t), _lib.ptr(dia), None, None, _lib.ptr(idx_t), _lib.ptr(ws), n, _lib.stream_ptr(ms.device))
    assert rc == 0
    assert _same(dia, np.asarray([d], np.float32)) and _same(hi_t, hi[None]) and idx_t.cpu().tolist() == [idx[:16].tolist()]


def test_two_streams_give_the_same_bits(models, cases):
    ms = _mesh_set(cases["rows"][0], cases["tile+1"][0])
    ref = models.prepare(ms, 16)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(models.prepare(ms, 16))
    torch.cuda.synchronize()
    for o in outs:
        assert all(torch.equal(a, b) for a, b in zip(o, ref))


def test_capture_and_replay_give_the_same_bits(models, cases):
    ms = _mesh_set(cases["rows"][0], cases["V65"][0])
    ref = models.prepare(ms, 16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = models.prepare(ms, 16)
    for t in out:
        t.fill_(0) if t.dtype == torch.float32 else t.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, ref))


def test_more_points_than_vertices_raise_before_any_launch(models, cases):
    v = cases["V65"][0]
    with pytest.raises(ValueError, match="fps_count 66 exceeds the 65 vertices of mesh 1"):
        models.prepare(_mesh_set(cases["rows"][0], v), len(v) + 1)
    with pytest.raises(ValueError):
        models.prepare(_mesh_set(v), -1)
    with pytest.raises(TypeError):
        models.prepare([v], 4)
