"""The crop geometry drawn on the device (`lc_amd.geometry.zoom_geometry`, `background_geometry`) against its definition in host numpy
(`zoom_geometry_host`, `augment.background_matrices`): every field by bit pattern, NaNs by position.  Batches and edge draws are those of
tests/geometry_cases.py."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

IM_HW, IN_WH, OUT_WH = (480, 640), (256, 192), (128, 96)
SEEDS = (7, 4294967301, 9223372036854788153)  # one half, both halves, above 2^63
FIELDS = ("in_affine", "out_affine", "out_K", "out_pix_scale", "step_id", "info", "centre", "scale", "cs")  # all but rot, which the device leaves out
B_ROWS = 67  # one full wavefront and a ragged one


def _cfg(rotate_prob=0.5):
    from lc_amd import augment

    return augment.AugmentConfig(rotate_prob=rotate_prob)


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    """Same type, shape and bit patterns; a NaN matches a NaN at the same place, whatever its payload."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def device(cfg, seed, ids, box, K, train=True, im_hw=IM_HW, in_wh=IN_WH, out_wh=OUT_WH):
    from lc_amd import geometry

    g = geometry.zoom_geometry(cfg, seed=seed, sample_id=_dev(ids, torch.int32), bbox_xyxy=_dev(box), im_hw=im_hw, cam_K=_dev(K), in_wh=in_wh, out_wh=out_wh,
                               train=train, want_info=True)
    torch.cuda.synchronize()
    assert g.rot is None
    return g


def host(cfg, seed, ids, box, K, train=True, im_hw=IM_HW, in_wh=IN_WH, out_wh=OUT_WH):
    from lc_amd import geometry

    return geometry.zoom_geometry_host(cfg, seed, ids, box, im_hw, K, in_wh, out_wh, train=train)


def assert_equal(g, h, rows=None, what=""):
    for name in FIELDS:
        a, b = getattr(g, name), getattr(h, name)
        a = a.cpu().numpy()
        if rows is not None:
            a, b = a[rows], b[rows]
        assert same(a, b), (what, name, np.argwhere(_bits(a) != _bits(b))[:4].tolist())


@pytest.mark.parametrize("train", [True, False])
def test_every_field_equals_the_host_definition(train):
    ids, box, K = gc.batch(B_ROWS, 1)
    gated = set()
    for seed in SEEDS:
        for prob in (1.0, 0.5, 0.0):
            cfg = _cfg(prob)
            g, h = device(cfg, seed, ids, box, K, train), host(cfg, seed, ids, box, K, train)
            assert_equal(g, h, what=(seed, prob))
            assert (h.info == 0).all()
            gated.add((prob, bool((h.cs[:, 1] != 0).any()), bool((h.cs[:, 1] == 0).any())))
    if train:  # the gate was open for every row, for some, for none
        assert gated == {(1.0, True, False), (0.5, True, True), (0.0, False, True)}
        assert (h.scale == 640.0).sum() >= B_ROWS // 5  # and the clamp of max(im_h, im_w) is met
    else:
        assert all(not rotated for _, rotated, _ in gated)


def test_without_want_info_the_three_are_left_out():
    from lc_amd import geometry

    ids, box, K = gc.batch(5, 2)
    g = geometry.zoom_geometry(_cfg(), seed=3, sample_id=_dev(ids, torch.int32), bbox_xyxy=_dev(box), im_hw=IM_HW, cam_K=_dev(K), in_wh=IN_WH, out_wh=OUT_WH)
    h = host(_cfg(), 3, ids, box, K)
    assert g.centre is None and g.scale is None and g.cs is None and g.rot is None
    assert all(same(getattr(g, n), getattr(h, n)) for n in FIELDS[:6])
    empty = geometry.zoom_geometry(_cfg(), seed=3, sample_id=_dev(ids[:0], torch.int32), bbox_xyxy=_dev(box[:0]), im_hw=IM_HW, cam_K=_dev(K[0]), in_wh=IN_WH,
                                   out_wh=OUT_WH)
    assert tuple(empty.in_affine.shape) == (0, 2, 3) and tuple(empty.info.shape) == (0,)


def test_edge_draws_of_the_angle():
    """u4 on each of the 16 octant edges and on the largest draw: the reduced argument is 0 or comes from above, (c, s) hold exact zeros
    (of either sign) and +-1."""
    cfg = _cfg(1.0)
    seen = []
    for seed in gc.EDGE_SEEDS:
        ids = gc.edge_ids(seed)
        _, box, K = gc.batch(len(ids), 3)
        g, h = device(cfg, seed, ids, box, K), host(cfg, seed, ids, box, K)
        assert_equal(g, h, what=seed)
        seen.append(g.cs.cpu().numpy())
    cs = np.concatenate(seen)
    assert len(cs) == len(gc.EDGE_DRAWS) == 17
    assert sum(sorted(np.abs(r).tolist()) == [0.0, 1.0] for r in cs) == 8  # the eight quarter turns
    assert (cs == 1.0).any() and (cs == -1.0).any() and (np.signbit(cs) & (cs == 0)).any()  # a negative zero is kept as the host has it


def test_bad_rows_are_refused_as_nan_next_to_unchanged_neighbours():
    cfg = _cfg()
    ids, box, K = gc.batch(13, 5)
    box2, K2 = box.copy(), K.copy()
    box2[1, 0] = np.nan
    box2[3, 3] = np.inf
    box2[5, 1] = -np.inf
    K2[7, 1, 1] = np.nan
    K2[9, 2, 2] = np.inf
    box2[11, [0, 2]] = box2[11, [2, 0]]
    box2[11, [1, 3]] = box2[11, [3, 1]]  # inverted: a negative width and height, scale <= 0
    bad = np.array([1, 3, 5, 7, 9, 11])
    good = np.setdiff1d(np.arange(13), bad)
    for train in (True, False):
        if not train:  # max(w, h, 1) keeps an inverted box's scale positive there: the host says so too
            bad, good = bad[:-1], np.append(good, 11)
        clean = host(cfg, 9, ids, box, K, train)
        g, h = device(cfg, 9, ids, box2, K2, train), host(cfg, 9, ids, box2, K2, train)
        assert_equal(g, h, what=train)
        info = g.info.cpu().numpy()
        assert (info[bad] == -1).all() and (info[good] == 0).all()
        for name in ("in_affine", "out_affine", "out_K", "out_pix_scale", "centre", "scale"):
            assert np.isnan(getattr(g, name).cpu().numpy()[bad]).all(), name
        assert_equal(g, clean, rows=np.setdiff1d(good, [11]), what="neighbours")
        assert same(g.step_id, clean.step_id)  # written for a refused row as for any


def test_a_row_is_the_same_alone_permuted_and_in_any_batch():
    cfg = _cfg()
    ids, box, K = gc.batch(65, 7)
    whole = device(cfg, 21, ids, box, K)
    assert_equal(whole, host(cfg, 21, ids, box, K))
    perm = np.random.default_rng(0).permutation(65)
    part = device(cfg, 21, ids[perm], box[perm], K[perm])
    for name in FIELDS:
        assert same(getattr(part, name).cpu().numpy(), getattr(whole, name).cpu().numpy()[perm]), name
    for b in (0, 63, 64):  # a batch of 1: the last lane of the first wavefront, the lone lane of the second
        one = device(cfg, 21, ids[b:b + 1], box[b:b + 1], K[b:b + 1])
        for name in FIELDS:
            assert same(getattr(one, name).cpu().numpy(), getattr(whole, name).cpu().numpy()[b:b + 1]), (b, name)


def test_one_camera_serves_all_rows():
    cfg = _cfg()
    ids, box, K = gc.batch(B_ROWS, 8)
    one = device(cfg, 5, ids, box, K[4])
    every = device(cfg, 5, ids, box, np.ascontiguousarray(np.broadcast_to(K[4], (B_ROWS, 3, 3))))
    for name in FIELDS:
        assert same(getattr(one, name), getattr(every, name).cpu().numpy()), name
    assert_equal(one, host(cfg, 5, ids, box, K[4]))


def test_a_replayed_graph_follows_its_seed_word():
    from lc_amd import geometry

    cfg = _cfg()
    ids, box, K = gc.batch(B_ROWS, 9)
    s_ids, s_box, s_K = _dev(ids, torch.int32), _dev(box), _dev(K)
    seed = SEEDS[2]
    word = torch.full((1,), seed - 2 ** 64, dtype=torch.int64, device=DEV)

    def call():
        return geometry.zoom_geometry(cfg, seed=word, sample_id=s_ids, bbox_xyxy=s_box, im_hw=IM_HW, cam_K=s_K, in_wh=IN_WH, out_wh=OUT_WH, want_info=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        res = call()
    seen = []
    for step in (0, 1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert_equal(res, host(cfg, seed + step, ids, box, K), what=step)
        seen.append(res.in_affine.cpu().clone())
        word.add_(1)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    u64 = torch.from_numpy(np.array([seed], dtype=np.uint64)).to(DEV)  # the same bits as a uint64 word
    by_word = geometry.zoom_geometry(cfg, seed=u64, sample_id=s_ids, bbox_xyxy=s_box, im_hw=IM_HW, cam_K=s_K, in_wh=IN_WH, out_wh=OUT_WH, want_info=True)
    torch.cuda.synchronize()
    assert_equal(by_word, host(cfg, seed, ids, box, K))


def test_background_matrices_equal_the_host_ones():
    from lc_amd import augment, geometry

    ids = np.arange(-5, 62).astype(np.int32)
    s_ids = _dev(ids)
    out_hw = (64, 48)
    pairs = np.stack((np.arange(67) * 7 + 40, np.arange(67)[::-1] * 11 + 30), axis=1).astype(np.int32)  # some smaller than the crop, in either direction
    assert (pairs[:, 0] < 64).any() and (pairs[:, 1] < 48).any() and ((pairs[:, 0] > 64) & (pairs[:, 1] > 48)).any()
    for seed in SEEDS:
        for hw in ((100, 120), (64, 48), (30, 200), (20, 16)):  # larger, equal, mixed, smaller than the crop
            got = geometry.background_geometry(seed=seed, sample_id=s_ids, bg_hw=hw, out_hw=out_hw)
            assert same(got, augment.background_matrices(seed, ids, hw, out_hw)), (seed, hw)
        got = geometry.background_geometry(seed=seed, sample_id=s_ids, bg_hw=_dev(pairs), out_hw=out_hw)
        want = augment.background_matrices(seed, ids, pairs, out_hw)
        assert same(got, want) and same(got, geometry.background_geometry_host(seed, ids, pairs, out_hw)), seed
    word = torch.full((1,), SEEDS[1], dtype=torch.int64, device=DEV)
    assert same(geometry.background_geometry(seed=word, sample_id=s_ids, bg_hw=_dev(pairs), out_hw=out_hw), augment.background_matrices(SEEDS[1], ids, pairs, out_hw))
    assert tuple(geometry.background_geometry(seed=1, sample_id=s_ids[:0], bg_hw=(9, 9), out_hw=out_hw).shape) == (0, 2, 3)
