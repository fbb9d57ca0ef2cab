"""The training mask crops on the device (lc_amd.maskcrop, liblc_amd_maskcrop.so) against the numpy restatement of their contract
(tests/maskcrop_oracle.py): EQUAL bits for msk_vis, equal msk_noc, valid_cnt, check points and info -- every output is an integer, or an
integer over 1024."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import maskcrop_cases as cases, maskcrop_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _run(masks, M, out_hw, *, mask_index=None, origin=None, sample_id=None, **kw):
    from lc_amd import maskcrop

    return maskcrop.mask_crops(_dev(masks), _dev(M, torch.float32), out_hw,
                               mask_index=None if mask_index is None else _dev(mask_index, torch.int32),
                               origin=None if origin is None else _dev(origin, torch.int32),
                               sample_id=None if sample_id is None else _dev(sample_id, torch.int32), **kw)


def _same(got, want, what, rows=None):
    """Every output of a MaskCrops equal to the oracle's dict (rows: this selection of the oracle's rows)."""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    assert torch.equal(got.info.cpu(), torch.from_numpy(pick(want["info"]))), (what, "info")
    if got.msk_vis is not None:
        assert got.msk_vis.dtype == torch.float32
        assert torch.equal(got.msk_vis.view(torch.int32).cpu(), torch.from_numpy(pick(want["msk_vis"]).view(np.int32))), (what, "msk_vis bits")
    if got.msk_noc is not None:
        assert got.msk_noc.dtype == torch.bool
        assert torch.equal(got.msk_noc.cpu(), torch.from_numpy(pick(want["msk_noc"]))), (what, "msk_noc")
    if got.valid_cnt is not None:
        assert torch.equal(got.valid_cnt.cpu(), torch.from_numpy(pick(want["valid_cnt"]))), (what, "valid_cnt")
    if got.sym_ck_pts2d is not None:
        assert torch.equal(got.sym_ck_pts2d.cpu().long(), torch.from_numpy(pick(want["sym_ck_pts2d"]))), (what, "sym_ck_pts2d")


@pytest.mark.parametrize("vis_interp", ["linear", "nearest"])
def test_crops_equal_the_oracle(vis_interp):
    """1 x 1, 1 x 37, 37 x 1, one tile, a tile + 1 each way and 64 x 64 from windows of 5 x 7 up to 48 x 40: identity, fractional shift,
    rotations, 3 x zoom in and out, the stretched and skewed kind; positive and negative origins, each window edge, a window that is missed."""
    for case in cases.WARPS:
        window = cases.mask(case.mask_hw, case.seed)
        kw = dict(vis_interp=vis_interp, valid_th=1, n_check=16, seed=5)
        got = _run(window[None], [case.M], case.out_hw, origin=[case.origin], **kw)
        want = oracle.mask_crops(window[None], [case.M], case.out_hw, origin=[case.origin], **kw)
        _same(got, want, case.name)
        if case.name == "window-outside":
            assert got.valid_cnt.item() == 0 and not got.msk_vis.any() and (got.sym_ck_pts2d == -1).all()
        elif "edge" in case.name or "rot" in case.name:
            assert 0 < got.valid_cnt.item() < case.out_hw[0] * case.out_hw[1]
            if vis_interp == "linear":
                assert ((got.msk_vis > 0) & (got.msk_vis < 1)).any()


def _window_batch():
    masks = np.stack([cases.mask((12, 14), s) for s in (21, 22, -1)])
    names = ["edge-left", "edge-right", "edge-top", "edge-bottom", "window-outside", "edge-left", "edge-top", "edge-right", "edge-bottom"]
    by_name = {c.name: c for c in cases.WARPS}
    M = np.array([by_name[n].M for n in names], dtype=np.float32)
    origin = np.array([by_name[n].origin for n in names], dtype=np.int64)
    index = np.array([2, 0, 0, 1, 2, 7, 1, 1, 2], dtype=np.int32)  # repeats, out of order, row 5 out of range
    M[6, 1, 2] = np.nan
    M[1, 0, 0] = np.inf
    origin[8, 0] = -(1 << 24) - 1  # beyond the bound; row 7's lies on it
    origin[7] = (1 << 24, -(1 << 24))
    return masks, M, origin, index


@pytest.mark.parametrize("vis_interp", ["linear", "nearest"])
def test_windows_indices_and_refused_rows(vis_interp):
    masks, M, origin, index = _window_batch()
    kw = dict(vis_interp=vis_interp, valid_th=1, n_check=8, seed=1)
    got = _run(masks, M, (18, 19), mask_index=index, origin=origin, **kw)
    want = oracle.mask_crops(masks, M, (18, 19), mask_index=index, origin=origin, **kw)
    assert want["info"].tolist() == [0, -1, 0, 0, 0, -1, -1, 0, -1]
    _same(got, want, "windows")
    for b in (1, 5, 6, 8):  # written as all zero, neighbours untouched (they equal the oracle above)
        assert not got.msk_vis[b].any() and not got.msk_noc[b].any() and got.valid_cnt[b].item() == 0 and (got.sym_ck_pts2d[b] == -1).all()
    assert got.valid_cnt[0].item() > 0 and got.valid_cnt[2].item() > 0 and got.valid_cnt[4].item() == 0 and got.valid_cnt[7].item() == 0
    # without mask_index row b reads mask b: rows beyond the masks are refused
    got = _run(masks, M[:5], (18, 19), origin=origin[:5], **kw)
    want = oracle.mask_crops(masks, M[:5], (18, 19), origin=origin[:5], **kw)
    assert want["info"].tolist() == [0, -1, 0, -1, -1]
    _same(got, want, "no index")


VALID_TH = 100
COUNTS = (0, VALID_TH - 1, VALID_TH, 255, 256, 257, 64 * 64)


@functools.lru_cache(maxsize=None)
def _count_masks():
    return np.stack([cases.noc_with(v, (64, 64), seed=100 + i) for i, v in enumerate(COUNTS)])


@pytest.mark.parametrize("n_check", [0, 1, 255, 256])
def test_check_points_at_every_count(n_check):
    """valid_cnt of 0, valid_th - 1, valid_th (rounds of 100, 100, 56), 255, 256, 257 and all 4 096 pixels of a 64 x 64 crop under the
    identity; and with valid_th = 1 a single valid pixel (256 rounds of one), two and none."""
    masks = _count_masks()
    eye = np.tile(np.array(cases.EYE, dtype=np.float32), (len(COUNTS), 1, 1))
    sid = np.arange(len(COUNTS)) * 7 + 3
    kw = dict(valid_th=VALID_TH, n_check=n_check, seed=0xC0FFEE1234567, sample_id=sid)
    got = _run(masks, eye, (64, 64), **kw)
    want = oracle.mask_crops(masks, eye, (64, 64), **kw)
    assert want["valid_cnt"].tolist() == list(COUNTS)
    _same(got, want, "counts")
    assert got.sym_ck_pts2d.dtype == torch.int64 and tuple(got.sym_ck_pts2d.shape) == (len(COUNTS), n_check, 2)
    if n_check:
        assert (got.sym_ck_pts2d[:2] == -1).all() and (got.sym_ck_pts2d[2:] >= 0).all()
    few = np.stack([cases.noc_with(v, (64, 64), seed=200 + v) for v in (1, 2, 0)])
    kw = dict(valid_th=1, n_check=n_check, seed=9, ck_dtype=torch.int32)
    got = _run(few, eye[:3], (64, 64), **kw)
    kw.pop("ck_dtype")
    _same(got, oracle.mask_crops(few, eye[:3], (64, 64), **kw), "few")
    assert got.sym_ck_pts2d.dtype == torch.int32
    if n_check:
        y, x = np.nonzero(few[0])
        assert (got.sym_ck_pts2d[0].cpu() == torch.tensor([int(x[0]), int(y[0])])).all() and (got.sym_ck_pts2d[2] == -1).all()


def _offset_view(n, shape, dtype, fill):
    """A contiguous view of `shape` that starts ONE element into a filled buffer (aligned to the element and to no four of them), and the buffer."""
    flat = torch.full((n + 9,), fill, device=DEV, dtype=dtype)
    return flat[1:1 + n].view(shape), flat


@pytest.mark.parametrize("vis_interp", ["linear", "nearest"])
@pytest.mark.parametrize("case", cases.WIDE_WARPS, ids=lambda c: c.name)
def test_wide_crops_equal_the_oracle_in_every_thread_layout(case, vis_interp):
    """64, 128 and 256 threads along x, a second trip of the quad loop and the workload's 256 x 256 (tests/maskcrop_cases.WIDE_WARPS):
    msk_vis, msk_noc, valid_cnt and the check points; then into outputs one element off, which the launcher writes element by element
    at any w: the same bits, and nothing written around them."""
    window = cases.mask(case.mask_hw, case.seed)
    h, w = case.out_hw
    kw = dict(vis_interp=vis_interp, valid_th=1, n_check=16, seed=5)
    want = oracle.mask_crops(window[None], [case.M], case.out_hw, origin=[case.origin], **kw)
    got = _run(window[None], [case.M], case.out_hw, origin=[case.origin], **kw)
    _same(got, want, case.name)
    assert 0 < got.valid_cnt.item() < h * w
    assert (got.msk_vis.data_ptr() % 16 == 0 and got.msk_noc.data_ptr() % 4 == 0) or w % 4, "these outputs were meant to take the four-pixel stores"
    (vis, vis_buf), (noc, noc_buf) = _offset_view(h * w, (1, h, w), torch.float32, 7.0), _offset_view(h * w, (1, h, w), torch.uint8, 9)
    assert vis.data_ptr() % 16 == 4 and noc.data_ptr() % 4 == 1
    off = _run(window[None], [case.M], case.out_hw, origin=[case.origin], out=dict(msk_vis=vis, msk_noc=noc), **kw)
    assert off.msk_vis.data_ptr() == vis.data_ptr() and off.msk_noc.data_ptr() == noc.data_ptr()
    _same(off, want, case.name + " element by element")
    assert vis_buf[0].item() == 7.0 and (vis_buf[1 + h * w:] == 7.0).all() and noc_buf[0].item() == 9 and (noc_buf[1 + h * w:] == 9).all()


@pytest.mark.parametrize("ck_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("size", [64, 256])
def test_check_point_selection_at_every_depth_and_at_the_16_bit_limit(size, ck_dtype):
    """One launch per crop size under the identity: four rows whose selection ends after one, two, three and four byte passes
    (tests/maskcrop_cases.depth_ids), and at 256 x 256, where p fills its 16 bits, three rows more: only the last 300 pixels set, 200
    pixels in the last two rows (fewer than the check points: the rounds), and exactly 256 pixels with p = 0 and p = 65535 among them."""
    ids = cases.depth_ids(size)
    masks, index, sid = [cases.depth_crop(size)], [0, 0, 0, 0], [ids[d] for d in (0, 1, 2, 3)]
    if size == 256:
        for _, m, s in cases.large_p_masks():
            index.append(len(masks)), masks.append(m), sid.append(s)
    masks = np.stack(masks)
    B = len(index)
    eye = np.tile(np.array(cases.EYE, dtype=np.float32), (B, 1, 1))
    kw = dict(mask_index=np.array(index, dtype=np.int32), sample_id=np.array(sid, dtype=np.int32), valid_th=VALID_TH, n_check=cases.DEPTH_N, seed=cases.DEPTH_SEED)
    want = oracle.mask_crops(masks, eye, (size, size), **kw)
    depths = [oracle.selection_depth(masks[f], cases.DEPTH_N, cases.DEPTH_SEED, s) for f, s in zip(index, sid)]
    assert depths[:4] == [0, 1, 2, 3] and (size == 64 or (depths[4] in range(4) and depths[5:] == [None, None]))  # None: nothing is left out
    assert not want["info"].any() and (want["sym_ck_pts2d"] >= 0).all()
    got = _run(masks, eye, (size, size), ck_dtype=ck_dtype, **kw)
    assert got.sym_ck_pts2d.dtype == ck_dtype and tuple(got.sym_ck_pts2d.shape) == (B, cases.DEPTH_N, 2)
    _same(got, want, f"depth rows {size}")
    if size == 256:
        assert want["valid_cnt"].tolist() == [size * size] * 4 + [300, 200, 256]
        p = got.sym_ck_pts2d[:, :, 1].cpu().long() * size + got.sym_ck_pts2d[:, :, 0].cpu().long()
        assert (p[4] >= 65236).all() and (p[5] >= 254 * 256).all() and p[6].min().item() == 0 and p[6].max().item() == 65535
        assert (p[:4] >= 4096).any(dim=1).all()


def _random_rows(B, seed):
    rng = np.random.default_rng(seed)
    masks = np.stack([cases.mask((40, 44), s) for s in (31, 32, 33, 34, -1)])
    masks[3] &= (np.random.default_rng(35).random((40, 44)) < 0.12).astype(np.uint8)  # a sparse one: fewer valid pixels than check points
    index = rng.integers(0, 5, B).astype(np.int32)
    origin = rng.integers(-20, 20, (B, 2))
    M = np.array([cases.affine((o[0] + 22, o[1] + 20), rng.uniform(0.5, 2.5), (32, 48), rot=rng.uniform(0, 2 * math.pi), stretch=rng.uniform(0.7, 1.4),
                               skew=rng.uniform(-0.3, 0.3), shift=rng.uniform(-8, 8, 2)) for o in origin], dtype=np.float32)
    sid = rng.integers(0, 1 << 20, B).astype(np.int32)
    return masks, index, origin, M, sid


def test_batch_invariance_and_the_oracle_on_a_batch_of_33():
    """The same rows alone, and in a batch of 33 in another order with other neighbours: the same bits per row (sample_id follows the row)."""
    masks, index, origin, M, sid = _random_rows(33, 4)
    kw = dict(valid_th=105, n_check=256, seed=77)
    a = _run(masks, M, (32, 48), mask_index=index, origin=origin, sample_id=sid, **kw)
    _same(a, oracle.mask_crops(masks, M, (32, 48), mask_index=index, origin=origin, sample_id=sid, **kw), "batch of 33")
    # one round of a selection, several rounds of everything, and too few pixels: all three in the batch
    assert (a.valid_cnt >= 256).any() and ((a.valid_cnt >= 105) & (a.valid_cnt < 256)).any() and ((a.valid_cnt > 0) & (a.valid_cnt < 105)).any()
    perm = np.random.default_rng(8).permutation(33)
    b = _run(masks, M[perm], (32, 48), mask_index=index[perm], origin=origin[perm], sample_id=sid[perm], **kw)
    for name in ("msk_vis", "msk_noc", "valid_cnt", "sym_ck_pts2d", "info"):
        assert torch.equal(getattr(a, name)[_dev(perm, torch.int64)], getattr(b, name)), name
    for r in (0, 13, 32):
        c = _run(masks, M[r:r + 1], (32, 48), mask_index=index[r:r + 1], origin=origin[r:r + 1], sample_id=sid[r:r + 1], **kw)
        for name in ("msk_vis", "msk_noc", "valid_cnt", "sym_ck_pts2d", "info"):
            assert torch.equal(getattr(a, name)[r:r + 1], getattr(c, name)), (name, r)


def test_seed_and_sample_id_change_the_points_and_nothing_else():
    masks, index, origin, M, sid = _random_rows(6, 5)
    kw = dict(mask_index=index, origin=origin, valid_th=1, n_check=200)
    a = _run(masks, M, (32, 48), sample_id=sid, seed=1, **kw)
    b = _run(masks, M, (32, 48), sample_id=sid, seed=1 << 32, **kw)  # the high word alone
    c = _run(masks, M, (32, 48), sample_id=sid + 1, seed=1, **kw)
    assert (a.valid_cnt > 20).all() and (a.valid_cnt < 200).any()
    for other in (b, c):
        assert torch.equal(a.msk_vis, other.msk_vis) and torch.equal(a.msk_noc, other.msk_noc) and torch.equal(a.valid_cnt, other.valid_cnt)
        assert all(not torch.equal(a.sym_ck_pts2d[r], other.sym_ck_pts2d[r]) for r in range(6))
    _same(b, oracle.mask_crops(masks, M, (32, 48), sample_id=sid, seed=1 << 32, **kw), "high seed word")
    # every returned point lies on a set pixel, and a round holds no pixel twice
    p = a.sym_ck_pts2d.cpu()
    for r in range(6):
        assert a.msk_noc[r].cpu()[p[r, :, 1], p[r, :, 0]].all()
        first = min(200, int(a.valid_cnt[r]))
        assert len({(int(x), int(y)) for x, y in p[r, :first]}) == first


def test_wanted_outputs_out_tensors_and_msk_in():
    """`want` leaves the others out (the check points then live on the caller's workspace); `out=` is written in place; the input-size
    call of the docstring gives msk_in."""
    masks, index, origin, M, sid = _random_rows(4, 6)
    kw = dict(mask_index=index, origin=origin, sample_id=sid, valid_th=1, n_check=32, seed=3)
    want = oracle.mask_crops(masks, M, (32, 48), **kw)
    only = _run(masks, M, (32, 48), want=("sym_ck_pts2d",), **kw)
    assert only.msk_vis is None and only.msk_noc is None and only.valid_cnt is None
    _same(only, want, "points alone")
    two = _run(masks, M, (32, 48), want=("valid_cnt", "msk_noc"), **kw)
    assert two.msk_vis is None and two.sym_ck_pts2d is None
    _same(two, want, "count and mask")
    mine = dict(msk_vis=torch.full((4, 32, 48), 7.0, device=DEV), msk_noc=torch.full((4, 32, 48), 9, device=DEV, dtype=torch.uint8),
                info=torch.full((4,), 5, device=DEV, dtype=torch.int32))
    got = _run(masks, M, (32, 48), out=mine, **kw)
    assert got.msk_vis is mine["msk_vis"] and got.msk_noc.data_ptr() == mine["msk_noc"].data_ptr() and got.info is mine["info"]
    _same(got, want, "out=")
    msk_in = _run(masks, M, (33, 47), want=("msk_vis",), n_check=0, mask_index=index, origin=origin)
    _same(msk_in, oracle.mask_crops(masks, M, (33, 47), mask_index=index, origin=origin, n_check=0), "msk_in")
    assert msk_in.msk_noc is None and msk_in.sym_ck_pts2d is None
    empty = _run(masks, np.zeros((0, 2, 3), np.float32), (8, 8))
    assert tuple(empty.msk_vis.shape) == (0, 8, 8) and tuple(empty.sym_ck_pts2d.shape) == (0, 256, 2)


def test_graph_replay_on_changed_inputs():
    from lc_amd import maskcrop

    masks, index, origin, M, sid = _random_rows(5, 7)
    kw = dict(valid_th=20, n_check=256, seed=21)
    s_masks, s_M, s_idx, s_org, s_sid = _dev(masks), _dev(M), _dev(index), _dev(origin, torch.int32), _dev(sid)

    def call():
        return maskcrop.mask_crops(s_masks, s_M, (32, 48), mask_index=s_idx, origin=s_org, sample_id=s_sid, **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up: library load, allocator
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        held = call()
    for seed in (8, 9):
        masks2, index2, origin2, M2, sid2 = _random_rows(5, seed)
        for dst, src in ((s_masks, masks2), (s_M, M2), (s_idx, index2), (s_org, origin2.astype(np.int32)), (s_sid, sid2)):
            dst.copy_(_dev(src))
        g.replay()
        torch.cuda.synchronize()
        eager = _run(masks2, M2, (32, 48), mask_index=index2, origin=origin2, sample_id=sid2, **kw)
        for name in ("msk_vis", "msk_noc", "valid_cnt", "sym_ck_pts2d", "info"):
            assert torch.equal(getattr(held, name), getattr(eager, name)), (name, seed)
        _same(held, oracle.mask_crops(masks2, M2, (32, 48), mask_index=index2, origin=origin2, sample_id=sid2, **kw), f"replay {seed}")


def test_chain_from_render_to_labels():
    """render_depth -> gt_info_from_depth with a window and mask_visib -> mask_crops with that origin -> the native label path."""
    from lc_amd import gtinfo, labels, maskcrop, render
    from tests import render_cases as rc

    H, W, win = 48, 64, (30, 28)
    f = 1.25 * W
    Kn = np.array([[f, 0.0, W // 2], [0, 0.97 * f, H // 2], [0, 0, 1]], dtype=np.float32)
    names = ("ico", "torus")
    ms = render.MeshSet([rc.MESHES[m] for m in names], DEV)
    R, t = _dev(np.stack([rc.POSES[m].R for m in names])), _dev(np.stack([rc.POSES[m].t for m in names]))
    B = 2
    K = _dev(Kn).expand(B, 3, 3).contiguous()
    origin = torch.tensor([[20, 10], [14, 6]], dtype=torch.int32, device=DEV)
    Kr = K.clone()
    Kr[:, 0, 2] -= origin[:, 0].float()
    Kr[:, 1, 2] -= origin[:, 1].float()
    depth = render.render_depth(ms, ms.index_of([0, 1]), R, t, Kr, win, near=rc.NEAR, far=rc.FAR, pixel_center=(0.0, 0.0)).depth
    scene = np.random.default_rng(5).uniform(0.35, 1.0, size=(1, H, W)).astype(np.float32)
    rec = gtinfo.gt_info_from_depth(depth, _dev(scene), K, delta=0.015, origin_xy=origin)
    assert rec.mask_visib.dtype == torch.bool and (rec.info[:, 2] > 20).all()
    out_hw = (32, 32)
    box = rec.info[:, 8:12].cpu().numpy().astype(np.float64)  # the visible box, frame coordinates
    M = np.array([cases.affine(((b[0] + b[2]) / 2, (b[1] + b[3]) / 2), 32 / (1.5 * max(b[2] - b[0], b[3] - b[1], 1)), out_hw) for b in box], dtype=np.float32)
    got = maskcrop.mask_crops(rec.mask_visib, _dev(M), out_hw, origin=origin, valid_th=10, n_check=256, seed=4)
    want = oracle.mask_crops(rec.mask_visib.cpu().numpy().astype(np.uint8), M, out_hw, origin=origin.cpu().numpy(), valid_th=10, n_check=256, seed=4)
    _same(got, want, "chain")
    assert (got.valid_cnt > 10).all() and torch.equal(got.valid_cnt.cpu(), torch.from_numpy(want["msk_noc"].reshape(B, -1).sum(1).astype(np.int32)))
    ck, noc = got.sym_ck_pts2d, got.msk_noc
    for b in range(B):  # every returned check point lies on a set pixel of msk_noc
        assert noc[b][ck[b, :, 1], ck[b, :, 0]].all()
    # the label path takes both as they are: no conversion makes a new tensor
    assert ck.is_cuda and ck.to(torch.int64).contiguous().data_ptr() == ck.data_ptr()
    assert noc.is_cuda and noc.contiguous().view(torch.uint8).data_ptr() == noc.data_ptr()
    h, w = out_hw
    gen = torch.Generator().manual_seed(2)
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    z = 0.45 + 0.05 * torch.rand(B, h, w, generator=gen)
    homo_z = torch.stack((u * z, v * z, z), -1).to(DEV)
    Rt = torch.cat((R, t.reshape(B, 3, 1)), -1)
    K_out = torch.tensor([[60.0, 0, 16], [0, 60, 16], [0, 0, 1]], device=DEV).expand(B, 3, 3).contiguous()
    xyz_noc = torch.rand(B, 3, h, w, generator=gen).to(DEV)
    best, which = labels._select(1, [Rt[:, None].contiguous()], K_out, 256, xyz_map=xyz_noc, noc_scale=torch.full((B, 3), 0.2, device=DEV), homo_z=homo_z, ck=ck)
    assert torch.allclose(best, Rt) and which.cpu().tolist() == [0, 0]
    xyz = labels._targets(homo_z, Rt, K_out, msk=noc)[0]
    torch.cuda.synchronize()
    assert tuple(xyz.shape) == (B, h, w, 3) and torch.isfinite(xyz).all()
    assert not xyz[~noc].any() and xyz[noc].abs().sum() > 0  # the mask was read as a mask
