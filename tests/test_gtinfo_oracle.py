"""The annotation oracle (tests/gtinfo_oracle.py) without a GPU: hand-worked 3 x 4 frames whose records are written out here, the hand-made
cases of tests/gtinfo_cases.py read pixel by pixel, the margin condition that makes equality with the device a fair demand on every case,
the float64 torch statement held to the numpy one, and the relation to the VSD oracle: the visible set is tests/vsd_oracle.py's vis_gt."""
import numpy as np
import pytest
import torch

from tests import gtinfo_cases as C
from tests import gtinfo_oracle as oracle

NAN, INF = np.nan, np.inf
K34 = np.array([[100, 0, 2], [0, 100, 1], [0, 0, 1]], dtype=np.float32)  # 1 <= n < 1.001 over the 3 x 4 frame
TEST34 = np.array([[1, 1, 1, 1],
                   [1, 0, 1, 1],
                   [1, 1, 0.5, 1]], dtype=np.float32)


def test_hand_worked_full_frame():
    gt = np.array([[0, 1.0, 1.0, 0],
                   [0, 1.0, 1.2, 0],
                   [0, 0, 1.0, 0]], dtype=np.float32)
    r = oracle.record(gt, TEST34, K34, 0.1)
    # five hits; (1,1) has no measurement: visible, not valid; (1,2) lies 0.2 n behind the scene and (2,2) 0.5 n: hidden
    # the border of the full-frame window holds (0,1), (0,2) and (2,2)
    assert r.info.tolist() == [5, 4, 3, 3, 1, 0, 2, 2, 1, 0, 2, 1]
    assert r.mask_visib.tolist() == [[0, 1, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]] and r.mask_visib.dtype == np.uint8
    assert r.info.dtype == np.int32 and r.obj.sum() == 5


def test_hand_worked_window_reaching_outside():
    # a 2 x 3 window at (-1, 1): window pixel (x,y) is frame pixel (x - 1, y + 1)
    gt = np.array([[1.0, 1.0, 1.0],
                   [0, 0, 1.0]], dtype=np.float32)
    r = oracle.record(gt, TEST34, K34, 0.1, origin_xy=(-1, 1))
    # (0,0) -> (-1,1): outside, a hit and no more.  (1,0) -> (0,1): scene 1, visible.  (2,0) -> (1,1): no measurement, visible, not valid.
    # (2,1) -> (1,2): scene 1, visible.  Every pixel of a two-row window lies on its border.
    assert r.info.tolist() == [4, 2, 3, 4, -1, 1, 1, 2, 0, 1, 1, 2]
    assert r.mask_visib.tolist() == [[0, 1, 1], [0, 0, 1]]
    # the same window wholly outside: the hits count, nothing else, and the box is where the window lies
    r = oracle.record(gt, TEST34, K34, 0.1, origin_xy=(4, -2))
    assert r.info.tolist() == [4, 0, 0, 4, 4, -2, 6, -1, -1, -1, -1, -1] and not r.mask_visib.any()
    r = oracle.record(np.zeros((2, 3), np.float32), TEST34, K34, 0.1, origin_xy=(0, 0))
    assert r.info.tolist() == [0, 0, 0, 0] + [-1] * 8


def test_hand_worked_batch_and_composition():
    gt = np.stack([np.array([[0, 1.0, 1.0, 0], [0, 1.0, 1.2, 0], [0, 0, 1.0, 0]], dtype=np.float32)] * 3)
    test = np.stack([TEST34, np.zeros_like(TEST34)])
    info, mask, _ = oracle.records(gt, test, K34, 0.1, np.array([0, 2, 1], np.int32))
    assert info[0].tolist() == [5, 4, 3, 3, 1, 0, 2, 2, 1, 0, 2, 1]
    assert (info[1] == -1).all() and not mask[1].any()  # scene 2 of two: refused
    assert info[2].tolist() == [5, 0, 5, 3, 1, 0, 2, 2, 1, 0, 2, 2] and np.array_equal(mask[2] > 0, gt[2] > 0)  # nothing measured: all visible
    # three full-frame rows of one 2 x 3 scene: the nearest wins, the lowest row among equals, and 0, negative, NaN and inf are no hits
    inst = np.array([[[1, 0, 2], [0, 0, NAN]],
                     [[1, 3, 1], [INF, -1, 0]],
                     [[0.5, 0, 1], [0, 0, 0]]], dtype=np.float32)
    c = oracle.compose(inst, np.zeros(3, np.int32), (2, 3), 1)
    assert c.depth.tolist() == [[[0.5, 3, 1], [0, 0, 0]]] and c.instance.tolist() == [[[2, 1, 1], [-1, -1, -1]]] and c.info.tolist() == [0, 0, 0]
    # the same rows in two scenes, the last one skipped, and windows: row 1 moved one column to the right drops its last column
    c = oracle.compose(inst, np.array([0, 1, 7], np.int32), (2, 3), 2, origins=np.array([[0, 0], [1, 0], [0, 0]]))
    assert c.depth.tolist() == [[[1, 0, 2], [0, 0, 0]], [[0, 1, 3], [0, 0, 0]]]
    assert c.instance.tolist() == [[[0, -1, 0], [-1, -1, -1]], [[-1, 1, 1], [-1, -1, -1]]] and c.info.tolist() == [0, 0, -1]


def test_hand_made_cases_say_what_they_are_meant_to():
    info, mask, _ = C.expected("values-7x9")
    c = C.case("values-7x9")
    assert info[0].tolist() == [0, 0, 0, 0] + [-1] * 8 and not mask[0].any()  # an empty render
    # row 1, a full silhouette 5 mm behind a scene of depth 1: the four special scene pixels (0, negative, NaN: no measurement; +inf: a
    # measurement infinitely far) are all visible, three of them not valid; row 5 of the scene lies in front by 105 mm and hides nine pixels
    assert info[1].tolist() == [63, 60, 54, 28, 0, 0, 8, 6, 0, 0, 8, 6] and mask[1, 1, 1:5].all() and not mask[1, 5].any()
    # row 2: NaN, negative and 0 in the render are no hits; +inf is a hit that nothing measured can leave visible
    assert info[2, 0] == 60 and info[2, 2] == 50 and not mask[2, 2, 2:5].any() and not mask[2, 3, 3] and np.isinf(c.depth_gt[2, 3, 3])
    info, mask, _ = C.expected("threshold-7x9")
    c = C.case("threshold-7x9")
    n = oracle.ray_length(c.K[0], np.arange(9), np.arange(7))
    assert n[3, 4] == 1.0 and n[3, 5] > 1.0
    assert np.float64(c.depth_gt[0, 3, 4]) - 1.0 == np.float64(np.float32(c.delta)) < np.float64(c.depth_gt[1, 3, 4]) - 1.0
    assert c.depth_gt[1, 3, 4].view(np.int32) - c.depth_gt[0, 3, 4].view(np.int32) == 1  # one ulp above
    assert mask[0, 3, 4] == 1 and mask[1, 3, 4] == 0 and info[:, 2].tolist() == [2, 0]
    info, _, _ = C.expected("edge-5x6")
    assert info[:, 3].tolist() == [0, 1, 1, 1, 1, 4] and info[:, 0].tolist() == [1, 1, 1, 1, 1, 4]
    assert info[5, 4:8].tolist() == [2, 1, 7, 5]  # the window's corners in frame coordinates: the window lies at (2,1)
    assert C.expected("ring-5x6")[0][0, :4].tolist() == [18, 18, 18, 18]
    assert C.expected("corners-7x9")[0][0].tolist() == [4, 4, 4, 4, 0, 0, 8, 6, 0, 0, 8, 6]
    assert C.expected("corners-3x-7x9")[0][0].tolist() == [6, 4, 4, 2, -9, -7, 17, 13, 0, 0, 8, 6]
    info, mask, _ = C.expected("outside-4x6")
    assert (info[:, 0] > 0).all() and not info[:, 1:3].any() and (info[:, 8:] == -1).all() and not mask.any()
    info, _, _ = C.expected("far-origin")
    assert (info[[1, 2]] == -1).all() and info[0, 0] > 0 and info[3, 0] > 0 and info[3, 4] >= oracle.MAX_ORIGIN


@pytest.mark.parametrize("name", C.names())
def test_cases_keep_their_margin_and_their_shapes(name):
    c = C.case(name)
    info, mask, margin = C.expected(name)
    print(f"{name}: margin {margin:.3g}")
    assert margin >= C.MARGIN
    B = len(c.depth_gt)
    H, W = c.frame_hw
    assert B <= 6 and len(c.depth_test) <= 3 and c.depth_gt.shape[1:] == c.window_hw and c.depth_test.shape[1:] == c.frame_hw
    assert c.depth_gt.dtype == c.depth_test.dtype == c.K.dtype == np.float32 and c.K.shape == (B, 3, 3)
    assert info.shape == (B, 12) and mask.shape == c.depth_gt.shape and set(np.unique(mask)) <= {0, 1}
    live = info[:, 0] >= 0
    assert (info[live, 1] <= info[live, 0]).all() and (info[live, 2] <= info[live, 0]).all() and (info[live, 3] <= info[live, 0]).all()
    assert np.array_equal(mask.reshape(B, -1).sum(1)[live], info[live, 2])
    seen = info[:, 2] > 0  # a visible box lies in the frame and inside the silhouette's box
    assert (info[seen, 8] >= np.maximum(info[seen, 4], 0)).all() and (info[seen, 10] <= np.minimum(info[seen, 6], W - 1)).all()
    assert (info[seen, 9] >= np.maximum(info[seen, 5], 0)).all() and (info[seen, 11] <= np.minimum(info[seen, 7], H - 1)).all()


def test_case_list_covers_what_the_kernel_can_get_wrong():
    th, tw = C.tile_sizes()
    cs = C.cases()
    assert {c.frame_hw for c in cs} >= {(7, 9), (16, 20), (33, 37)}
    assert {c.window_hw for c in cs} >= {(1, 1), (1, 5), (6, 1), (5, 7), (5, 8), (5, 9), (21, 27), (48, 60)}
    x0 = {int(o[0]) % 4 for c in cs if c.origins is not None and c.frame_hw == (16, 20) for o in c.origins if o[0] >= 0}
    assert x0 == {0, 1, 2, 3}
    assert any((c.origins < 0).any() for c in cs if c.origins is not None)
    t = C.case("tiles")
    h, w = t.window_hw
    assert -(-h // th) >= 3 and h % th and -(-((w + 6) // 4) // (tw // 4)) >= 3 and w % tw
    both = np.concatenate([c.depth_test.ravel() for c in cs]), np.concatenate([c.depth_gt.ravel() for c in cs])
    for a in both:
        assert np.isnan(a).any() and np.isposinf(a).any() and (a < 0).any() and (a == 0).any()
    assert any(i[0] == 0 for c in cs for i in C.expected(c.name)[0]) and any(i[0] == -1 for c in cs for i in C.expected(c.name)[0])


def test_composition_of_the_cases_has_ties_and_skips():
    ties = 0
    for name in C.names():
        c, got = C.case(name), C.expected_compose(name)
        S = len(c.depth_test)
        assert got.depth.shape == (S, *c.frame_hw) and got.instance.shape == got.depth.shape and got.depth.dtype == np.float32
        assert np.array_equal(got.instance >= 0, got.depth > 0) and np.isfinite(got.depth).all()
        for b, s in enumerate(c.scene_index):
            assert got.info[b] == (-1 if oracle.refused(s, S, None if c.origins is None else c.origins[b]) else 0)
            assert got.info[b] == 0 or not (got.instance == b).any()
        if c.origins is None:  # full-frame rows: count the pixels at which two rows of a scene hold the winning z
            for s in range(S):
                rows = [b for b in range(len(c.depth_gt)) if c.scene_index[b] == s]
                ties += int(((np.stack([c.depth_gt[b] for b in rows]) == got.depth[s]) & (got.depth[s] > 0)).sum(0).__ge__(2).sum()) if rows else 0
    assert ties >= 20


def test_torch_statement_is_the_oracle():
    for name in ("full-16x20", "win-5x9", "larger-20x25", "bop3x-7x9", "values-7x9", "threshold-7x9", "outside-4x6"):
        c = C.case(name)
        keep = [b for b, s in enumerate(c.scene_index) if 0 <= s < len(c.depth_test)]
        info, mask, _ = C.expected(name)
        org = None if c.origins is None else torch.from_numpy(c.origins[keep])
        got_i, got_m = oracle.torch_statement(torch.from_numpy(c.depth_gt[keep]), torch.from_numpy(c.depth_test), torch.from_numpy(c.K[keep]), c.delta,
                                              torch.from_numpy(c.scene_index[keep]), org, c.center)
        assert got_i.dtype == torch.int32 and got_m.dtype == torch.uint8
        assert np.array_equal(got_i.numpy(), info[keep]), name
        assert np.array_equal(got_m.numpy(), mask[keep]), name


def test_visible_set_is_the_vsd_oracles_vis_gt():
    """Steps 1 and 2 of include/lc_amd_vsd.h are restated in include/lc_amd_gtinfo.h: on the VSD case list the two oracles, written
    apart, find the same visible ground-truth pixels, and the counts follow."""
    from tests import vsd_cases

    seen = 0
    for c in vsd_cases.CASES:
        b = vsd_cases.batch(c.name)
        for i, ref in enumerate(b.refs):
            if ref is None:
                continue
            r = oracle.record(b.depth_gt[i], b.depth_test[b.scene_index[i]], b.K[i], vsd_cases.DELTA, None, c.center)
            assert np.array_equal(r.mask_visib.astype(bool), ref.vis_gt), (c.name, i)
            assert r.info[2] == ref.vis_gt.sum() and r.info[0] == (b.depth_gt[i] > 0).sum()
            seen += int(ref.vis_gt.sum())
    assert seen > 1000
