"""The crop geometry's contract without a GPU (lc_amd/geometry.py, include/lc_amd.h): `zoom_geometry_host` against the host functions it
restates (`augment.draw_zoom`, `crops.affine_from_box`, `augment.background_matrices`), the polynomial (c, s) against numpy over every
draw, and the committed edge draws."""
import dataclasses
import math

import numpy as np
import pytest

from lc_amd import augment, crops, geometry
from tests import geometry_cases as gc

CFG = augment.AugmentConfig(rotate_prob=0.5)
IM_HW, IN_WH, OUT_WH = (480, 640), (256, 192), (128, 96)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_centre_scale_and_rotation_are_draw_zooms_bit_for_bit():
    for seed in (0, 3, 2 ** 32 + 9, 2 ** 64 - 1):
        ids, box, K = gc.batch(257, seed)
        g = geometry.zoom_geometry_host(CFG, seed, ids, box, IM_HW, K, IN_WH, OUT_WH)
        centre, scale, rot = augment.draw_zoom(CFG, seed, ids, box, IM_HW)
        assert (g.info == 0).all()
        assert _same(g.centre, centre) and _same(g.scale, scale) and _same(g.rot, rot)
        assert (scale == 640.0).sum() >= 257 // 5  # the clamp of max(im_h, im_w) is met
        assert (rot == 0).any() and (rot != 0).any()


def test_background_matrices_are_the_existing_ones_bit_for_bit():
    ids = np.arange(-5, 60)
    hw = np.stack((np.arange(65) * 7 + 40, np.arange(65)[::-1] * 11 + 30), axis=1)
    for seed in (1, 2 ** 40 + 1):
        assert _same(geometry.background_geometry_host(seed, ids, hw, (64, 48)), augment.background_matrices(seed, ids, hw, (64, 48)))


@pytest.mark.parametrize("train", [True, False])
def test_unrotated_matrices_equal_affine_from_box_bit_for_bit(train):
    cfg = dataclasses.replace(CFG, rotate_prob=0.0)
    ids, box, K = gc.batch(65, 4)
    g = geometry.zoom_geometry_host(cfg, 11, ids, box, IM_HW, K, IN_WH, OUT_WH, train=train)
    if train:
        centre, scale, _ = augment.draw_zoom(cfg, 11, ids, box, IM_HW)
    else:
        b = box.astype(np.float64)
        centre = np.stack((0.5 * (b[:, 0] + b[:, 2]), 0.5 * (b[:, 1] + b[:, 3])), axis=1)
        scale = np.array([max(x2 - x1, y2 - y1, 1) * cfg.dzi_pad_scale for x1, y1, x2, y2 in b])
        assert _same(g.centre, centre) and _same(g.scale, scale)
    assert (g.rot == 0).all() and (g.cs == [1.0, 0.0]).all()
    for b in range(len(ids)):
        assert _same(g.in_affine[b], crops.affine_from_box(centre[b], scale[b], 0.0, IN_WH)[0])
        assert _same(g.out_affine[b], crops.affine_from_box(centre[b], scale[b], 0.0, OUT_WH)[0])
    assert _same(g.out_pix_scale, (scale / OUT_WH[0]).astype(np.float32))


def test_rotated_matrices_lie_within_one_ulp_of_affine_from_box():
    """The two fp64 values differ by the polynomial's distance from libm's (c, s), a few 2^-52 of terms of up to 1e5: one float32 ulp
    of the entry, or 1e-9 absolute where the entry is tiny, whichever is larger."""
    cfg = dataclasses.replace(CFG, rotate_prob=1.0)
    ids, box, K = gc.batch(257, 6)
    g = geometry.zoom_geometry_host(cfg, 5, ids, box, IM_HW, K, IN_WH, OUT_WH)
    centre, scale, rot = augment.draw_zoom(cfg, 5, ids, box, IM_HW)
    worst = 0.0
    for b in range(len(ids)):
        for got, wh in ((g.in_affine[b], IN_WH), (g.out_affine[b], OUT_WH)):
            ref = crops.affine_from_box(centre[b], scale[b], rot[b], wh)[0]
            tol = np.maximum(np.spacing(np.abs(ref)), np.float32(1e-9))
            d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            worst = max(worst, float((d / tol).max()))
            assert (d <= tol).all(), (b, got, ref)
    print(f"largest distance from affine_from_box: {worst:.3f} of the tolerance")


def test_out_K_is_the_stated_fp64_product_rounded_once():
    ids, box, K = gc.batch(64, 2)
    g = geometry.zoom_geometry_host(CFG, 8, ids, box, IM_HW, K, IN_WH, OUT_WH)
    A, K64 = g.out_affine.astype(np.float64), K.astype(np.float64)
    for b in range(64):
        for i in range(2):
            for j in range(3):
                want = np.float32((A[b, i, 0] * K64[b, 0, j] + A[b, i, 1] * K64[b, 1, j]) + A[b, i, 2] * K64[b, 2, j])
                assert g.out_K[b, i, j] == want
        assert _same(g.out_K[b, 2], K[b, 2])
    # and it is the reference's `affine33 @ cam_K` up to the fp32 product's own rounding
    a33 = np.tile(np.eye(3, dtype=np.float32), (64, 1, 1))
    a33[:, :2] = g.out_affine
    assert np.allclose(g.out_K, a33 @ K, rtol=1e-5, atol=1e-3)


def test_step_id_is_the_sixth_zoom_key():
    ids, box, K = gc.batch(63, 3)
    for seed in (0, 2 ** 33 + 1):
        g = geometry.zoom_geometry_host(CFG, seed, ids, box, IM_HW, K, IN_WH, OUT_WH)
        assert g.step_id.dtype == np.int32 and (g.step_id >= 0).all()
        assert (g.step_id == (augment.key(seed, ids, augment.OP_ZOOM, 5) & np.uint64(0x7FFFFFFF)).astype(np.int64)).all()
    other = geometry.zoom_geometry_host(CFG, 1, ids, box, IM_HW, K, IN_WH, OUT_WH).step_id
    assert (other != g.step_id).mean() > 0.9  # it changes with the seed word


def test_bad_rows_are_refused_as_nan_and_leave_their_neighbours_alone():
    ids, box, K = gc.batch(9, 5)
    good = geometry.zoom_geometry_host(CFG, 2, ids, box, IM_HW, K, IN_WH, OUT_WH)
    box2, K2 = box.copy(), K.copy()
    box2[1, 2:] = box2[1, :2]       # a zero-size box: scale 0
    box2[3, 0] = np.nan
    box2[5, 3] = np.inf
    K2[7, 1, 1] = np.nan
    g = geometry.zoom_geometry_host(CFG, 2, ids, box2, IM_HW, K2, IN_WH, OUT_WH)
    bad = np.array([1, 3, 5, 7])
    assert (g.info[bad] == -1).all() and (np.delete(g.info, bad) == 0).all()
    for name in ("in_affine", "out_affine", "out_K", "out_pix_scale", "centre", "scale"):
        a = getattr(g, name)
        assert np.isnan(a[bad]).all(), name
        assert _same(np.delete(a, bad, axis=0), np.delete(getattr(good, name), bad, axis=0)), name
    assert _same(g.step_id, good.step_id) and _same(g.rot, good.rot) and _same(g.cs, good.cs)


def test_a_row_depends_on_its_own_inputs_only():
    ids, box, K = gc.batch(65, 7)
    whole = geometry.zoom_geometry_host(CFG, 21, ids, box, IM_HW, K, IN_WH, OUT_WH)
    pick = np.array([64, 3, 3, 17])
    part = geometry.zoom_geometry_host(CFG, 21, ids[pick], box[pick], IM_HW, K[pick], IN_WH, OUT_WH)
    for a, b in zip(whole, part):
        assert _same(a[pick], b)


# ---- the polynomial ---------------------------------------------------------------------------------------------------------------
def test_polynomial_cos_sin_over_all_draws():
    """|c - cos(2 pi f)|, |s - sin(2 pi f)| <= 2^-50 over all 2^24 draws: the bound covers the argument's single rounding plus about nine
    Horner roundings of partials <= 1, with margin; a value above it means a wrong coefficient."""
    k = np.arange(1 << 24, dtype=np.float64)
    u4 = k / float(1 << 24)
    c, s = geometry.cos_sin_turns(u4)
    tau = 2.0 * u4
    f = tau - np.floor(tau)
    ang = 2.0 * math.pi * f
    dc, ds = np.abs(c - np.cos(ang)).max(), np.abs(s - np.sin(ang)).max()
    print(f"largest |c - cos| = {dc:.3e} = 2^{math.log2(dc):.2f}, largest |s - sin| = {ds:.3e} = 2^{math.log2(ds):.2f}")
    assert dc <= 2.0 ** -50 and ds <= 2.0 ** -50
    assert np.abs(c * c + s * s - 1.0).max() <= 2.0 ** -50
    # the coefficients are the Taylor series'
    assert all(v == (-1) ** ((n - 1) // 2) / math.factorial(n) for v, n in zip(geometry.SIN_C, range(3, 18, 2)))
    assert all(v == (-1) ** (n // 2) / math.factorial(n) for v, n in zip(geometry.COS_C, range(2, 17, 2)))
    assert geometry.PI_4 == math.pi / 4


def test_quarter_turns_are_exact():
    """g = 0 at the 8 draws u4 = j / 8: rot is a whole number of quarter turns and (c, s) are exactly 0 or +-1."""
    u4 = np.arange(8) / 8.0
    c, s = geometry.cos_sin_turns(u4)
    assert c.tolist() == [1, 0, -1, 0, 1, 0, -1, 0] and s.tolist() == [0, 1, 0, -1, 0, 1, 0, -1]
    # the other 8 octant edges reach a = fl(pi / 4) from above: both are the polynomial's values there, within 2^-52 of sqrt(1/2)
    c, s = geometry.cos_sin_turns((2 * np.arange(8) + 1) / 16.0)
    assert np.abs(np.abs(c) - math.sqrt(0.5)).max() <= 2.0 ** -52 and np.abs(np.abs(s) - math.sqrt(0.5)).max() <= 2.0 ** -52
    assert (np.sign(c) == [1, -1, -1, 1] * 2).all() and (np.sign(s) == [1, 1, -1, -1] * 2).all()


def test_committed_edge_draws_land_on_their_edges():
    assert sorted(k for k, _, _ in gc.EDGE_DRAWS) == [j << 20 for j in range(16)] + [(1 << 24) - 1]
    assert any(s >= 2 ** 32 for s in gc.EDGE_SEEDS) and any(s >= 2 ** 63 for s in gc.EDGE_SEEDS)
    for k, seed, sid in gc.EDGE_DRAWS:
        assert -2 ** 31 <= sid < 2 ** 31
        assert augment.u(seed, [sid], augment.OP_ZOOM, 4)[0] == k / float(1 << 24), (k, seed, sid)
    for seed in gc.EDGE_SEEDS:
        assert len(gc.edge_ids(seed))
