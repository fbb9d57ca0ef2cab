"""The oracle of the zoom-in crops judged on the host: the closed-form identities that follow from the contract, the case list's
sensitivity to every planted mistake, and affine_from_box against an fp64 three-point solve.  No GPU needed."""
import numpy as np
import pytest

from lc_amd.crops import affine_from_box
from tests import crops_cases as cc
from tests import crops_oracle as co


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("interp", [co.LINEAR, co.NEAREST])
def test_identity_reproduces_the_source_bytes(C, interp):
    frame = cc.FRAMES[C][0]
    I = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)
    assert np.array_equal(co.warp_one(frame, I, (cc.H, cc.W), interp), frame)
    big = co.warp_one(frame, I, (cc.H + 3, cc.W + 2), interp)  # beyond the frame: border
    assert np.array_equal(big[:cc.H, :cc.W], frame) and not big[cc.H:].any() and not big[:, cc.W:].any()


@pytest.mark.parametrize("C", [3, 1])
def test_half_pixel_shift_is_the_rounded_mean_of_two_neighbours(C):
    frame = cc.FRAMES[C][1].astype(np.int64)
    Mx = np.array([[1, 0, -0.5], [0, 1, 0]], dtype=np.float32)  # crop x reads source x + 1/2
    got = co.warp_one(cc.FRAMES[C][1], Mx, (cc.H, cc.W - 1), co.LINEAR)
    assert np.array_equal(got, (frame[:, :-1] + frame[:, 1:] + 1) >> 1)
    My = np.array([[1, 0, 0], [0, 1, -0.5]], dtype=np.float32)
    got = co.warp_one(cc.FRAMES[C][1], My, (cc.H - 1, cc.W), co.LINEAR)
    assert np.array_equal(got, (frame[:-1] + frame[1:] + 1) >> 1)


def _changed_bytes(mistake):
    n = 0
    for C in (3, 1):
        for hw in cc.OUT_SIZES:
            for interp in (co.LINEAR, co.NEAREST):
                for names, M, ref, _ in cc.reference(C, hw, interp):
                    got, _ = co.warp(cc.FRAMES[C], M, hw, cc.FRAME_INDEX, interp, mistake=mistake)
                    n += int((got != ref).sum())
    return n


@pytest.mark.parametrize("mistake", co.MISTAKES)
def test_case_list_notices_the_planted_mistake(mistake):
    assert _changed_bytes(mistake) > 0, mistake


def test_case_list_holds_a_row_where_contraction_matters():
    """The seeded search found a matrix, it is in the list, and on that row alone one fma in the coordinate sums moves bytes."""
    assert "fma-row" in cc.NAMES
    M = dict(cc.CASES)["fma-row"]
    assert np.array_equal(M, cc.find_fma_row())  # the search is deterministic
    frame = cc.FRAMES[3][0]
    a, b = co.warp_one(frame, M, (16, 16), co.LINEAR), co.warp_one(frame, M, (16, 16), co.LINEAR, mistake="fma")
    assert (a != b).any() and a.any()
    Xa, _ = co.coordinates(M, (16, 16), co.LINEAR)
    Xb, _ = co.coordinates(M, (16, 16), co.LINEAR, mistake="fma")
    assert np.abs(Xa - Xb).max() == 1


def test_ties_row_parts_half_up_from_half_even():
    M = dict(cc.CASES)["ties"]
    Xa, _ = co.coordinates(M, (16, 16), co.LINEAR)
    Xb, _ = co.coordinates(M, (16, 16), co.LINEAR, mistake="rint_half_up")
    assert (Xa != Xb).any() and ((Xa >> 5) != (Xb >> 5)).any()


def test_bad_rows_are_all_border_and_flagged():
    M = np.stack([dict(cc.CASES)[n] for n in ("identity", "nan", "inf", "identity", "identity")])
    out, info = co.warp(cc.FRAMES[3], M, (16, 16), np.array([0, 0, 1, 2, -1]), co.LINEAR)
    assert info.tolist() == [0, -1, -1, -1, -1] and out[0].any() and not out[1:].any()
    out, info = co.warp(cc.FRAMES[3], M[:1], (16, 16), None, co.LINEAR)
    assert info.tolist() == [0]
    # D = 0 is NOT a bad row: the inverse is all zeros and every pixel reads the tap at (0, 0)
    out, info = co.warp(cc.FRAMES[3], dict(cc.CASES)["det-zero"][None], (16, 16), None, co.NEAREST)
    assert info.tolist() == [0] and (out[0] == cc.FRAMES[3][0][0, 0][:, None, None]).all()


def test_finish_follows_normalize_order_in_fp32():
    v = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, axis=1)
    q = co.finish(v)
    assert q.dtype == np.float32 and q[0, 0, 15, 15] == 1.0 and q[0, 0, 0, 1] == np.float32(1) / np.float32(255)
    n = co.finish(v, cc.NORMALIZE)
    mean, std = (np.asarray(a, dtype=np.float32) for a in cc.NORMALIZE)
    assert n[0, 2, 3, 4] == (np.float32(52) / np.float32(255) - mean[2]) / std[2]


def _reference_points(center, scale, rot, out_wh):
    """The three point pairs of dataset.py:88-103 in fp64 (no fp32 staging)."""
    center = np.asarray(center, dtype=np.float64)
    dst_w, dst_h = out_wh
    sn, cs = np.sin(rot), np.cos(rot)
    src_dir = np.array([0 * cs - (scale * -0.5) * sn, 0 * sn + (scale * -0.5) * cs])
    dst_dir = np.array([0, dst_w * -0.5])
    third = lambda a, b: b + np.array([-(a - b)[1], (a - b)[0]])  # noqa: E731
    src = np.stack([center, center + src_dir, third(center, center + src_dir)])
    d0 = np.array([dst_w * 0.5, dst_h * 0.5])
    dst = np.stack([d0, d0 + dst_dir, third(d0, d0 + dst_dir)])
    return src, dst


@pytest.mark.parametrize("rot", [0.0, 0.3, 2.0, -4.1])
@pytest.mark.parametrize("out_wh", [(16, 16), (40, 24), (256, 256)])
def test_affine_from_box_is_the_three_point_solve(rot, out_wh):
    """Both sides carry about 1e-15 of relative error before their single rounding to fp32, so they may land on neighbouring fp32 values
    and no further apart: one fp32 ulp.  An entry that is zero but for the solver's rounding noise (rot = 0: the closed form gives
    exactly 0 there, the solver about 1e-17) is held to 1e-12 absolute."""
    for center, scale in (((26.5, 18.25), 60.0), ((311.7, 204.9), 187.35), ((5.0, 400.0), 33.0)):
        src, dst = _reference_points(center, scale, rot, out_wh)
        M, Mi = affine_from_box(center, scale, rot, out_wh)
        assert M.dtype == Mi.dtype == np.float32 and M.shape == Mi.shape == (2, 3)
        for got, want in ((M, co.three_point_solve(src, dst)), (Mi, co.three_point_solve(dst, src))):
            want32 = want.astype(np.float32)
            ulp = np.spacing(np.maximum(np.abs(want32), np.float32(1e-30)))
            zero = np.abs(want) < 1e-12  # entries that are zero but for the solver's rounding (rot = 0)
            ulp = np.where(zero, 1e-12, ulp)
            assert (np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= ulp).all(), (rot, out_wh, center, got, want32)


def test_wide_sizes_reach_the_layouts_the_small_sizes_stop_short_of():
    """The restated launch geometry: the old sizes end at 32 threads along x (lg_tx = 5, eight rows per pass), the wide ones reach 64,
    128 and 256 threads along x, a second trip of the quad loop, and a second band that holds one row."""
    assert max(cc.warp_grid(h, w)[2] for h, w in cc.OUT_SIZES) <= 5
    assert [cc.warp_grid(h, w) for h, w in ((16, 64), (17, 65), (17, 128))] == [(16, 1, 4), (16, 2, 5), (16, 2, 5)]
    grids = {hw: cc.warp_grid(*hw) for hw in cc.WIDE_SIZES}
    assert {g[2] for g in grids.values()} == {6, 7, 8}
    assert [grids[(17, w)][2] for w in (129, 256, 257, 513, 1024, 1025, 1028)] == [6, 6, 7, 8, 8, 8, 8] and grids[(256, 256)] == (16, 16, 6)
    assert all(g[:2] == (16, 2) for hw, g in grids.items() if hw[0] == 17)
    quads = sorted((w + 3) // 4 for _, w in cc.WIDE_SIZES)
    assert quads[-3:] == [256, 257, 257]  # one full trip, and two sizes that need a second
    assert {w % 4 for _, w in cc.WIDE_SIZES if (w + 3) // 4 > 256} == {0, 1}  # a whole last quad and a partial one
    for h, w in cc.OUT_SIZES + cc.WIDE_SIZES:
        assert cc.rows_walked(h, w).all()
    assert cc.rows_walked(17, 256, stride=8).tolist() == [True] * 4 + [False] * 4 + [True] * 4 + [False] * 4 + [True]
    assert cc.rows_walked(17, 513, stride=8).sum() == 3 and cc.rows_walked(24, 40, stride=8).all()  # TY >= 8: the mistake cannot show


@pytest.mark.parametrize("interp", [co.LINEAR, co.NEAREST])
@pytest.mark.parametrize("out_hw", cc.WIDE_SIZES)
@pytest.mark.parametrize("C", [3, 1])
def test_wide_cases_cross_the_frames_edges_and_notice_a_wrong_layout(C, out_hw, interp):
    """Every row of every wide case reads pixels inside and outside its frame, and its bytes part from the oracle's under each planted
    mistake that its layout can show: a row loop that steps by 8 (every wide size has fewer than 8 rows per pass), and x terms formed
    from x mod 1024 (which is x itself up to w = 1024: only the sizes with a second trip can tell, and they must)."""
    M, ref, info = cc.wide_reference(C, out_hw, interp)
    assert not info.any()
    for b in range(2):
        X, Y = co.coordinates(M[b], out_hw, co.NEAREST)
        inside = ((X >> 10) >= 0) & ((X >> 10) < cc.W) & ((Y >> 10) >= 0) & ((Y >> 10) < cc.H)
        assert inside.any() and not inside.all()
        sides = [bool(s.any()) for s in ((X >> 10) < 0, (X >> 10) >= cc.W, (Y >> 10) < 0, (Y >> 10) >= cc.H)]  # left, right, top, bottom
        assert sum(sides) >= 2, sides
        assert ref[b].any()
        assert (cc.wide_planted(C, out_hw, interp, "row_stride_8")[b] != ref[b]).any()
        moved = (cc.wide_planted(C, out_hw, interp, "x_mod_1024")[b] != ref[b])
        assert moved.any() == (out_hw[1] > 1024) and not moved[..., :1024].any()
