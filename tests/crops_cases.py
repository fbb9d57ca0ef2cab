"""The case list of the zoom-in crops (tests/test_crops_oracle.py on the host, tests/test_gpu_crops.py on the device): two small unsmooth
frames, every forward matrix that takes another path through the contract, three output sizes and one batch layout.  Everything is
generated from fixed seeds."""
import numpy as np

from lc_amd.crops import affine_from_box
from tests import crops_oracle as co

H, W = 37, 53
SEED = 20261018


def make_frames(C, n=2, hw=(H, W), seed=SEED):
    """(n,H,W,C) uint8: (37 x + 101 y + 59 c) mod 251 XOR a seeded byte -- nothing smooth about it, so a wrong tap or weight shows."""
    h, w = hw
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(C), indexing="ij")
    base = ((37 * x + 101 * y + 59 * c) % 251).astype(np.uint8)
    rng = np.random.default_rng(seed + C)
    return np.stack([base ^ rng.integers(0, 256, size=base.shape, dtype=np.uint8) for _ in range(n)])


FRAMES = {3: make_frames(3), 1: make_frames(1)}
OUT_SIZES = ((16, 16), (24, 40), (10, 6))  # (h, w): w = 6 leaves the last thread of a row with two of its four pixels
FRAME_INDEX = np.array([0, 1, 1, 0, 1], dtype=np.int32)  # B = 5
B = len(FRAME_INDEX)
NORMALIZE = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _m(a, b, tx, c, d, ty):
    return np.array([[a, b, tx], [c, d, ty]], dtype=np.float32)


def _about_centre(k, deg):
    """Scale k and rotation about the frame's centre, the centre going to the centre of a 16 x 16 crop."""
    t = np.deg2rad(deg)
    L = k * np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]])
    tr = np.array([8.0, 8.0]) - L @ np.array([W / 2, H / 2])
    return np.concatenate((L, tr[:, None]), axis=1).astype(np.float32)


def find_fma_row(seed=SEED, tries=4000):
    """A matrix for which contracting m01 * y + b1 into one fma changes bytes of a 16 x 16 linear crop of frame 0, found by a seeded
    search: 1 / det is inexact (det in {3, 5, 6, 7}), so m01 y carries a rounding error for some row y0, and the translation is
    chosen so that the separately rounded sum lands on a half-integer of the 1/1024 px grid whose neighbour lies in the next 1/32 px
    weight.  The candidates are judged by the oracle itself; None when none of them qualifies."""
    rng = np.random.default_rng(seed)
    frame = FRAMES[3][0]
    for _ in range(tries):
        a, c = float(rng.choice([3, 5, 6, 7])), float(rng.choice([-2, -1, 1, 2]))
        y0, j = int(rng.integers(1, 16)), int(rng.integers(64, 900))
        m01 = co.inverse(_m(a, c, 0, 0, 1, 0))[1]
        b1 = (32 * j + 15 + 0.5) / 1024.0 - m01 * y0
        M = _m(a, c, -a * b1, 0, 1, 0)
        if not np.array_equal(co.warp_one(frame, M, (16, 16), co.LINEAR), co.warp_one(frame, M, (16, 16), co.LINEAR, mistake="fma")):
            return M
    return None


def _cases():
    nan, inf = float("nan"), float("inf")
    box = dict(center=(26.5, 18.25), scale=40 * 1.5)  # a 40 px detection with dzi_pad_scale 1.5
    cases = [
        ("identity", _m(1, 0, 0, 0, 1, 0)),
        ("shift-int", _m(1, 0, -7, 0, 1, -5)),
        ("shift-half", _m(1, 0, -0.5, 0, 1, 0)),
        ("down-3.7", _about_centre(1 / 3.7, 0)),
        ("up-0.31", _about_centre(1 / 0.31, 0)),
        ("rot-33", _about_centre(1.0, 33)),
        ("border-left", _m(1, 0, 6, 0, 1, -9)),
        ("border-right", _m(1, 0, -(W - 9), 0, 1, -9)),
        ("border-top", _m(1, 0, -20, 0, 1, 5)),
        ("border-bottom", _m(1, 0, -20, 0, 1, -(H - 7))),
        ("corner", _m(0.8, 0.1, -(W - 12) * 0.8, -0.1, 0.8, -(H - 10) * 0.8)),
        ("outside", _m(1, 0, 500, 0, 1, 300)),
        ("det-zero", _m(1, 2, 0, 2, 4, 0)),
        ("nan", _m(1, 0, nan, 0, 1, 0)),
        ("inf", _m(1, 0, 0, inf, 1, 0)),
        ("far-1e7", _m(1, 0, 1e7, 0, 1, -1e7)),
        ("box-16", affine_from_box(box["center"], box["scale"], 0.0, (16, 16))[0]),
        ("box-40x24", affine_from_box(box["center"], box["scale"], 0.0, (40, 24))[0]),
        ("box-rot", affine_from_box(box["center"], box["scale"], 0.3, (16, 16))[0]),
        # every row's y term is a half-integer of the 1/1024 px grid (m01 = -1/1024, b1 = -20.5/1024) and the x term 1025 x is odd for
        # odd x: round-half-up and round-half-even then part, and for some (x, y) the parting crosses a 1/32 px weight
        ("ties", _m(1, 1 / 1024, 0, 1, 1025 / 1024, -20.5)),
    ]
    fma = find_fma_row()
    if fma is None:  # the row that pins the contraction trap must not go missing without a word
        raise RuntimeError("tests/crops_cases.py: the seeded search found no matrix on which fma contraction changes bytes")
    cases.append(("fma-row", fma))
    return cases


CASES = _cases()
NAMES = [n for n, _ in CASES]


def batches():
    """The case list cut into batches of B = 5 rows (the last one filled up from the front): [(names, M (5,2,3))]."""
    out = []
    for i in range(0, len(CASES), B):
        rows = [CASES[(i + k) % len(CASES)] for k in range(B)]
        out.append(([n for n, _ in rows], np.stack([m for _, m in rows])))
    return out


_REF = {}


def reference(C, out_hw, interp):
    """[(names, M, out (5,C,h,w) uint8, info (5) int32)] of every batch from the oracle, computed once per (C, size, interp)."""
    key = (C, tuple(out_hw), interp)
    if key not in _REF:
        res = []
        for names, M in batches():
            out, info = co.warp(FRAMES[C], M, out_hw, FRAME_INDEX, interp)
            out.setflags(write=False)
            info.setflags(write=False)
            res.append((names, M, out, info))
        _REF[key] = res
    return _REF[key]


# ---- the loader fixture (tests/golden/gen_golden_crops.py writes crops_item.npz from it, tests/test_crops_host.py rebuilds it) ----
NET_INPUT_WH, NET_OUTPUT_WH = (24, 16), (12, 8)  # (w, h), not square: a swapped pair shows
DZI_PAD_SCALE = 1.5
EXACT_ITEMS = (0, 1)  # items of the fixture on which `test_item` equals the reference's blob bit for bit, matrices included


def affine_tolerance(center, scale, out_wh):
    """Entry-wise bound (2,3) on |closed form - reference| for a rot = 0 box inside the 37 x 53 frame, from the reference's fp32 staging
    (dataset.py:95-103).  Centre and scale are rounded to fp32 on both sides; the reference then rounds its second point and forms the
    third in fp32, each coordinate (below 64 in magnitude) off by at most e = 2^-19 px, half an fp32 ulp there.  The solve maps the
    direction p1 - p0 of length s/2 to a fixed one, so the linear part moves by at most k * 2e / (s/2 - 2e) per entry (k = dst_w / s),
    doubled for the third point, which inherits the second's error and adds its own; the translation t = q0 - L p0 moves by that times
    (|cx| + |cy|).  One fp32 ulp is added for the two final roundings."""
    e, k, half = 2.0 ** -19, out_wh[0] / scale, scale / 2
    dl = 2 * k * 2 * e / (half - 2 * e)
    dt = dl * (abs(center[0]) + abs(center[1]))
    ulp_l, ulp_t = np.spacing(np.float32(k)), np.spacing(np.float32(max(out_wh) + k * (abs(center[0]) + abs(center[1]))))
    return np.array([[dl + ulp_l, dl + ulp_l, dt + ulp_t]] * 2)


def loader_fixture():
    """What a reference `BOP_Dataset` object holds for three instances of one 37 x 53 frame, two of them with `bbox_det`: a dict of the
    attributes the non-training `_get_single_item` reads.  The first two are the EXACT items (`EXACT_ITEMS`): box coordinates are exact in fp32 (BOP's boxes are whole pixels; the
    detection here lies on quarter pixels), so the reference's fp32 staging of its three points loses nothing; cam_K is float64 with
    short mantissas, so `affine33 @ cam_K` is exact however the matrix product is evaluated.  The boxes are also ones for which the
    fp64 three-point solve returns exact zeros off the diagonal: a linear solver may leave rounding noise of order 1e-17 there, which the
    closed form of `affine_from_box` does not reproduce (it moves no coordinate of the warp, and out_K by parts in 1e17).  The third is
    a detection as a detector delivers it, exact in nothing: there the reference's fp32 staging of its points shows, and
    `affine_tolerance` bounds what it can do."""
    import types

    cam_K = np.array([[572.5, 0.0, 26.25], [0.0, 573.75, 18.5], [0.0, 0.0, 1.0]], dtype=np.float64)
    im_info = dict(rgb="frame_000.png", cam_K=cam_K, im_id=7, scene_id=2, split="test")
    R = np.eye(3, dtype=np.float32)
    t = np.array([[10.0], [-20.0], [700.0]], dtype=np.float32)
    insts = [dict(obj_id=5, cam_R_m2c=R, cam_t_m2c=t, mask_visib=None, bbox_visib=np.array([8, 4, 30, 24], dtype=np.int64)),
             dict(obj_id=9, cam_R_m2c=R, cam_t_m2c=t, mask_visib=None, bbox_visib=np.array([5, 3, 41, 30], dtype=np.int64),
                  bbox_det=np.array([6.25, 2.5, 32.0, 22.75], dtype=np.float64)),
             dict(obj_id=9, cam_R_m2c=R, cam_t_m2c=t, mask_visib=None, bbox_visib=np.array([5, 3, 41, 30], dtype=np.int64),
                  bbox_det=np.array([6.3, 2.7, 33.1, 22.9], dtype=np.float64))]
    rng = np.random.default_rng(SEED + 9)
    model_info = {oid: dict(noc_scale_xfd=rng.random(3).astype(np.float32), noc_scale_ori=rng.random(3).astype(np.float32),
                            xform=rng.random((4, 4)).astype(np.float32), bbox_3d_ori=rng.random((8, 3)).astype(np.float32),
                            diameter=np.float32(100 + oid)) for oid in (5, 9)}
    fps = {oid: rng.random((8, 3)).astype(np.float32) for oid in (5, 9)}
    return dict(cfg=types.SimpleNamespace(dzi_pad_scale=DZI_PAD_SCALE, rotate_prob=0.5, switch_bg_prob=0.5, pixel_aug_prob=0.5),
                cfg_global=types.SimpleNamespace(), np_annots=[(im_info, inst) for inst in insts], model_info=model_info, sym_obj_ids=[],
                fps=fps, sparse_cnt=3, transform_model=True, training=False, debug=False, valid_pix_cnt_th=100, mask_interp=1,
                net_input_wh=NET_INPUT_WH, net_output_wh=NET_OUTPUT_WH)


# ---- wide crops: the warp launch's layouts beyond 32 threads along x (tests/test_crops_oracle.py, tests/test_gpu_crops.py) ----
# h = 17 is two bands of 16 rows, the second with one row.  w = 129 and 256 lay the 256 threads out as 64 quads x 4 rows (256: whole
# quads, vector stores), 257 as 128 x 2, 513 as 256 x 1; 1024 is one full trip of the quad loop, 1025 a second trip with a partial quad,
# 1028 a second trip with a whole one.  256 x 256 is the workload's size.
WIDE_SIZES = ((17, 129), (17, 256), (17, 257), (17, 513), (17, 1024), (17, 1025), (17, 1028), (256, 256))
WIDE_FRAME_INDEX = np.array([1, 0], dtype=np.int32)
WIDE_MISTAKES = ("x_mod_1024", "row_stride_8")
THREADS, MIN_BAND = 256, 16


def warp_grid(h, w, threads=THREADS, min_band=MIN_BAND):
    """(band, nbands, lg_tx) of the warp launch, as lc_amd/csrc/shared/lc_warp_grid.h lays it out: 2^lg_tx threads along x, each owning
    four pixels, and threads >> lg_tx rows per pass."""
    quads, lg_tx = (w + 3) // 4, 0
    while (1 << lg_tx) < quads and (1 << lg_tx) < threads:
        lg_tx += 1
    band = max(threads >> lg_tx, min_band)
    return band, (h + band - 1) // band, lg_tx


def rows_walked(h, w, stride=None):
    """(h,) bool: the crop rows that the launch's row loop `for (y = band * grid.band + ty; y < y_end; y += TY)` reaches when it steps
    by `stride` (None: by TY, and then every row is reached)."""
    band, nbands, lg_tx = warp_grid(h, w)
    TY = THREADS >> lg_tx
    seen = np.zeros(h, dtype=bool)
    for b in range(nbands):
        for ty in range(TY):
            seen[b * band + ty:min(h, (b + 1) * band):stride or TY] = True
    return seen


def stress_matrix(center, frame_hw, out_hw, rot, stretch, skew, cover=1.25, anchor=0.9):
    """Forward matrix of the suite's `stress` kind (rotation, x stretched, x sheared by y), zoomed so that the crop's longer side spans
    `cover` frame diagonals.  Frame point `center` goes to the crop point `anchor` of the way along x, half way down: the crop's last
    columns -- the ones a second trip of the quad loop forms -- read inside the frame, and its first ones far outside it."""
    c, s = np.cos(rot), np.sin(rot)
    zoom = max(out_hw) / (cover * np.hypot(*frame_hw))
    A = np.array([[c, s], [-s, c]]) @ np.array([[stretch, skew], [0.0, 1.0]]) * zoom
    t = np.array([out_hw[1] * anchor, out_hw[0] * 0.5]) - A @ np.asarray(center, dtype=np.float64)
    return np.concatenate((A, t[:, None]), axis=1).astype(np.float32)


STRESS_KINDS = ((np.deg2rad(25.0), 1.31, 0.23), (np.deg2rad(-50.0), 0.77, -0.4))  # (rot, stretch, skew)


def wide_matrices(out_hw):
    """(2,2,3): one matrix of each stress kind; the crop runs into the frame across one of its corners and ends near its centre."""
    return np.stack([stress_matrix((W / 2, H / 2), (H, W), out_hw, *kind) for kind in STRESS_KINDS])


class planted_coordinates:
    """Within the block crops_oracle.coordinates carries a mistake of the launch geometry: "x_mod_1024" forms the x terms of column x
    from x mod 1024 (a thread that keeps its first trip's quad terms on its second trip)."""

    def __init__(self, mistake):
        self.mistake = mistake

    def __enter__(self):
        real = self.real = co.coordinates
        if self.mistake == "x_mod_1024":
            def wrong(M, out_hw, interp, mistake=None):
                X, Y = real(M, out_hw, interp, mistake)  # X[y, x] = row term(y) + x term(x) + delta: column x mod 1024 holds the wrong sum
                cols = np.arange(out_hw[1]) % 1024
                return X[:, cols], Y[:, cols]
            co.coordinates = wrong

    def __exit__(self, *exc):
        co.coordinates = self.real


def wide_planted(C, out_hw, interp, mistake):
    """The oracle's (2,C,h,w) crops of the wide batch under one planted mistake of WIDE_MISTAKES.  "row_stride_8" steps the row loop by 8
    whatever the layout: the rows it never reaches keep what the buffer held, here 0."""
    with planted_coordinates(mistake):
        out, _ = co.warp(FRAMES[C], wide_matrices(out_hw), out_hw, WIDE_FRAME_INDEX, interp)
    if mistake == "row_stride_8":
        out[:, :, ~rows_walked(*out_hw, stride=8)] = 0
    return out


def wide_reference(C, out_hw, interp):
    """(M (2,2,3), out (2,C,h,w) uint8, info (2) int32) of the wide batch from the oracle, computed once per (C, size, interp)."""
    key = ("wide", C, tuple(out_hw), interp)
    if key not in _REF:
        M = wide_matrices(out_hw)
        out, info = co.warp(FRAMES[C], M, out_hw, WIDE_FRAME_INDEX, interp)
        out.setflags(write=False)
        info.setflags(write=False)
        _REF[key] = (M, out, info)
    return _REF[key]
