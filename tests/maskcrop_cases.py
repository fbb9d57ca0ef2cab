"""The case list of the training mask crops, shared by tests/test_maskcrop_oracle.py (numpy) and tests/test_gpu_maskcrop.py (device):
small windows of 5 x 7 up to 48 x 40, matrices from the identity to the stretched and skewed kind of the suite's `stress` camera, origins
on both sides of zero, crops that straddle each window edge or miss the window.  The crop sizes follow the warp launch's shape: a
workgroup covers a band of 16 crop rows (more where the crop is narrower than 64), its 256 threads laid out as 16 x 16 quads of four
pixels at w = 64, so 16 x 64 is one pass of one workgroup exactly; a row more starts a second band, a column more a second quad layout
(32 x 8) with a partial quad.  Two 16 x 16 rows hold the device to the coordinate traps of tests/crops_cases.py: its "ties" matrix, and a
matrix on which contracting m01 * y + b1 into one fma changes the mask crop."""
import math
from typing import NamedTuple

import numpy as np

from tests import crops_oracle, maskcrop_oracle

TILE_H, TILE_W = 16, 64
EYE = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))


class Warp(NamedTuple):
    name: str
    mask_hw: tuple
    seed: int
    origin: tuple  # (x0, y0)
    M: tuple       # (2,3), frame -> crop
    out_hw: tuple


def mask(hw, seed):
    """A (Hm,Wm) uint8 0/1 window; seed < 0: all set (the window's edges alone decide)."""
    if seed < 0:
        return np.ones(hw, dtype=np.uint8)
    return (np.random.default_rng(seed).random(hw) < 0.6).astype(np.uint8)


def noc_with(valid, hw, seed):
    """A (h,w) uint8 mask with exactly `valid` set pixels, anywhere."""
    m = np.zeros(hw[0] * hw[1], dtype=np.uint8)
    m[np.random.default_rng(seed).permutation(m.size)[:valid]] = 1
    return m.reshape(hw)


def embed(window, origin):
    """(frame, (dx, dy)): a frame that holds the window at its origin, so that frame pixel (X + dx, Y + dy) is the contract's frame pixel
    (X, Y).  A non-negative origin gives the frame itself (dx = dy = 0); else the window serves, shifted."""
    x0, y0 = int(origin[0]), int(origin[1])
    if x0 >= 0 and y0 >= 0:
        frame = np.zeros((y0 + window.shape[0], x0 + window.shape[1]), dtype=np.uint8)
        frame[y0:, x0:] = window
        return frame, (0, 0)
    return window, (-x0, -y0)


def affine(center, zoom, out_hw, rot=0.0, stretch=1.0, skew=0.0, shift=(0.0, 0.0)):
    """Forward matrix that takes frame point `center` to the crop's centre (+ shift): rotation by rot, zoom (crop pixels per frame pixel),
    x stretched by `stretch`, x sheared by `skew` of y."""
    c, s = math.cos(rot), math.sin(rot)
    A = np.array([[c, s], [-s, c]]) @ np.array([[stretch, skew], [0.0, 1.0]]) * zoom
    t = np.array([out_hw[1] * 0.5 + shift[0], out_hw[0] * 0.5 + shift[1]]) - A @ np.asarray(center, dtype=np.float64)
    return tuple(map(tuple, np.concatenate((A, t[:, None]), 1).astype(np.float32).tolist()))


def planted(window, origin, M, out_hw, vis_interp, mistake):
    """maskcrop_oracle.warp_row with its coordinates taken from crops_oracle.coordinates(..., mistake=mistake)."""
    real = crops_oracle.coordinates
    crops_oracle.coordinates = lambda M_, out_hw_, interp, mistake_=None: real(M_, out_hw_, interp, mistake)
    try:
        return maskcrop_oracle.warp_row(window, origin, M, out_hw, vis_interp)
    finally:
        crops_oracle.coordinates = real


def moved_by(window, origin, M, out_hw, mistake):
    """The number of pixels of (msk_vis linear, msk_noc) that the planted mistake changes."""
    good, bad = maskcrop_oracle.warp_row(window, origin, M, out_hw), planted(window, origin, M, out_hw, maskcrop_oracle.LINEAR, mistake)
    return int((good[0] != bad[0]).sum()), int((good[1] != bad[1]).sum())


def find_fma_row(window, origin, out_hw=(16, 16), tries=4000):
    """A matrix on which contracting m01 * y + b1 into one fma changes the mask crop of this window: the one tests/crops_cases.py finds
    for its frame if it qualifies here too, else the same seeded search judged on the window; None when no candidate qualifies."""
    from tests import crops_cases

    M = dict(crops_cases.CASES)["fma-row"]
    if any(moved_by(window, origin, M, out_hw, "fma")):
        return M
    rng = np.random.default_rng(crops_cases.SEED)
    for _ in range(tries):
        a, c = float(rng.choice([3, 5, 6, 7])), float(rng.choice([-2, -1, 1, 2]))
        y0, j = int(rng.integers(1, 16)), int(rng.integers(64, 900))
        m01 = crops_oracle.inverse(crops_cases._m(a, c, 0, 0, 1, 0))[1]
        b1 = (32 * j + 15 + 0.5) / 1024.0 - m01 * y0
        M = crops_cases._m(a, c, -a * b1, 0, 1, 0)
        if any(moved_by(window, origin, M, out_hw, "fma")):
            return M
    return None


def _centre(mask_hw, origin):
    return (origin[0] + mask_hw[1] * 0.5, origin[1] + mask_hw[0] * 0.5)


def _warps():
    out = []

    def add(name, mask_hw, seed, origin, out_hw, M=None, **kw):
        out.append(Warp(name, mask_hw, seed, origin, M if M is not None else affine(_centre(mask_hw, origin), out_hw=out_hw, **kw), out_hw))

    add("identity-5x7", (5, 7), 1, (0, 0), (5, 7), M=EYE)
    add("identity-1x1", (5, 7), 2, (0, 0), (1, 1), M=((1.0, 0.0, -3.0), (0.0, 1.0, -2.0)))
    add("shift-fraction-1x37", (9, 40), 3, (0, 0), (1, 37), M=((1.0, 0.0, -0.3125), (0.0, 1.0, -3.71875)))
    add("shift-fraction-37x1", (40, 9), 4, (0, 0), (37, 1), M=((1.0, 0.0, -4.4), (0.0, 1.0, 0.53)))
    add("rot30-one-tile", (48, 40), 5, (3, 2), (TILE_H, TILE_W), zoom=1.4, rot=math.radians(30))
    add("rot90-tile-plus-row", (31, 33), 6, (0, 0), (TILE_H + 1, TILE_W), zoom=1.0, rot=math.pi / 2)
    add("rot200-tile-plus-col", (40, 48), 7, (-5, 4), (TILE_H, TILE_W + 1), zoom=1.7, rot=math.radians(200))
    add("zoom-in-3x-64", (20, 24), 8, (10, -7), (64, 64), zoom=3.0)
    add("zoom-out-3x-64", (48, 40), 9, (-11, -13), (64, 64), zoom=1.0 / 3.0)
    add("stress-64", (33, 47), 10, (6, 9), (64, 64), zoom=1.6, rot=math.radians(17), stretch=1.31, skew=0.23)
    add("stress-odd", (48, 40), 11, (-20, 15), (23, 41), zoom=0.9, rot=math.radians(-71), stretch=0.77, skew=-0.4)
    # all-set windows: the values are decided by the window's edges alone
    add("edge-left", (12, 14), -1, (5, 5), (18, 19), zoom=1.3, shift=(6.3, 0.0))
    add("edge-right", (12, 14), -1, (5, 5), (18, 19), zoom=1.3, shift=(-6.7, 0.0))
    add("edge-top", (12, 14), -1, (-30, -40), (18, 19), zoom=1.3, shift=(0.0, 5.9), rot=0.1)
    add("edge-bottom", (12, 14), -1, (-30, -40), (18, 19), zoom=1.3, shift=(0.0, -6.1), rot=-0.1)
    add("window-outside", (12, 14), -1, (200, 300), (18, 19), M=EYE)
    # the coordinate traps of the zoom-in crops, on a mask window
    from tests import crops_cases

    as_rows = lambda M: tuple(map(tuple, np.asarray(M, dtype=np.float32).tolist()))
    add("ties", (48, 40), 12, (0, 0), (16, 16), M=as_rows(dict(crops_cases.CASES)["ties"]))
    fma = find_fma_row(mask((48, 40), 13), (0, 0))
    if fma is None:  # the row that pins the contraction trap must not go missing without a word
        raise RuntimeError("tests/maskcrop_cases.py: the seeded search found no matrix on which fma contraction changes the mask crop")
    add("fma-row", (48, 40), 13, (0, 0), (16, 16), M=as_rows(fma))
    return tuple(out)


WARPS = _warps()


# ---- wide crops: the warp launch's layouts beyond 32 threads along x, at the sizes of tests/crops_cases.WIDE_SIZES ----
def _wide_warps():
    from tests import crops_cases

    out = []
    windows = (((33, 47), 10, (6, 9)), ((48, 40), 11, (-20, 15)))  # the windows of "stress-64" and "stress-odd"
    for hw in crops_cases.WIDE_SIZES:
        for k, ((mask_hw, seed, origin), kind) in enumerate(zip(windows, crops_cases.STRESS_KINDS)):
            M = crops_cases.stress_matrix(_centre(mask_hw, origin), mask_hw, hw, *kind)
            out.append(Warp(f"wide-{hw[0]}x{hw[1]}-{k}", mask_hw, seed, origin, tuple(map(tuple, M.tolist())), hw))
    return tuple(out)


WIDE_WARPS = _wide_warps()


def wide_planted(case, vis_interp, mistake):
    """(msk_vis, msk_noc) of one wide case under a mistake of tests/crops_cases.WIDE_MISTAKES."""
    from tests import crops_cases

    with crops_cases.planted_coordinates(mistake):
        vis, noc = maskcrop_oracle.warp_row(mask(case.mask_hw, case.seed), case.origin, case.M, case.out_hw, vis_interp)
    if mistake == "row_stride_8":  # the rows the loop never reaches keep what the buffer held, here 0
        skipped = ~crops_cases.rows_walked(*case.out_hw, stride=8)
        vis[skipped], noc[skipped] = 0, 0
    return vis, noc


# ---- check points: a selection that ends after one, two, three and four passes, and pixels up to p = 65535 ----
# How many byte passes the device's selection of the n_check smallest keys takes depends only on how many leading key bytes the
# n_check-th and the (n_check + 1)-th smallest keys share (maskcrop_oracle.selection_depth).  One in a few hundred sample ids shares
# three bytes on a 256 x 256 crop, one in some ten thousand on a 64 x 64 one, so the rows are searched for, not hoped for.
DEPTH_SEED = 0xC0FFEE1234567
DEPTH_N = 256
# 64 x 64, about 60 % set: the sample ids the search below returns (tests/test_maskcrop_oracle.py runs it for depths 0..2 and
# re-derives the depth of all four); depth 3 is too rare at this size to be searched for whenever the module is imported
DEPTH_IDS_64 = {0: 0, 1: 1, 2: 23, 3: 41403}


def depth_crop(size):
    """The (size,size) uint8 crop of the depth rows: 64 -> about 60 % set, 256 -> all set."""
    return mask((64, 64), 64) if size == 64 else np.ones((size, size), dtype=np.uint8)


def boundary_pair(noc, n_check, seed, sample_id):
    """(depth, p of the n_check-th smallest round-0 key, p of the next): the pair a selection has to part."""
    p = np.flatnonzero(np.asarray(noc).reshape(-1)).astype(np.int64)
    k = maskcrop_oracle.key(seed, sample_id, 0, p)
    at = np.argpartition(k, (n_check - 1, n_check))[n_check - 1:n_check + 1]
    a, b = int(k[at[0]]), int(k[at[1]])
    return next((d for d in range(4) if (a >> (24 - 8 * d)) != (b >> (24 - 8 * d))), 4), int(p[at[0]]), int(p[at[1]])


def find_depth_ids(noc, depths=(0, 1, 2, 3), tries=4000, n_check=DEPTH_N, seed=DEPTH_SEED):
    """{depth: the first sample id 0, 1, 2, ... at which the selection is that deep}; a depth-3 row also has the pair's pixels in the
    order opposite to their keys', so that a selection which stops a byte early and falls back on p takes the wrong pixel.  Raises
    where `tries` sample ids do not hold every depth asked for."""
    found = {}
    for sid in range(tries):
        d, pa, pb = boundary_pair(noc, n_check, seed, sid)
        if d in depths and d not in found and (d < 3 or pa > pb):
            found[d] = sid
            if len(found) == len(depths):
                return found
    raise RuntimeError(f"tests/maskcrop_cases.py: no sample id below {tries} for the selection depths {sorted(set(depths) - set(found))}")


_DEPTH_IDS = {}


def depth_ids(size):
    """{depth: sample id} for depths 0..3 on depth_crop(size), found once."""
    if size not in _DEPTH_IDS:
        _DEPTH_IDS[size] = dict(DEPTH_IDS_64) if size == 64 else find_depth_ids(depth_crop(size))
    return _DEPTH_IDS[size]


def large_p_masks():
    """[(name, (256,256) uint8 mask, sample id)]: the pixel index at the width it is packed in, 16 bits.
    last-300: only the last 300 pixels are set, p = 65236..65535 -- every selected point has bit 15 of p set;
    last-rows-200: 200 pixels among the last two rows, fewer than the check points -- the rounds path with large p;
    exactly-256: 256 pixels that include p = 0 and p = 65535 -- the selection takes everything, both ends of the range among it."""
    n = 256 * 256
    a = np.zeros(n, dtype=np.uint8)
    a[n - 300:] = 1
    b = np.zeros(n, dtype=np.uint8)
    b[n - 512 + np.random.default_rng(71).permutation(512)[:200]] = 1
    c = np.zeros(n, dtype=np.uint8)
    c[1 + np.random.default_rng(72).permutation(n - 2)[:254]] = 1
    c[0] = c[n - 1] = 1
    return [("last-300", a.reshape(256, 256), 5), ("last-rows-200", b.reshape(256, 256), 6), ("exactly-256", c.reshape(256, 256), 7)]


def planted_points(noc, n_check, seed, sample_id, mistake):
    """maskcrop_oracle.check_points of a crop with V >= n_check under a mistake of the selection:
    "top_24_bits": the keys are ordered by their top 24 bits, then by p (a selection that never looks at the last key byte);
    "p_12_bits": the pixel is taken out of the composite with 12 bits instead of 16."""
    p = np.flatnonzero(np.asarray(noc).reshape(-1)).astype(np.int64)
    assert len(p) >= n_check
    k = maskcrop_oracle.key(seed, sample_id, 0, p)
    if mistake == "top_24_bits":
        k = k >> np.uint64(8)
    q = p[np.lexsort((p, k))][:n_check]
    if mistake == "p_12_bits":
        q = q & 0xFFF
    w = noc.shape[1]
    return np.stack((q % w, q // w), axis=1)
