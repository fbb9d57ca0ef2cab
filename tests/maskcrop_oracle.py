"""Numpy restatement of the training mask crops' contract (include/lc_amd_maskcrop.h): the warps of a 0/1 window with the coordinates of
tests/crops_oracle.py (imported, not restated), the valid count, and the check points with their hash and round rule in plain integer
numpy.  Test infrastructure: nothing in the product imports it.

`opencv_float_linear` is a second statement of the linear warp: OpenCV's float path in float32 (table weights as fp32 products, the
four-tap sum in fp32), which tests/test_maskcrop_oracle.py holds to `k / 1024` bit for bit."""
import numpy as np

from tests import crops_oracle

NEAREST, LINEAR = crops_oracle.NEAREST, crops_oracle.LINEAR
MAX_ORIGIN = 1 << 24
MAX_CHECK = 256
MAX_CHECK_PIXELS = 65536
_M32 = np.uint64(0xFFFFFFFF)


def fmix32(v):
    """MurmurHash3's 32-bit finaliser on uint32 values (any shape), in uint64 arithmetic masked to 32 bits."""
    v = np.asarray(v, dtype=np.uint64) & _M32
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & _M32
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & _M32
    v = v ^ (v >> np.uint64(16))
    return v


def key(seed, sample_id, r, p):
    """key_r(p) as uint64 holding 32 bits; p may be an array."""
    seed = int(seed)
    k = fmix32(seed & 0xFFFFFFFF)
    k = fmix32(k ^ np.uint64((seed >> 32) & 0xFFFFFFFF))
    k = fmix32(k ^ np.uint64(int(sample_id) & 0xFFFFFFFF))
    k = fmix32(k ^ np.uint64(int(r)))
    return fmix32(k ^ np.asarray(p, dtype=np.uint64))


def taps(window, origin, sx, sy):
    """The 0/1 values of frame pixels (sx, sy) (int64 arrays): the window's bytes at (sx - x0, sy - y0), 0 outside the window."""
    Hm, Wm = window.shape
    u, v = sx - int(origin[0]), sy - int(origin[1])
    inside = (u >= 0) & (u < Wm) & (v >= 0) & (v < Hm)
    s = window[np.clip(v, 0, Hm - 1), np.clip(u, 0, Wm - 1)] != 0
    return np.where(inside, s, False).astype(np.int64)


def linear_parts(window, origin, M, out_hw):
    """(four taps, fx, fy) of the linear warp, each (h,w) int64."""
    X, Y = crops_oracle.coordinates(M, out_hw, LINEAR)
    X, Y = X >> 5, Y >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    t = [taps(window, origin, sx + dx, sy + dy) for dy in (0, 1) for dx in (0, 1)]
    return t, fx, fy


def linear_count(window, origin, M, out_hw):
    """k (h,w) int64 in 0..1024."""
    t, fx, fy = linear_parts(window, origin, M, out_hw)
    return (32 - fx) * (32 - fy) * t[0] + fx * (32 - fy) * t[1] + (32 - fx) * fy * t[2] + fx * fy * t[3]


def opencv_float_linear(window, origin, M, out_hw):
    """OpenCV's float path for a float32 0/1 source: the table entry of a weight pair is the fp32 product of (1 - f/32, f/32) in y and in
    x, and the result the fp32 sum S0 w0 + S1 w1 + S2 w2 + S3 w3 taken left to right."""
    t, fx, fy = linear_parts(window, origin, M, out_hw)
    one, step = np.float32(1.0), np.float32(1.0 / 32.0)
    ax1, ay1 = fx.astype(np.float32) * step, fy.astype(np.float32) * step
    ax0, ay0 = one - ax1, one - ay1
    wts = [ay0 * ax0, ay0 * ax1, ay1 * ax0, ay1 * ax1]
    S = [s.astype(np.float32) for s in t]
    acc = S[0] * wts[0]
    for s, wt in zip(S[1:], wts[1:]):
        acc = acc + s * wt
    assert acc.dtype == np.float32
    return acc


def warp_row(window, origin, M, out_hw, vis_interp=LINEAR):
    """(msk_vis (h,w) float32, msk_noc (h,w) uint8) of one good row."""
    X, Y = crops_oracle.coordinates(M, out_hw, NEAREST)
    noc = taps(window, origin, X >> 10, Y >> 10)
    if vis_interp == NEAREST:
        vis = noc.astype(np.float32)
    else:
        vis = linear_count(window, origin, M, out_hw).astype(np.float32) / np.float32(1024.0)
    return vis, noc.astype(np.uint8)


def rounds(noc, n_check, seed, sample_id):
    """The list of rounds, each an int64 array of pixels p = y w + x in output order (the last one truncated)."""
    p = np.flatnonzero(np.asarray(noc).reshape(-1)).astype(np.int64)
    out, have, r = [], 0, 0
    while have < n_check:
        k = key(seed, sample_id, r, p)
        order = np.lexsort((p, k))  # by key, then by p
        take = p[order][:n_check - have]
        out.append(take)
        have += len(take)
        r += 1
    return out


def selection_depth(noc, n_check, seed, sample_id):
    """How deep a selection of the n_check smallest round-0 keys from the top byte down has to look: the number of leading key bytes
    that the n_check-th and the (n_check + 1)-th smallest keys share, 0..3 (4 if the two keys are equal and only p parts them).  None
    where there are at most n_check valid pixels: nothing is left out, so there is nothing to select."""
    p = np.flatnonzero(np.asarray(noc).reshape(-1)).astype(np.int64)
    if len(p) <= n_check:
        return None
    k = np.partition(key(seed, sample_id, 0, p), (n_check - 1, n_check))
    a, b = int(k[n_check - 1]), int(k[n_check])
    return next((d for d in range(4) if (a >> (24 - 8 * d)) != (b >> (24 - 8 * d))), 4)


def check_points(noc, valid_th, n_check, seed, sample_id):
    """(n_check,2) int64 (x, y)."""
    w = noc.shape[1]
    cnt = int(np.count_nonzero(noc))
    if n_check == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if cnt < valid_th or cnt == 0:
        return np.full((n_check, 2), -1, dtype=np.int64)
    p = np.concatenate(rounds(noc, n_check, seed, sample_id))
    return np.stack((p % w, p // w), axis=1)


def mask_crops(masks, M, out_hw, mask_index=None, origin=None, vis_interp=LINEAR, valid_th=100, n_check=256, seed=0, sample_id=None):
    """The batch contract, bad rows included: dict(msk_vis (B,h,w) float32, msk_noc (B,h,w) bool, valid_cnt (B) int32, sym_ck_pts2d
    (B,n_check,2) int64, info (B) int32)."""
    masks, M = np.asarray(masks), np.asarray(M, dtype=np.float32)
    F, B = masks.shape[0], M.shape[0]
    h, w = out_hw
    assert n_check == 0 or h * w <= MAX_CHECK_PIXELS
    idx = np.arange(B) if mask_index is None else np.asarray(mask_index)
    org = np.zeros((B, 2), dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
    sid = np.arange(B) if sample_id is None else np.asarray(sample_id)
    vis = np.zeros((B, h, w), dtype=np.float32)
    noc = np.zeros((B, h, w), dtype=np.uint8)
    ck = np.full((B, n_check, 2), -1, dtype=np.int64)
    info = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if not (0 <= idx[b] < F) or not np.isfinite(M[b]).all() or np.abs(org[b]).max() > MAX_ORIGIN:
            info[b] = -1
            continue
        vis[b], noc[b] = warp_row(masks[idx[b]], org[b], M[b], out_hw, vis_interp)
        ck[b] = check_points(noc[b], valid_th, n_check, seed, sid[b])
    return dict(msk_vis=vis, msk_noc=noc.astype(bool), valid_cnt=noc.reshape(B, -1).sum(1).astype(np.int32), sym_ck_pts2d=ck, info=info)
