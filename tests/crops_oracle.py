"""Numpy restatement of the zoom-in crops' contract (include/lc_amd_crop.h): OpenCV's published fixed-point scheme for 8-bit images
(INTER_BITS = 5, AB_BITS = 10, constant border 0).  float64 with every product and sum rounded on its own (numpy never fuses), int64 for
the coordinates, float32 for the output stage.  Test infrastructure: nothing in the product imports it.

`mistake` plants one deviation from the contract (tests/test_crops_oracle.py shows that the case list notices each):
    "swap_fxfy"  "taps_shifted"  "no_delta"  "no_blend_half"  "border_per_pixel"  "rint_half_up"  "fma"
"""
from fractions import Fraction

import numpy as np

NEAREST, LINEAR = "nearest", "linear"
LIMIT = 2.0 ** 30
MISTAKES = ("swap_fxfy", "taps_shifted", "no_delta", "no_blend_half", "border_per_pixel", "rint_half_up", "fma")


def inverse(M):
    """(m00, m01, b1, m10, m11, b2) in float64 from one (2,3) forward matrix."""
    M = np.asarray(M, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
        m00, m01, m10, m11 = M[1, 1] * D, (-M[0, 1]) * D, (-M[1, 0]) * D, M[0, 0] * D
        b1 = (-m00) * M[0, 2] - m01 * M[1, 2]
        b2 = (-m10) * M[0, 2] - m11 * M[1, 2]
    return m00, m01, b1, m10, m11, b2


def _fix(v, half_up=False):
    with np.errstate(all="ignore"):
        r = np.floor(v + 0.5) if half_up else np.rint(v)
        return np.clip(r, -LIMIT, LIMIT).astype(np.int64)


def _fma(a, ys, b):
    """fl(a * y + b) with ONE rounding, exactly (rational arithmetic; Fraction -> float rounds to nearest even)."""
    return np.asarray([float(Fraction(float(a)) * Fraction(float(y)) + Fraction(float(b))) for y in ys], dtype=np.float64)


def coordinates(M, out_hw, interp, mistake=None):
    """(X, Y) int64 (h,w): the fixed-point source coordinates of every crop pixel, delta included."""
    h, w = out_hw
    m00, m01, b1, m10, m11, b2 = inverse(M)
    ys, xs = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    hu = mistake == "rint_half_up"
    with np.errstate(all="ignore"):
        if mistake == "fma":
            X0, Y0 = _fix(_fma(m01, ys, b1) * 1024.0), _fix(_fma(m11, ys, b2) * 1024.0)
        else:
            X0, Y0 = _fix((m01 * ys + b1) * 1024.0, hu), _fix((m11 * ys + b2) * 1024.0, hu)
        ax, ay = _fix(m00 * xs * 1024.0, hu), _fix(m10 * xs * 1024.0, hu)
    delta = 0 if mistake == "no_delta" else (512 if interp == NEAREST else 16)
    return X0[:, None] + ax[None, :] + delta, Y0[:, None] + ay[None, :] + delta


def _taps(frame, sx, sy):
    """frame (H,W,C) at integer positions (h,w), 0 outside; -> int64 (h,w,C) and the inside mask."""
    H, W = frame.shape[:2]
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    v = frame[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64)
    return np.where(inside[..., None], v, 0), inside


def warp_one(frame, M, out_hw, interp=LINEAR, mistake=None):
    """One crop (h,w,C) uint8 of one (H,W,C) uint8 frame; a matrix with a non-finite entry gives all border."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3
    h, w = out_hw
    if not np.isfinite(np.asarray(M, dtype=np.float32)).all():
        return np.zeros((h, w, frame.shape[2]), dtype=np.uint8)
    X, Y = coordinates(M, out_hw, interp, mistake)
    if interp == NEAREST:
        v, _ = _taps(frame, X >> 10, Y >> 10)
        return v.astype(np.uint8)
    X, Y = X >> 5, Y >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    if mistake == "swap_fxfy":
        fx, fy = fy, fx
    if mistake == "taps_shifted":
        sx = sx + 1
    t = [_taps(frame, sx + dx, sy + dy) for dy in (0, 1) for dx in (0, 1)]
    wts = [(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy]
    acc = sum(wt[..., None] * s for wt, (s, _) in zip(wts, t))
    v = (acc + (0 if mistake == "no_blend_half" else 512)) >> 10
    if mistake == "border_per_pixel":
        v = np.where((t[0][1] & t[1][1] & t[2][1] & t[3][1])[..., None], v, 0)
    return v.astype(np.uint8)


def warp(frames, M, out_hw, frame_index=None, interp=LINEAR, mistake=None):
    """(out (B,C,h,w) uint8, info (B) int32): the batch contract, bad rows included."""
    frames, M = np.asarray(frames), np.asarray(M, dtype=np.float32)
    F, B = frames.shape[0], M.shape[0]
    idx = np.arange(B) if frame_index is None else np.asarray(frame_index)
    out = np.zeros((B, frames.shape[3]) + tuple(out_hw), dtype=np.uint8)
    info = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if not (0 <= idx[b] < F) or not np.isfinite(M[b]).all():
            info[b] = -1
            continue
        out[b] = warp_one(frames[idx[b]], M[b], out_hw, interp, mistake).transpose(2, 0, 1)
    return out, info


def finish(v, normalize=None):
    """The float output stage in float32: v / 255, then (. - mean_c) / std_c; v is (B,C,h,w) uint8."""
    q = v.astype(np.float32) / np.float32(255.0)
    if normalize is not None:
        mean, std = (np.asarray(a, dtype=np.float32).reshape(1, -1, 1, 1) for a in normalize)
        with np.errstate(all="ignore"):
            q = (q - mean) / std
    assert q.dtype == np.float32
    return q


def three_point_solve(src, dst):
    """The (2,3) matrix that takes three points src (3,2) to dst (3,2), in float64 (what cv2.getAffineTransform computes)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    A = np.concatenate((src, np.ones((3, 1))), axis=1)
    return np.linalg.solve(A, dst).T
