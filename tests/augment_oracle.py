"""Numpy restatement of include/lc_amd_augment.h (the stages of the launch, in integers, on whole images: no tiles, no halo) and of the
host side's building blocks in lc_amd/augment.py (the key, u, the two weight builders, the table steps), written out a second time."""
import math

import numpy as np
import torch

OP_SNP, OP_SNPV, OP_DROP, OP_HOST = 65537, 65538, 65539, 131072
M32 = 0xFFFFFFFF


def f(v):
    """MurmurHash3's 32-bit finaliser on Python ints or uint64 arrays that hold 32 bits."""
    v = np.asarray(v, dtype=np.uint64) & np.uint64(M32)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return v ^ (v >> np.uint64(16))


def key(seed, sample_id, op, q):
    k = f(seed & M32)
    k = f(k ^ np.uint64(seed >> 32))
    k = f(k ^ np.uint64(int(sample_id) & M32))
    k = f(k ^ np.uint64(op))
    return f(k ^ (np.asarray(q, dtype=np.int64).astype(np.uint64) & np.uint64(M32)))


def u(seed, sample_id, op, i):
    return float(int(key(seed, sample_id, op, i)) >> 8) / 2.0 ** 24


def reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def filter5(img, wq):
    """img (3,h,w) uint8, wq 25 Q16 weights row-major from (dy, dx) = (-2, -2): (sum w tap + 32768) >> 16 with BORDER_REFLECT_101."""
    _, h, w = img.shape
    acc = np.full(img.shape, 32768, dtype=np.int64)
    src = img.astype(np.int64)
    for dy in range(-2, 3):
        ry = reflect(np.arange(h) + dy, h)
        for dx in range(-2, 3):
            rx = reflect(np.arange(w) + dx, w)
            acc += int(wq[(dy + 2) * 5 + dx + 2]) * src[:, ry][:, :, rx]
    return (acc >> 16).astype(np.uint8)


def blend(fg, bg, msk):
    """(k fg + (1024 - k) bg) / 1024 rounded half to even, k = rint(1024 msk) clamped to 0..1024 (NaN: 0)."""
    t = msk.astype(np.float32) * np.float32(1024)
    k = np.where(t >= 1024, 1024, np.where(t > 0, np.rint(np.where(t > 0, t, 0)), 0)).astype(np.int64)
    S = k[None] * fg.astype(np.int64) + (1024 - k[None]) * bg.astype(np.int64)
    q, rem = S >> 10, S & 1023
    return (q + ((rem > 512) | ((rem == 512) & (q & 1 == 1)))).astype(np.uint8)


def row_ok(P, h, w, G, has_mask, pointwise):
    P = P.astype(np.int64)
    bits = int(P[0])
    ok = (bits & ~63) == 0 and not P[56:].any()
    for bit, lo in ((4, 6), (16, 31)):
        if bits & bit:
            ok = ok and P[lo:lo + 25].min() >= 0 and int(P[lo:lo + 25].sum()) == 65536
    if bits & 8:
        ok = ok and 1 <= P[4] <= h and 1 <= P[5] <= w
    if bits & 1:
        ok = ok and has_mask and G > 0 and 0 <= P[1] < G
    if pointwise and bits & 20:
        ok = False
    return bool(ok)


def augment(crops, params, lut, msk_in=None, backgrounds=None, seed=0, sample_id=None, pointwise=False):
    """-> (out (B,3,h,w) uint8, info (B,) int32)"""
    B, _, h, w = crops.shape
    G = 0 if backgrounds is None else len(backgrounds)
    out, info = np.empty_like(crops), np.zeros(B, dtype=np.int32)
    ys, xs = np.mgrid[0:h, 0:w]
    for b in range(B):
        P, sid = params[b].astype(np.int64), (b if sample_id is None else int(sample_id[b]))
        v = crops[b].copy()
        if not row_ok(P, h, w, G, msk_in is not None, pointwise):
            out[b], info[b] = v, -1
            continue
        bits = int(P[0])
        if bits & 1:
            v = blend(v, backgrounds[P[1]], msk_in[b])
        if bits & 2:
            p = ys * w + xs
            hit = key(seed, sid, OP_SNP, p) < np.uint64(int(P[2]) & M32)
            salt = (key(seed, sid, OP_SNPV, p) >> np.uint64(31)).astype(bool)
            v = np.where(hit[None], np.where(salt[None], 255, 0), v).astype(np.uint8)
        if bits & 4:
            v = filter5(v, P[6:31])
        if bits & 8:
            cell = (ys * P[4] // h) * P[5] + (xs * P[5] // w)
            v = np.where((key(seed, sid, OP_DROP, cell) < np.uint64(int(P[3]) & M32))[None], 0, v).astype(np.uint8)
        if bits & 16:
            v = filter5(v, P[31:56])
        if bits & 32:
            v = np.stack([lut[b, c][v[c]] for c in range(3)])
        out[b] = v
    return out, info


def finish(u8, dtype, normalize=None):
    """The stated fp32 operations on the bytes, as a CPU torch tensor of `dtype`: v / 255, (. - mean) / std, one rounding to 16 bits."""
    if dtype == torch.uint8:
        return torch.from_numpy(u8.copy())
    q = u8.astype(np.float32) / np.float32(255)
    if normalize is not None:
        mean, std = (np.asarray(a, dtype=np.float32).reshape(1, 3, 1, 1) for a in normalize)
        q = (q - mean) / std
    assert q.dtype == np.float32
    return torch.from_numpy(q).to(dtype)


# ---- the host side's building blocks


def quantise(g):
    q = [int(math.floor(x * 65536.0 + 0.5)) for x in np.asarray(g, dtype=np.float64).reshape(25)]
    q[12] += 65536 - sum(q)
    return np.array(q, dtype=np.int64)


def gaussian_weights(sigma):
    g = np.array([math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-2, 3)])
    g = g / g.sum()
    return quantise(g[:, None] * g[None, :])


def motion_weights(angle_deg, d):
    t = math.radians(angle_deg)
    grid = np.zeros((5, 5))
    for s in range(-2, 3):
        wgt = (1 - d) / 2 + (s + 2) / 4 * d
        px, py = 2 + s * math.sin(t), 2 - s * math.cos(t)
        for yy in range(5):
            for xx in range(5):  # the bilinear hat of the tap at every grid point
                grid[yy, xx] += wgt * max(0.0, 1 - abs(px - xx)) * max(0.0, 1 - abs(py - yy))
    return quantise(grid / grid.sum())


def table_step(t, fn):
    return np.clip(np.rint(np.array([fn(float(v)) for v in t])), 0, 255).astype(np.int64)
