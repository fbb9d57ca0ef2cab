"""The background switch of include/lc_amd_bgstore.h as the composition it is defined by, in host numpy: `augment.draw` (gate and pick),
`augment.background_matrices` (region), `crops_oracle.warp_one` (cut) and `augment_oracle.blend` (blend).  Test infrastructure: nothing in
the product imports it.

`mistake` plants one deviation (tests/test_bgstore_host.py shows that the case list notices each):
    "hw_of_wrong_image"    the region is drawn for the size of the image after the chosen one
    "row_stride_padded"    image rows are read as if each started on a multiple of four bytes
    "tie_half_up"          an exact tie of the blend goes up instead of to the even neighbour
    "closed_rows_written"  a row whose gate is closed is blended with image 0
"""
import numpy as np

from lc_amd import augment
from tests import augment_oracle, crops_oracle

MISTAKES = ("hw_of_wrong_image", "row_stride_padded", "tie_half_up", "closed_rows_written")


def pick(cfg, seed, ids, sizes, mistake=None):
    """(gate (B,) int32, which (B,) int32 with -1 on closed rows, bg_hw (B,2) int32 with (1, 1) on closed rows)"""
    G = len(sizes)
    P, _ = augment.draw(cfg, seed, ids, G)
    gate = (P[:, 0] & augment.BIT_SWITCH).astype(np.int32)
    which = np.where(gate == 1, P[:, 1], -1).astype(np.int32)
    sized = (which + 1) % G if mistake == "hw_of_wrong_image" else which
    bg_hw = np.array([sizes[g] if open_ else (1, 1) for g, open_ in zip(sized, gate)], dtype=np.int32).reshape(-1, 2)
    return gate, which, bg_hw


def _padded_rows(image):
    """The image a reader sees that takes every row to start on a multiple of four bytes of the packed buffer."""
    hb, wb, _ = image.shape
    stride = -(-3 * wb // 4) * 4
    flat = np.concatenate((image.reshape(-1), np.zeros(hb * stride, dtype=np.uint8)))
    return np.stack([flat[y * stride:y * stride + 3 * wb] for y in range(hb)]).reshape(hb, wb, 3)


def _blend_half_up(fg, bg, msk):
    t = msk.astype(np.float32) * np.float32(1024)
    k = np.where(t >= 1024, 1024, np.where(t > 0, np.rint(np.where(t > 0, t, 0)), 0)).astype(np.int64)
    return ((k[None] * fg.astype(np.int64) + (1024 - k[None]) * bg.astype(np.int64) + 512) >> 10).astype(np.uint8)


def switch(crops, images, cfg, seed, ids, msk_in, mistake=None):
    """-> (switched crops (B,3,h,w) uint8, info (B,) int32, which (B,) int32, M (B,2,3) float32)"""
    B, _, h, w = crops.shape
    sizes = [im.shape[:2] for im in images]
    gate, which, bg_hw = pick(cfg, seed, ids, sizes, mistake)
    M = augment.background_matrices(seed, ids, bg_hw, (h, w))
    out = crops.copy()
    for b in range(B):
        if not gate[b] and mistake != "closed_rows_written":
            continue
        image = images[max(int(which[b]), 0)]
        if mistake == "row_stride_padded":
            image = _padded_rows(image)
        bg = crops_oracle.warp_one(image, M[b], (h, w)).transpose(2, 0, 1)
        out[b] = (_blend_half_up if mistake == "tie_half_up" else augment_oracle.blend)(crops[b], bg, msk_in[b])
    return out, gate.copy(), which, M
