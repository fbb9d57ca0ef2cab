"""The shapes at which the run-length kernels can go wrong (tests/test_gpu_rle.py, tests/test_rle_oracle.py, the pycocotools hand-off):
three frame sizes -- H below a wavefront, equal to one, and no multiple of one -- and per frame the lists and windows named below."""
import numpy as np

FRAMES = ((37, 53), (64, 64), (130, 67))  # (H, W)
BIG = 2 ** 32 - 1


def blob(H, W, seed):
    """A few overlapping discs: an object-like mask."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), dtype=bool)
    for _ in range(3):
        cx, cy, r = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H, rng.uniform(0.1, 0.3) * min(H, W)
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    return m.astype(np.uint8)


def valid_lists(H, W):
    """(name, counts) of the valid lists of one frame; the counts as Python's whole numbers."""
    HW = H * W
    out = [("empty", [HW]), ("full", [0, HW]), ("starts-with-1", [0, 3, HW - 3]),
           ("corner-tl", [0, 1, HW - 1]), ("corner-bl", [H - 1, 1, HW - H]), ("corner-tr", [HW - H, 1, H - 1]), ("corner-br", [HW - 1, 1]),
           ("alternate", [1] * HW),                                   # HW runs of length 1
           ("long-run", [H + 5, 3 * H + 7, HW - 4 * H - 12]),          # one run longer than 3 H: it spans columns
           ("zeros-inside", [7, 0, 0, 5, 0, 2 * H, 0, 0, 0, 4, HW - 2 * H - 16, 0]),  # zero counts in the middle and at the end
           ("column-cross", [2 * H - 2, 4, HW - 2 * H - 2])]           # two pixels at the foot of a column, two at the head of the next
    from tests import rle_oracle

    out.append(("blob", [int(c) for c in rle_oracle.encode(blob(H, W, H + W))]))
    yy, xx = np.mgrid[:H, :W]
    out.append(("checkerboard", [int(c) for c in rle_oracle.encode(((xx + yy) & 1).astype(np.uint8))]))
    return out


def invalid_lists(H, W):
    HW = H * W
    return [("sum-plus-1", [5, 9, HW - 13]), ("sum-minus-1", [5, 9, HW - 15]),
            ("wraps-to-HW", [HW, 2 ** 31, 2 ** 31]),                   # 64 bits: HW + 2^32; the low 32 bits alone say HW
            ("partial-overflow", [BIG, BIG, 3, HW]), ("no-counts", [])]


def windows(H, W):
    """(name, (x0, y0), (Hm, Wm)) per frame; every one with info 0."""
    return [("frame", (0, 0), (H, W)), ("inside", (5, 7), (H - 12, W - 11)),
            ("over-left", (-9, 3), (H - 6, W - 4)), ("over-right", (W - 20, 2), (H - 4, 33)), ("over-top", (4, -11), (H - 5, W - 8)),
            ("over-bottom", (3, H - 13), (29, W - 6)), ("over-all", (-3, -2), (H + 5, W + 7)),
            ("outside", (W + 5, 2), (16, 16)), ("outside-above", (1, -40), (33, 9)),
            ("one-pixel", (W - 1, H - 1), (1, 1)), ("one-past-a-wave", (-3, -2), (H + 5, 65)),
            ("second-tile", (-250, 1), (H - 2, 300))]  # columns 256.. of the window belong to a second workgroup
