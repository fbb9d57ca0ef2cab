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


# ---- across chunk edges: the encoder takes 1024 frame columns at a time, the indexer 256 counts ----
WIDE_FRAMES = ((3, 1030), (5, 2049))  # two and three encoder chunks; H is small to keep the lists short
ENC_CHUNK, IDX_CHUNK = 1024, 256


def wide_masks(H, W):
    """(name, (H,W) uint8 mask) of one wide frame."""
    yy, xx = np.mgrid[:H, :W]
    out = [("empty", np.zeros((H, W), np.uint8)), ("full", np.ones((H, W), np.uint8)), ("blob", blob(H, W, H + W)),
           ("checkerboard", ((xx + yy) & 1).astype(np.uint8))]
    m = np.zeros((H, W), np.uint8)
    m[H - 1, 1023] = m[0, 1024] = 1  # the foot of column 1023 and the head of column 1024: one run over the chunk edge
    out.append(("edge-run", m))
    m = np.zeros((H, W), np.uint8)
    m[0, 7] = m[H - 2:, 1023] = 1  # the last set pixel is the last pixel of column 1023: its run is closed by column 1024
    out.append(("last-of-1023", m))
    if W > 2 * ENC_CHUNK:
        # one run from column 1000 to column 2048: every boundary lies in a column < 1024 or >= 2048, the middle chunk holds none
        flat = np.zeros(H * W, np.uint8)
        flat[1000 * H + 1:2048 * H + 2] = 1
        flat[2048 * H + H - 1] = 1
        out.append(("empty-middle", np.ascontiguousarray(flat.reshape(W, H).T)))
    return out


def wide_windows(H, W):
    """(name, (x0, y0), (Hm, Wm)) for the encoder on a wide frame."""
    return [("frame", (0, 0), (H, W)),
            ("closing-alone", (0, 0), (H, ENC_CHUNK)),      # columns [0, 1024): the column that closes a run behind the window is alone in chunk two
            ("from-6", (6, 0), (H, W - 6)),                 # chunk edges at frame columns 1030 and 2054
            ("over-right-bottom", (9, 1), (H + 2, W))]


def boundaries(frame):
    """The column-major positions whose value differs from the one before (0 before position 0), in order."""
    flat = (np.asarray(frame) != 0).ravel(order="F")
    return np.flatnonzero(np.diff(flat.astype(np.int8), prepend=np.int8(0)))


def walked_columns(origin, hw, HW):
    """(xa, ncols): the frame columns [xa, xa + ncols) that the encoder walks for a window -- the window's columns inside the frame and,
    where the frame goes on behind them, the one column that closes a run which ends with the window."""
    xa, xb = max(origin[0], 0), min(origin[0] + hw[1], HW[1])
    return xa, (xb - xa) + (1 if xb < HW[1] else 0)


def encode_restarting(frame, xa=0, ncols=None, chunk=ENC_CHUNK):
    """The list of an encoder that takes `chunk` of the frame columns [xa, xa + ncols) at a time and forgets, from one chunk to the next,
    how many boundaries came before and where the last one lay: a planted mistake.  A later chunk writes over the first one's counts.
    `frame` is the frame that holds the window alone (rle_oracle.frame_of): all its boundaries lie in the walked columns."""
    H, W = frame.shape
    ncols = W - xa if ncols is None else ncols
    pos = boundaries(frame)
    col = pos // H
    assert ((col >= xa) & (col < xa + ncols)).all()
    row, n, last = {}, 0, 0
    for c0 in range(xa, xa + ncols, chunk):
        n, last = 0, 0
        for q in pos[(col >= c0) & (col < c0 + chunk)].tolist():
            row[n] = q - last
            n, last = n + 1, q
    row[n] = H * W - last
    return [row[i] for i in range(n + 1)]


def chunked_index_lists(H=64, W=64):
    """((name, counts, valid)) for the indexer, each of more than two chunks of 256 counts:
    carried-sum: zeros and ones, the running sum reaches H W only with the carries of all three chunks;
    carried-overflow: the sum is H W + 2^32 and passes 2^32 in the third chunk; the low 32 bits alone say H W."""
    HW = H * W
    ones = [1, 0, 1, 1] * 175
    good = ones + [HW - sum(ones)]
    over = [1] * 600 + [BIG, HW + 2 ** 32 - 600 - BIG]
    assert len(good) > 2 * IDX_CHUNK and sum(good) == HW and sum(good[:2 * IDX_CHUNK]) < HW
    assert sum(over) == HW + 2 ** 32 and sum(over[:2 * IDX_CHUNK]) < 2 ** 32 and all(0 <= c <= BIG for c in over)
    return (("carried-sum", good, True), ("carried-overflow", over, False))


def valid_with(counts, H, W, mistake):
    """Whether an indexer judges the list valid under a planted mistake: "sum_32_bits" keeps the running sum in 32 bits,
    "no_carry" starts every chunk of 256 counts from zero."""
    if mistake == "sum_32_bits":
        total = 0
        for c in counts:
            total = (total + int(c)) & 0xFFFFFFFF
        return total == H * W
    assert mistake == "no_carry"
    return sum(int(c) for c in counts[(len(counts) - 1) // IDX_CHUNK * IDX_CHUNK:]) == H * W


def windows(H, W):
    """(name, (x0, y0), (Hm, Wm)) per frame; every one with info 0."""
    return [("frame", (0, 0), (H, W)), ("inside", (5, 7), (H - 12, W - 11)),
            ("over-left", (-9, 3), (H - 6, W - 4)), ("over-right", (W - 20, 2), (H - 4, 33)), ("over-top", (4, -11), (H - 5, W - 8)),
            ("over-bottom", (3, H - 13), (29, W - 6)), ("over-all", (-3, -2), (H + 5, W + 7)),
            ("outside", (W + 5, 2), (16, 16)), ("outside-above", (1, -40), (33, 9)),
            ("one-pixel", (W - 1, H - 1), (1, 1)), ("one-past-a-wave", (-3, -2), (H + 5, 65)),
            ("second-tile", (-250, 1), (H - 2, 300))]  # columns 256.. of the window belong to a second workgroup
