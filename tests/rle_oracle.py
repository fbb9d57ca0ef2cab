"""The run-length mask store restated in numpy and plain Python (include/lc_amd_rle.h): a mask of a frame with H rows and W columns is a
list of counts over the column-major positions p = x H + y, run k having value k & 1.  Everything here goes through the DECODED mask or
through Python's whole numbers, never through the kernels' run arithmetic."""
import numpy as np

MAX_SIZE = 16384
MAX_ORIGIN = 16777216


def is_valid(counts, H, W):
    """The counts sum to exactly H W (Python's whole numbers: no width to overflow) and the size is in range."""
    return 1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE and sum(int(c) for c in counts) == H * W


def decode(counts, H, W):
    """(H,W) uint8 of a valid list: zero counts anywhere are fine."""
    counts = np.asarray(counts, dtype=np.int64)
    assert is_valid(counts, H, W)
    return np.ascontiguousarray(np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8).reshape(W, H).T)


def encode(mask):
    """The canonical list of an (H,W) mask (non-zero = set): only counts[0] may be zero."""
    flat = (np.asarray(mask) != 0).ravel(order="F")
    edges = np.flatnonzero(np.diff(flat.astype(np.int8), prepend=np.int8(0))) if flat.size else np.zeros(0, np.int64)
    # prepend 0: a mask that starts with a 1 has an edge at position 0, which makes the empty first run
    bounds = np.concatenate(([0], edges, [flat.size]))
    return np.diff(bounds).astype(np.uint32)


def area_box(mask):
    """(area, [x_min, y_min, x_max, y_max]) of the set pixels, four times -1 for none."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return 0, [-1, -1, -1, -1]
    return int(ys.size), [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def index(counts_flat, offsets, sizes):
    """The index launch over a flat store: (ends (T) uint32, zero where no mask with good offsets wrote; area (F); box (F,4); valid (F))."""
    counts_flat = np.asarray(counts_flat, dtype=np.uint32)
    T, F = len(counts_flat), len(offsets) - 1
    ends = np.zeros(T, dtype=np.uint32)
    area, box, valid = np.zeros(F, np.int32), np.full((F, 4), -1, np.int32), np.full(F, -1, np.int32)
    for f in range(F):
        a, b, (H, W) = int(offsets[f]), int(offsets[f + 1]), (int(sizes[f][0]), int(sizes[f][1]))
        if not (0 <= a <= b <= T) or not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
            continue
        run = 0
        for k in range(a, b):
            run += int(counts_flat[k])
            ends[k] = run & 0xFFFFFFFF
        if run == H * W:
            valid[f] = 0
            area[f], box[f] = area_box(decode(counts_flat[a:b], H, W))
    return ends, area, box, valid


def window_of(mask, origin, hw):
    """The (Hm,Wm) window at origin = (x0, y0) of an (H,W) frame: 0 outside the frame."""
    (x0, y0), (Hm, Wm) = origin, hw
    H, W = mask.shape
    out = np.zeros((Hm, Wm), dtype=np.uint8)
    ii, jj = np.arange(Hm) + y0, np.arange(Wm) + x0
    vi, vj = (ii >= 0) & (ii < H), (jj >= 0) & (jj < W)
    out[np.ix_(vi, vj)] = mask[np.ix_(ii[vi], jj[vj])]
    return out


def decode_rows(masks, valid, F, mask_index, origins, hw):
    """The decode launch: masks[f] is the decoded frame of mask f (None where invalid).  -> (out (B,Hm,Wm) uint8, info (B) int32)."""
    B = len(mask_index)
    out, info = np.zeros((B,) + tuple(hw), dtype=np.uint8), np.zeros(B, dtype=np.int32)
    for b, f in enumerate(mask_index):
        x0, y0 = (0, 0) if origins is None else (int(origins[b][0]), int(origins[b][1]))
        if not (0 <= f < F) or valid[f] != 0 or abs(x0) > MAX_ORIGIN or abs(y0) > MAX_ORIGIN:
            info[b] = -1
            continue
        out[b] = window_of(masks[f], (x0, y0), hw)
    return out, info


def frame_of(window, origin, HW):
    """The (H,W) frame that holds `window` (non-zero = set) at origin: 0 outside the window; the window's pixels outside the frame drop out."""
    (x0, y0), (H, W) = origin, HW
    Hm, Wm = window.shape
    frame = np.zeros((H, W), dtype=np.uint8)
    ii, jj = np.arange(Hm) + y0, np.arange(Wm) + x0
    vi, vj = (ii >= 0) & (ii < H), (jj >= 0) & (jj < W)
    frame[np.ix_(ii[vi], jj[vj])] = window[np.ix_(vi, vj)] != 0
    return frame


def encode_rows(windows, sizes, origins, cap):
    """The encode launch.  -> (counts_out (F,cap) uint32, n_runs (F), info (F))."""
    F = len(windows)
    out, n_runs, info = np.zeros((F, cap), dtype=np.uint32), np.zeros(F, np.int32), np.zeros(F, np.int32)
    for f in range(F):
        H, W = windows[f].shape if sizes is None else (int(sizes[f][0]), int(sizes[f][1]))
        x0, y0 = (0, 0) if origins is None else (int(origins[f][0]), int(origins[f][1]))
        if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE) or abs(x0) > MAX_ORIGIN or abs(y0) > MAX_ORIGIN:
            info[f] = -1
            continue
        c = encode(frame_of(windows[f], (x0, y0), (H, W)))
        n_runs[f] = len(c)
        if len(c) > cap:
            info[f] = -2
        else:
            out[f, :len(c)] = c
    return out, n_runs, info


# ---- COCO's compressed string, step by step, as lc_amd/rle.py states the rule


def to_string(counts):
    out = []
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i >= 2:  # from the third count on: less the count two places before
            x -= counts[i - 2]
        while True:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
            if not more:
                break
    return "".join(out)


def from_string(s):
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)  # the sign, from bit 4 of the last group
        if len(counts) >= 2:
            x += counts[-2]
        counts.append(x)
    return counts
