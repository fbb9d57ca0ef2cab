"""Exact probes for the four streaming reductions (TEST INFRASTRUCTURE ONLY; pure torch, runs on any device).

`lc_sqnorm_kernel`, `lc_dense_aux_fwd_kernel`, `lc_xyz_bin_loss_fwd_kernel` and `block_lse` / `lse_thread_share` reduce a whole map to a
few scalars with several requests in flight per thread, capped grids and a last-arriver sum.  A dense random input checks such a sum
statistically; the probes here make it an integer identity:

  * the launch geometry of each kernel, restated from its launcher, and from it the CRITICAL POSITIONS -- the first and the last element
    and both sides of every index edge the kernel has (vector group, in-flight slot, round, workgroup, grid-stride wrap, sample, slab,
    scalar tail), plus elements owned by workgroups 0 / 255 / 256 / last (the last arriver adds the partials in a loop that strides by 256);
  * three 0/1 patterns -- all-hot, one-hot at a position, seeded random-hot -- as input tensors in which a cold element contributes
    exactly 0 and a hot one exactly 1 (or 100, or 9) to the sum;
  * the exact expected result of a pattern from its integer counts.

tests/test_reduction_probes.py proves the expectations against the plain float64 torch formulas and the position sets against numbers
written out by hand; tests/test_gpu_reduction_coverage.py runs the kernels on the patterns."""
from __future__ import annotations

import numpy as np
import torch

HOT_SQ = 3.0      # a one-hot probe of the sum of squares is 3: counted twice it reads 18, not 2
BIG = 100.0       # a saturated logit: exp(-100) vanishes against 1 in fp32, and 100 is exact in fp16 / bf16
SPIKE = 20.0      # the log-sum-exp spike: left out of the normaliser it scales every weight by e^20


def _ceil_div(a, b):
    return -(-a // b)


class Positions(dict):
    """label -> element index, in order of priority (ends and edges first); indices outside [0, n) are not kept."""

    def __init__(self, n):
        super().__init__()
        self.n = n

    def add(self, label, i):
        if 0 <= i < self.n and label not in self:
            self[label] = int(i)

    def edge(self, label, e):
        """both sides of the edge in front of element `e`"""
        self.add(label + "-", e - 1)
        self.add(label + "+", e)

    def pick(self, limit=None):
        """distinct indices in priority order, at most `limit` of them"""
        out = list(dict.fromkeys(self.values()))
        return out if limit is None else out[:limit]


def random_hot(shape, seed, device="cpu"):
    """seeded 0/1 pattern, about half of it hot (generated on the CPU: the same pattern whatever the device)"""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    if n > (1 << 22):  # large maps: drawn on the device (still seeded)
        gd = torch.Generator(device=device).manual_seed(seed)
        return torch.rand(shape, generator=gd, device=device) < 0.5
    return (torch.rand(shape, generator=g) < 0.5).to(device)


def ulps_apart(a, b):
    """distance of two float32 tensors of one sign in units in the last place"""
    a = torch.as_tensor(a, dtype=torch.float32).contiguous().cpu()
    b = torch.as_tensor(b, dtype=torch.float32).contiguous().cpu()
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


def f32(x):
    """a float64 value rounded once to float32"""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.float32)


# ---- sum of squares -------------------------------------------------------------------------------------------------------------------
SQ_THREADS, SQ_AHEAD, SQ_MAX_BLOCKS = 256, 4, 512


def sqnorm_grid(n):
    """lc_clip.hip grid_for_sqnorm: 32 elements per thread before the grid grows, at most kClipMaxBlocks = 512 workgroups"""
    return min(SQ_MAX_BLOCKS, max(1, _ceil_div(n, SQ_THREADS * 32)))


def sqnorm_positions(n, vec=True):
    """lc_sqnorm_kernel as launched by launch_sqnorm: request r (elements 4r .. 4r+3) of n4 = n / 4 belongs to thread r % stride,
    in-flight slot (r / stride) % 4 of round r / (4 stride), stride = grid * 256; the elements behind 4 n4 are walked one by one by
    threads 0, 1, 2.  vec = False (a view that does not start on a 16-byte boundary): n4 = 0, element e belongs to thread e % stride."""
    g = sqnorm_grid(n)
    stride = g * SQ_THREADS
    p = Positions(n)
    p.add("first", 0)
    p.add("last", n - 1)
    w = 4 if vec else 1  # elements per request
    n4 = n // 4 if vec else 0
    if vec:
        p.edge("group", 4)
        p.edge("tail", 4 * n4)
        for e in range(4 * n4, n):
            p.add(f"tail{e - 4 * n4}", e)
        p.add("last_group", 4 * (n4 - 1))
    walk = n4 if vec else n
    for u in range(1, _ceil_div(walk, stride) + 1):  # slot edges; u = 4, 8, ...: round edges (SQ_AHEAD * stride)
        p.edge(f"slot{u}", w * u * stride)
    p.edge("wg", w * SQ_THREADS)
    for label, block in (("wg255", 255), ("wg256", 256), ("wg_last", g - 1)):
        if 0 < block < g:
            p.add(label, w * block * SQ_THREADS)
            p.add(label + "_end", w * (block + 1) * SQ_THREADS - 1)
    p.add("wave", w * 64)
    p.add("second", 1)
    return p


def sq_pattern(n, hot, dtype=torch.float32, device="cpu"):
    """hot: 'all', an element index (one-hot, value 3) or a seed ('random', seed) -> (tensor, exact sum of squares as an int)"""
    if hot == "all":
        return torch.ones(n, dtype=dtype, device=device), n
    if isinstance(hot, tuple):
        m = random_hot((n,), hot[1], device)
        return m.to(dtype), int(m.sum())
    x = torch.zeros(n, dtype=dtype, device=device)
    x[hot] = HOT_SQ
    return x, int(HOT_SQ * HOT_SQ)


# ---- dense auxiliary losses -----------------------------------------------------------------------------------------------------------
AUX_THREADS, AUX_MAX_BLOCKS = 256, 1024


def aux_geometry(B, HW):
    """lc_dense_aux.hip launch_dense_aux_fwd: one request of V pixels per thread (V = 4 where H*W % 4 == 0 and the maps are aligned)
    up to kDenseAuxMaxBlocks = 1024 workgroups of 256 threads, then a grid-stride loop.  -> (V, grid, stride in requests, requests)"""
    n = B * HW
    V = 4 if HW % 4 == 0 else 1
    grid = min(AUX_MAX_BLOCKS, max(1, _ceil_div(n, 4 * AUX_THREADS)))
    return V, grid, grid * AUX_THREADS, n // V


def aux_positions(B, HW):
    """flat pixel indices b * HW + px: request j (pixels V j .. V j + V - 1) belongs to thread j % stride of the grid, iteration j / stride"""
    V, grid, stride, nv = aux_geometry(B, HW)
    n = B * HW
    p = Positions(n)
    p.add("first", 0)
    p.add("last", n - 1)
    for b in sorted({1, B - 1}):
        p.edge(f"sample{b}", b * HW)
    p.edge("group", 4)
    p.add("lane1", 1)
    p.add("lane2", 2)
    p.add("last_request", V * (nv - 1))
    p.edge("wg", V * AUX_THREADS)
    for k in range(1, _ceil_div(nv, stride) + 1):
        p.edge(f"wrap{k}", V * k * stride)
    for label, block in (("wg255", 255), ("wg256", 256), ("wg_last", grid - 1)):
        if 0 < block < grid:
            p.add(label, V * block * AUX_THREADS)
            p.add(label + "_end", V * (block + 1) * AUX_THREADS - 1)
    p.add("wave", V * 64)
    return p


def aux_inputs(B, H, W, vis_hot=None, x_hot=None, mask_hot=None, w_hot=None, dtype=torch.float32, device="cpu"):
    """Maps of the dense auxiliary losses in which only the hot elements contribute: seg and weight logits +100, msk_vis = 1 (hot: 0, which
    is hot for the seg logit and both weight logits of the pixel), weight logit -100 at a hot element of `w_hot` (B,2,H,W), coordinates and
    their targets 0 with mask 1 (x_hot (B,3,H,W): coordinate 1) or coordinates 1 with the mask as the pattern (mask_hot (B,H,W)).
    -> dict(xyz, msk_noc (bool), tgt, seg, vis, wl)"""
    f = dict(dtype=torch.float32, device=device)
    vis = torch.ones(B, H, W, **f) if vis_hot is None else (~vis_hot.to(device)).float()
    wl = torch.full((B, 2, H, W), BIG, **f)
    if w_hot is not None:
        wl = torch.where(w_hot.to(device), -wl, wl)
    if mask_hot is not None:
        xyz, msk = torch.ones(B, 3, H, W, **f), mask_hot.to(device).clone()
    else:
        xyz = torch.zeros(B, 3, H, W, **f) if x_hot is None else x_hot.to(device).float()
        msk = torch.ones(B, H, W, dtype=torch.bool, device=device)
    return dict(xyz=xyz.to(dtype), msk_noc=msk, tgt=torch.zeros(B, 3, H, W, **f), seg=torch.full((B, 1, H, W), BIG, **f).to(dtype), vis=vis, wl=wl.to(dtype))


def aux_counts(B, H, W, vis_hot=None, x_hot=None, mask_hot=None, w_hot=None):
    """hot terms of (loss_noc, loss_seg, loss_weight_seg) as integers; a weight logit of -100 under msk_vis = 0 is cold again"""
    k_noc = 3 * int(mask_hot.sum()) if mask_hot is not None else (0 if x_hot is None else int(x_hot.sum()))
    k_seg = 0 if vis_hot is None else int(vis_hot.sum())
    v2 = torch.zeros(B, 2, H, W, dtype=torch.bool, device=(w_hot if w_hot is not None else vis_hot).device) if (vis_hot is not None or w_hot is not None) else None
    if v2 is None:
        return k_noc, k_seg, 0
    if vis_hot is not None:
        v2 = v2 | vis_hot[:, None].to(v2.device)
    if w_hot is not None:
        v2 = v2 ^ w_hot
    return k_noc, k_seg, int(v2.sum())


def aux_expected(k_noc, k_seg, k_w, n, seg_type):
    """(loss_noc, loss_seg, loss_weight_seg) of k hot terms among n = B*H*W pixels: exact integers divided once in float64, rounded to float32"""
    per = BIG if seg_type == "bce" else 1.0  # (1 - t) * 100 against |1 - t|
    return torch.stack([f32(k_noc / (3.0 * n)), f32(per * k_seg / n), f32(per * k_w / (2.0 * n))])


# ---- code loss ------------------------------------------------------------------------------------------------------------------------
BIN_THREADS, BIN_CHUNKS = 1024, 32


def bin_geometry(B, C, HW, vec=None):
    """lc_dense_aux.hip launch_xyz_bin_loss_fwd: grid C x chunks.  Vectorised walk (H*W % 4 == 0): a unit is one slab of 1024 requests of
    four pixels of ONE sample's plane, units dealt to the channel's chunks round robin; element-wise walk: flat over (sample, pixel), 1024
    pixels per workgroup and trip.  -> (vec, slabs per plane, units, chunks)"""
    vec = HW % 4 == 0 if vec is None else vec
    slabs = _ceil_div(HW // 4, BIN_THREADS) if vec else 0
    units = B * slabs if vec else _ceil_div(_ceil_div(B * HW, 4), 4 * BIN_THREADS)
    chunks = min(BIN_CHUNKS, max(1, units))
    chunks = min(chunks, max(1, 512 // C))
    return vec, slabs, units, chunks


def bin_pixels(B, C, HW):
    """vectorised walk: pixel indices inside a plane -- thread t of the workgroup takes request slab * 1024 + t"""
    p = Positions(HW)
    p.add("first", 0)
    p.add("last", HW - 1)
    p.edge("group", 4)
    p.add("lane1", 1)
    p.add("lane2", 2)
    p.add("last_request", 4 * (HW // 4 - 1))
    for k in range(1, _ceil_div(HW // 4, BIN_THREADS)):
        p.edge(f"slab{k}", 4 * k * BIN_THREADS)
    p.edge("wave", 4 * 64)
    return p


def bin_samples(B, C, HW):
    _, _, _, chunks = bin_geometry(B, C, HW)
    return sorted({b for b in (0, 1, chunks - 1, chunks, B - 1) if 0 <= b < B})


def bin_channels(C):
    return sorted({c for c in (0, 1, C - 1) if 0 <= c < C})


def bin_positions(B, C, HW):
    """(sample, pixel) pairs: the vectorised walk's samples x plane positions, or the element-wise walk's flat edges (a workgroup's trips of
    1024 pixels, chunks * 1024 apart; the sample edges)"""
    vec, _, _, chunks = bin_geometry(B, C, HW)
    if vec:
        return [(b, px) for b in bin_samples(B, C, HW) for px in bin_pixels(B, C, HW).pick()]
    n = B * HW
    p = Positions(n)
    p.add("first", 0)
    p.add("last", n - 1)
    for b in sorted({1, B - 1}):
        p.edge(f"sample{b}", b * HW)
    for k in range(1, _ceil_div(n, BIN_THREADS) + 1):
        p.edge(f"trip{k}", k * BIN_THREADS)
    p.edge("wave", 64)
    return [divmod(i, HW) for i in p.pick()]


def bin_inputs(B, C, H, W, err_hot=None, invis_hot=None, dtype=torch.float32, device="cpu"):
    """logits +100 everywhere, ground-truth bit 1 (hot error: 0), visibility logit +1 (hot invisible: -1) -> (logits, bits (uint8), vis_logits (B,1,H,W))"""
    logits = torch.full((B, C, H, W), BIG, dtype=dtype, device=device)
    bits = torch.ones(B, C, H, W, dtype=torch.uint8, device=device) if err_hot is None else (~err_hot.to(device)).to(torch.uint8)
    vis = torch.ones(B, 1, H, W, dtype=dtype, device=device)
    if invis_hot is not None:
        vis = torch.where(invis_hot.to(device)[:, None], -vis, vis)
    return logits, bits, vis


def bin_counts(B, C, H, W, err_hot=None, invis_hot=None):
    """-> int64 (C + 1,): the per-bit Hamming errors inside the visibility mask, then the visible pixels"""
    dev = (err_hot if err_hot is not None else invis_hot).device if (err_hot is not None or invis_hot is not None) else "cpu"
    visible = torch.ones(B, H, W, dtype=torch.bool, device=dev) if invis_hot is None else ~invis_hot
    err = torch.zeros(B, C, H, W, dtype=torch.bool, device=dev) if err_hot is None else err_hot
    return torch.cat(((err & visible[:, None]).sum([0, 2, 3]), visible.sum().reshape(1)))


def bin_bce_mean(counts, n):
    """per-bit BCE means with every pixel visible: each error costs (1 - 0) * 100 exactly"""
    return f32(BIG * counts[:-1].double().cpu() / n)


def bin_histogram_step(counts, momentum, start=0.5):
    """the reference's losses.py:205-208 (restated at bin_loss_finish) in float32 and in its operation order, on exact integer counts"""
    counts = counts.cpu()
    hist = counts[:-1] / (counts[-1] + 1)  # integer tensors divide as float32
    h = torch.full((counts.numel() - 1,), start, dtype=torch.float32)
    h.mul_(1 - momentum).add_(hist * momentum)
    return h


# ---- log-sum-exp ----------------------------------------------------------------------------------------------------------------------
LSE_THREADS = 512


def lse_positions(n, ahead=(4, 8)):
    """lc_dense_lse.h lse_share_loop over the n = 2*H*W weight logits of one sample: group r (logits 4r .. 4r+3) of n4 = n / 4 belongs to thread
    r % 512, in-flight slot (r / 512) % AHEAD of round r / (512 AHEAD); AHEAD = 4 in block_lse, 8 in the several-workgroups selection,
    whose part g of P plays threads [512 g / P, 512 (g + 1) / P); thread 0 takes the logits behind 4 n4 one by one"""
    n4 = n // 4
    p = Positions(n)
    p.add("first", 0)
    p.add("last", n - 1)
    p.edge("channel", n // 2)
    p.edge("group", 4)
    p.edge("tail", 4 * n4)
    for e in range(4 * n4, n):
        p.add(f"tail{e - 4 * n4}", e)
    p.add("last_group", 4 * (n4 - 1))
    for u in range(1, _ceil_div(n4, LSE_THREADS) + 1):  # slot edges; multiples of AHEAD: round edges
        p.edge(f"slot{u}", 4 * u * LSE_THREADS)
    p.edge("wave", 4 * 64)
    for parts in (2, 4, 8):
        p.edge(f"part{parts}", 4 * (LSE_THREADS // parts))
    p.add("lane1", 1)
    p.add("lane2", 2)
    return p


def lse_inputs(B, H, W, spikes=None, dtype=torch.float32, device="cpu"):
    """weight logits 0 everywhere (uniform), +20 at flat index spikes[b] of sample b's (2,H,W) logits"""
    wl = torch.zeros(B, 2, H, W, dtype=dtype, device=device)
    if spikes is not None:
        wl.view(B, -1)[torch.arange(B, device=device), torch.as_tensor(spikes, device=device)] = SPIKE
    return wl


# ---- what a lost or doubled request does to a probed output ----------------------------------------------------------------------------
def bite(n, allowance_ulp):
    """One request of four elements lost or counted twice, against the allowance of the check (in float32 ulp, 2^-23 relative at worst):
    one-hot -- the request holding the hot element: the output goes to 0 or doubles (relative change 1); random-hot -- the request's
    two hot elements of about n / 2: 4 / n of the output.  -> (one-hot change, random-hot change, allowance) as relative figures"""
    return 1.0, 4.0 / n, allowance_ulp * 2.0 ** -23


# ---- the shapes both test files run ----------------------------------------------------------------------------------------------------
def sq_sizes():
    """Element counts for the sum of squares.  stride = grid * 256 requests; a grid of g workgroups holds n in (8192 (g - 1), 8192 g], so
    n / 4 lies in (8 (g - 1) / g, 8] strides: the slot edges that exist AT grid 2 are 5 .. 8 strides (8: the round edge and the step to grid 3),
    at grid 7 they are 7 and 8 strides.  4 stride +- 1 and 16 stride +- {0, 1, 3} for g = 2, 7 are run as well (the launcher gives them a
    smaller grid, where they are the first slot's and the first round's edges)."""
    s = [1, 3, 4, 5, 6, 8191, 8192, 8193]
    for g in (2, 7):
        stride = g * SQ_THREADS
        s += [4 * stride - 1, 4 * stride + 1] + [16 * stride + d for d in (-3, -1, 0, 1, 3)]
        for k in range(8 * (g - 1) // g + 1, 9):
            s += [4 * k * stride + d for d in (-3, -1, 0, 1, 2, 3)]
    s += [512 * 8192 - 4, 512 * 8192, 512 * 8192 + 8197, 512 * 8192 + 8198, 512 * 8192 + 8199]  # the cap: 512 workgroups, two full rounds, then a third
    return sorted(set(s))


AUX_SHAPES = [(3, 17, 23), (5, 32, 32), (17, 128, 128), (65, 128, 128), (3, 301, 301)]
BIN_SHAPES = [(3, 2, 72, 72), (40, 2, 64, 64), (5, 72, 40, 36), (2, 128, 16, 16), (3, 21, 37, 29)]
BIN_TRAINING_SHAPE = (32, 21, 128, 128)
LSE_SHAPES = [(2, 64, 64, 2), (1, 128, 128, 3), (2, 30, 50, 3), (4, 9, 7, 1), (2, 45, 47, 1)]
