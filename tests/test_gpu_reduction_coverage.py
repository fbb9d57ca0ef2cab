"""Which elements the streaming reductions sum, element by element: lc_sqnorm_kernel, lc_dense_aux_fwd_kernel, lc_xyz_bin_loss_fwd_kernel and
block_lse / lse_thread_share on the exact probes of tests/reduction_probes.py (proven against the float64 torch formulas in
tests/test_reduction_probes.py).  An element dropped or counted twice at a vector-group, in-flight-slot, round, workgroup, grid-wrap, sample,
slab or tail edge, or a partial sum the last arriver misses, changes an integer that must come out exactly (sum of squares, Hamming and
visibility counts) or a float32 that must come out within 1 ulp (the means) -- not a mean of a random map by 4 / n of itself.

Every one-hot sweep reuses one device buffer (set the element, launch, keep the device scalar, clear the element) and reads all results back
at the end of the test."""
import pytest
import torch

from tests import reduction_probes as rp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _report(labels, bad):
    return [labels[i] for i in torch.nonzero(bad).flatten().tolist()[:12]]


# ---- 1. sum of squares ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_sum_of_squares_counts_every_element_exactly_once(dt):
    """`_launch_sqnorm` on a NormClipper's own workspace: all-hot, random-hot and one-hot sweeps at every size of `rp.sq_sizes()`, from an
    aligned view and from a view one element off (the scalar walk), as a list of three tensors, and once more after each size (the ticket is
    back at zero): `sq` is the integer, exactly."""
    from lc_amd.grad import NormClipper, _launch_sqnorm

    dtype = DTYPES[dt]
    clip = NormClipper().to(DEV)
    ws, state = clip._ws(DEV), clip.max_norm
    sizes = rp.sq_sizes()
    buf = torch.zeros(max(sizes) + 1, dtype=dtype, device=DEV)
    extra5, (extra_r, k_r) = torch.ones(5, dtype=dtype, device=DEV), rp.sq_pattern(8193, ("random", 5), dtype, DEV)
    got, want, labels, dev_want = [], [], [], {}

    def run(xs, expect, label):
        got.append(_launch_sqnorm(xs, ws, state)[0])
        if isinstance(expect, torch.Tensor):
            dev_want[len(want)] = expect
            expect = -1
        want.append(expect)
        labels.append(label)

    for n in sizes:
        assert n + 8193 + 5 < 2 ** 24
        m = rp.random_hot((n,), n, DEV)
        k = m.sum()
        for off in (0, 1):
            x = buf[off:off + n]
            x.fill_(1)
            run([x], n, (n, off, "all-hot"))
            run([extra5, x, extra_r], n + 5 + k_r, (n, off, "list of three"))
            x.copy_(m)
            run([x], k, (n, off, "random-hot"))
            run([extra_r, x, extra5], k + (5 + k_r), (n, off, "list of three, random-hot"))
            x.zero_()
            for i in rp.sqnorm_positions(n, vec=off == 0).pick(48):
                x[i:i + 1].fill_(rp.HOT_SQ)
                run([x], 9, (n, off, "one-hot", i))
                x[i:i + 1].zero_()
            x.fill_(1)
            run([x], n, (n, off, "all-hot again"))
            x.zero_()
    res = torch.stack(got).double().cpu()
    exp = torch.tensor(want, dtype=torch.float64)
    if dev_want:
        exp[list(dev_want)] = torch.stack(list(dev_want.values())).double().cpu()
    assert ws[1].item() == 0
    assert torch.equal(res, exp), _report([(l, float(a), float(b)) for l, a, b in zip(labels, res, exp)], res != exp)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", [8193, 512 * 8192 + 8197])
def test_clip_apply_scales_every_element_by_exactly_a_quarter(n, dt):
    """Small integers of squared norm exactly 4096 under initial_max_norm = 16: the norm is 64, 64 + 1e-6 rounds to 64 in fp32 and 16 / 64 is
    exact, so the clipped gradient is x / 4 bit for bit at every element."""
    from lc_amd.grad import NormClipper

    dtype = DTYPES[dt]
    twos = rp.sqnorm_positions(n).pick()
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g)
    ones = perm[~torch.isin(perm, torch.tensor(twos))][:4096 - 4 * len(twos)]
    x = torch.zeros(n)
    x[twos] = 2.0
    x[ones] = 1.0
    x[::2] *= -1
    assert float(x.double().square().sum()) == 4096.0
    x = x.to(DEV, dtype)
    clip = NormClipper(initial_max_norm=16).to(DEV)
    out = clip.clip(x)
    assert out.dtype == dtype and torch.equal(out, x * 0.25) and float(clip.last_norm) == 64.0


# ---- 2. dense auxiliary losses --------------------------------------------------------------------------------------------------------
def _aux_launch(t, mask, with_xyz, with_w, seg_type):
    from lc_amd.dense_aux import dense_aux_losses

    with torch.no_grad():
        return torch.stack(dense_aux_losses(t["xyz"] if with_xyz else None, mask if with_xyz else None, t["tgt"] if with_xyz else None, t["seg"], t["vis"],
                                            t["wl"] if with_w else None, seg_type))


def _mask_as(m, mask_dtype):
    return m if mask_dtype == torch.bool else m.to(mask_dtype)


def _check_aux(got, want, labels, n, seg_type):
    res = torch.stack(got).cpu()
    exp = torch.stack([rp.aux_expected(*k, n, seg_type) for k in want])
    ulp = rp.ulps_apart(res, exp)
    bad = (ulp > 1).any(-1)
    assert not bool(bad.any()), _report([(l, a.tolist(), b.tolist()) for l, a, b in zip(labels, res, exp)], bad)


AUX_CASES = [(B, H, W, dt) for B, H, W in rp.AUX_SHAPES for dt in DTYPES if dt == "f32" or (B, H, W) in ((5, 32, 32), (17, 128, 128))]


@pytest.mark.parametrize("seg_type", ["bce", "l1"])
@pytest.mark.parametrize("B,H,W,dt", AUX_CASES)
def test_dense_aux_losses_count_every_pixel_exactly_once(B, H, W, dt, seg_type):
    """`dense_aux_losses` with bool / uint8 / float32 masks, with and without the coordinate head and the weight logits: all-hot, random-hot
    and one-hot sweeps over `rp.aux_positions`; each loss within 1 ulp of float32(exact count / n)."""
    dtype, n, HW = DTYPES[dt], B * H * W, H * W
    kw = dict(dtype=dtype, device=DEV)
    full = dict(vis_hot=torch.ones(B, H, W, dtype=torch.bool), x_hot=torch.ones(B, 3, H, W, dtype=torch.bool))
    full2 = dict(vis_hot=full["vis_hot"], mask_hot=torch.ones(B, H, W, dtype=torch.bool))
    rnd = dict(vis_hot=rp.random_hot((B, H, W), 1), x_hot=rp.random_hot((B, 3, H, W), 2), w_hot=rp.random_hot((B, 2, H, W), 3))
    rnd2 = dict(mask_hot=rp.random_hot((B, H, W), 4), w_hot=rp.random_hot((B, 2, H, W), 5))
    fixed = [(name, rp.aux_inputs(B, H, W, **case, **kw), rp.aux_counts(B, H, W, **case))
             for name, case in (("all-hot", full), ("all-hot through the mask", full2), ("random-hot", rnd), ("random-hot through the mask", rnd2))]
    cold, cold2 = rp.aux_inputs(B, H, W, **kw), rp.aux_inputs(B, H, W, mask_hot=torch.zeros(B, H, W, dtype=torch.bool), **kw)
    pos = rp.aux_positions(B, HW).pick(32)
    got, want, labels = [], [], []
    for with_xyz, with_w, mask_dtype in [(True, w, m) for w in (True, False) for m in (torch.bool, torch.uint8, torch.float32)] + [(False, True, None), (False, False, None)]:
        cfg = (with_xyz, with_w, mask_dtype)

        def run(t, mask, k, label):
            got.append(_aux_launch(t, mask, with_xyz, with_w, seg_type))
            want.append((k[0] if with_xyz else 0, k[1], k[2] if with_w else 0))
            labels.append((cfg, label))

        for name, t, k in fixed:
            run(t, _mask_as(t["msk_noc"], mask_dtype) if with_xyz else None, k, name)
        # one-hot, first way: msk_vis = 0 at one pixel (hot for the seg logit and both weight logits) and one coordinate of another pixel = 1
        mask = _mask_as(cold["msk_noc"], mask_dtype) if with_xyz else None
        for j, i in enumerate(pos):
            b2, px2 = divmod(pos[(j + 1) % len(pos)], HW)
            v, x = cold["vis"].view(-1)[i:i + 1], cold["xyz"].view(B, 3, HW)[b2, j % 3, px2:px2 + 1]
            v.fill_(0)
            x.fill_(1)
            run(cold, mask, (1, 1, 2), ("one-hot", i, j % 3))
            v.fill_(1)
            x.fill_(0)
        # second way: coordinates 1 everywhere and the mask hot at one pixel (the byte mask, lane by lane); one weight logit alone at -100
        mask = _mask_as(cold2["msk_noc"], mask_dtype) if with_xyz else None
        for j, i in enumerate(pos):
            b, px = divmod(i, HW)
            w = cold2["wl"].view(B, 2, HW)[b, j % 2, px:px + 1]
            w.fill_(-rp.BIG)
            if with_xyz:
                mask.view(-1)[i:i + 1].fill_(1)
            run(cold2, mask, (3, 0, 1), ("one-hot through the mask", i, j % 2))
            w.fill_(rp.BIG)
            if with_xyz:
                mask.view(-1)[i:i + 1].fill_(0)
    _check_aux(got, want, labels, n, seg_type)


@pytest.mark.parametrize("seg_type", ["bce", "l1"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_dense_aux_losses_find_a_pixel_behind_each_sample_edge_of_channel_slices(dt, seg_type):
    """The three heads as channel slices of one (B,9,H,W) tensor (sample strides that are not the dense ones); the channels between them hold
    values that would be hot.  A one-hot at the first and at the last pixel of every sample, in every head, is found, and nothing else is."""
    B, H, W = 5, 32, 32
    HW, n = H * W, B * H * W
    raw = torch.zeros(B, 9, H, W, dtype=DTYPES[dt], device=DEV)
    xyz, wl, seg = raw[:, 0:3], raw[:, 4:6], raw[:, 8:9]
    raw[:, 3] = 1.0
    raw[:, 4:6] = rp.BIG
    raw[:, 6:8] = -rp.BIG
    raw[:, 8] = rp.BIG
    t = dict(xyz=xyz, seg=seg, wl=wl, tgt=torch.zeros(B, 3, H, W, device=DEV), vis=torch.ones(B, H, W, device=DEV))
    mask = torch.ones(B, H, W, dtype=torch.bool, device=DEV)
    got, want, labels = [_aux_launch(t, mask, True, True, seg_type)], [(0, 0, 0)], ["cold"]
    j = 0
    for b in range(B):
        for px in (0, 1, HW - 2, HW - 1):
            cells = (xyz[b, j % 3].view(-1)[px:px + 1], 1.0, 0.0), (wl[b, j % 2].view(-1)[px:px + 1], -rp.BIG, rp.BIG), (seg[b, 0].view(-1)[px:px + 1], -rp.BIG, rp.BIG)
            for cell, hot, _ in cells:
                cell.fill_(hot)
            got.append(_aux_launch(t, mask, True, True, seg_type))
            want.append((1, 1, 1))
            labels.append((b, px, j % 3, j % 2))
            for cell, _, cold in cells:
                cell.fill_(cold)
            j += 1
    _check_aux(got, want, labels, n, seg_type)


# ---- 3. code loss ---------------------------------------------------------------------------------------------------------------------
def _bin_counts_launch(logits, bits, vis):
    """`lc_xyz_bin_loss_counts` as lc_amd/dense_aux.py calls it under a process group (the same workspace arrangement)"""
    from lc_amd import _lib, dense_aux

    lib = _lib.load()
    B, C = logits.shape[:2]
    HW = logits.numel() // (B * C)
    (x, v), (ls, vs), code = _lib.hip_maps(xyz_noc_bin=logits, msk_vis_logits=vis.reshape(B, HW))
    counts = torch.empty(C + 1, device=DEV, dtype=torch.int64)
    bce_mean = torch.empty(C, device=DEV, dtype=torch.float32)
    partials, ticket = dense_aux._workspace(DEV)
    P = _lib.ptr
    rc = lib.lc_xyz_bin_loss_counts(P(x), P(bits), P(v), code, ls, vs, B, C, HW, P(counts), P(bce_mean), P(partials), P(ticket), _lib.stream_ptr(DEV))
    _lib.check(rc, "lc_xyz_bin_loss_counts")
    return counts, bce_mean


class _BinRuns:
    def __init__(self, B, C, H, W):
        from lc_amd.losses import Loss_xyz_bin

        self.n, self.C = B * H * W, C
        self.fn = Loss_xyz_bin(C).to(DEV)
        self.counts, self.bce, self.hist, self.want, self.all_visible, self.labels = [], [], [], [], [], []

    def run(self, logits, bits, vis, want, label):
        """want: the exact (C + 1,) int64 counts, on any device"""
        c, m = _bin_counts_launch(logits, bits, vis)
        self.counts.append(c)
        self.bce.append(m)
        self.fn.histogram.fill_(0.5)
        with torch.no_grad():
            self.fn(logits, bits, vis)  # the one-launch form from a fresh histogram
        self.hist.append(self.fn.histogram.clone())
        self.want.append(want.to(DEV))
        self.labels.append(label)

    def check(self):
        got, want = torch.stack(self.counts).cpu(), torch.stack(self.want).cpu()
        bad = (got != want).any(-1)
        assert got.dtype == torch.int64 and not bool(bad.any()), _report([(l, a.tolist(), b.tolist()) for l, a, b in zip(self.labels, got, want)], bad)
        bce, hist = torch.stack(self.bce).cpu(), torch.stack(self.hist).cpu()
        visible = want[:, -1] == self.n
        exp = torch.stack([rp.bin_bce_mean(w, self.n) for w in want])
        bad = (rp.ulps_apart(bce, exp) > 1).any(-1) & visible
        assert bool(visible.any()) and not bool(bad.any()), _report([(l, a.tolist(), b.tolist()) for l, a, b in zip(self.labels, bce, exp)], bad)
        exp = torch.stack([rp.bin_histogram_step(w, self.fn.momentum) for w in want])
        bad = (rp.ulps_apart(hist, exp) > 1).any(-1)
        assert not bool(bad.any()), _report([(l, a.tolist(), b.tolist()) for l, a, b in zip(self.labels, hist, exp)], bad)


BIN_CASES = [(*s, dt) for s in rp.BIN_SHAPES for dt in DTYPES if dt == "f32" or s in rp.BIN_SHAPES[:2]]


@pytest.mark.parametrize("B,C,H,W,dt", BIN_CASES)
def test_code_loss_counts_every_pixel_of_every_plane_exactly_once(B, C, H, W, dt):
    """Counts form (`lc_xyz_bin_loss_counts`) and one-launch form (`Loss_xyz_bin`, fresh histogram): the C Hamming counts and the visible count
    equal torch's integer sums, the per-bit BCE means are within 1 ulp of float32(100 k_c / n) when every pixel is visible, and the histogram
    after one step is within 1 ulp of the float32 update on the exact counts."""
    dtype, n, HW = DTYPES[dt], B * H * W, H * W
    r = _BinRuns(B, C, H, W)
    full = torch.ones(B, C, H, W, dtype=torch.bool, device=DEV)
    err, inv = rp.random_hot((B, C, H, W), 6, DEV), rp.random_hot((B, H, W), 8, DEV)
    for label, case in (("all-hot", dict(err_hot=full)), ("all-hot, second launch", dict(err_hot=full)), ("random errors", dict(err_hot=err)),
                        ("random visibility", dict(err_hot=full, invis_hot=inv)), ("random errors and visibility", dict(err_hot=err, invis_hot=inv)),
                        ("nothing visible", dict(err_hot=full, invis_hot=torch.ones(B, H, W, dtype=torch.bool, device=DEV))), ("cold", dict())):
        logits, bits, vis = rp.bin_inputs(B, C, H, W, **case, dtype=dtype, device=DEV)
        # torch's own integer sums (Loss_xyz_bin's count lines) on the tensors the kernel reads
        hard = vis > 0
        want = torch.cat(((logits > 0).logical_xor(bits.bool()).logical_and(hard).sum([0, 2, 3]), hard.sum().reshape(1)))
        assert torch.equal(want, rp.bin_counts(B, C, H, W, **case).to(DEV)) if case else int(want.sum()) == n
        r.run(logits, bits, vis, want, label)
    positions = rp.bin_positions(B, C, HW)
    logits, bits, vis = rp.bin_inputs(B, C, H, W, dtype=dtype, device=DEV)
    base = torch.zeros(C + 1, dtype=torch.int64)
    base[-1] = n
    for c in rp.bin_channels(C):
        want = base.clone()
        want[c] = 1
        for b, px in positions:
            cell = bits.view(B, C, HW)[b, c, px:px + 1]
            cell.fill_(0)
            r.run(logits, bits, vis, want, ("one error", b, c, px))
            cell.fill_(1)
    bits.fill_(0)  # every bit wrong: a pixel that is not visible is missing from every count
    want = torch.full((C + 1,), n - 1, dtype=torch.int64)
    for b, px in positions:
        cell = vis.view(B, HW)[b, px:px + 1]
        cell.fill_(-1)
        r.run(logits, bits, vis, want, ("one invisible pixel", b, px))
        cell.fill_(1)
    r.check()


def test_code_loss_counts_at_the_training_shape():
    B, C, H, W = rp.BIN_TRAINING_SHAPE
    r = _BinRuns(B, C, H, W)
    err, inv = rp.random_hot((B, C, H, W), 6, DEV), rp.random_hot((B, H, W), 8, DEV)
    for label, case in (("all-hot", dict(err_hot=torch.ones(B, C, H, W, dtype=torch.bool, device=DEV))), ("random errors", dict(err_hot=err)),
                        ("random errors and visibility", dict(err_hot=err, invis_hot=inv))):
        logits, bits, vis = rp.bin_inputs(B, C, H, W, **case, device=DEV)
        r.run(logits, bits, vis, rp.bin_counts(B, C, H, W, **case), label)
    r.check()


# ---- 4. log-sum-exp -------------------------------------------------------------------------------------------------------------------
def _per_sample_rel_err(a, b):
    """tests.util.rel_err sample by sample: the largest error of a sample against the sample's own largest entry"""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


def _spike_rounds(B, n):
    pos = rp.lse_positions(n).pick()
    step = max(1, len(pos) // B)
    return [[pos[(k + b * step) % len(pos)] for b in range(B)] for k in range(len(pos))]  # every sample sees every position


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("B,H,W,sample", rp.LSE_SHAPES)
def test_front_end_normaliser_holds_every_logit_exactly_once(B, H, W, sample, dt):
    """`dense_front_end` on weight logits 0 with a +20 spike swept over `rp.lse_positions` (both channels, every sample), and on uniform logits:
    weights against oracle/dense_oracle.py in float64 at test_dense_front_end_vs_oracle's tolerances (2e-6 weights, 1e-6 points), sample by sample."""
    from lc_amd.dense import dense_front_end
    from oracle import dense_oracle

    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(B * H + W)
    xyz = torch.randn(B, 3, H, W, generator=g).to(dtype)
    ws = torch.exp(torch.randn(B, 1, 1, 1, generator=g) * 0.3 + 3)
    ns = torch.rand(B, 3, generator=g) * 40 + 10
    d_xyz, d_ws, d_ns = xyz.to(DEV), ws.to(DEV), ns.to(DEV)
    wl = rp.lse_inputs(B, H, W, None, dtype, DEV)
    flat, rows = wl.view(B, -1), torch.arange(B, device=DEV)
    rounds = [None] + _spike_rounds(B, 2 * H * W)
    got = []
    for spikes in rounds:
        if spikes is not None:
            flat[rows, torch.tensor(spikes, device=DEV)] = rp.SPIKE
        with torch.no_grad():
            p2, s, p3 = dense_front_end(d_xyz, wl, d_ws, d_ns, sample=sample, top_left=(0, 0))
        got.append((s, p3))
        if spikes is not None:
            flat[rows, torch.tensor(spikes, device=DEV)] = 0
    torch.cuda.synchronize()
    for spikes, (s, p3) in zip(rounds, got):
        _, r, q3 = dense_oracle.dense_front_end(xyz.double(), rp.lse_inputs(B, H, W, spikes, torch.float64), ws.double(), ns.double(), sample, (0, 0))
        assert _per_sample_rel_err(s.cpu(), r) <= 2e-6 and _per_sample_rel_err(p3.cpu(), q3) <= 1e-6, (spikes, _per_sample_rel_err(s.cpu(), r))


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("B,H,W,sample,top_left", [(3, 65, 64, 1, (0, 0)), (64, 96, 100, 1, (0, 0)), (100, 90, 90, 1, (0, 0)), (5, 200, 160, 2, (1, 0))])
def test_selection_kernels_normalise_the_spike_inputs_alike(B, H, W, sample, top_left, dt):
    """The same spike inputs through `lc_dense_frontend_select3` without a workspace (block_lse, four requests in flight) and with one (several
    workgroups per object: lse_thread_share<512, 8>, each part its own threads of the reduction) at rows of more than 4096 candidates: rows,
    weights, indices and counts bit for bit as each other, the weights at 2e-6 of the float64 oracle, sample by sample."""
    from lc_amd.dense import dense_front_end_select
    from oracle import dense_oracle

    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(B * H + W)
    ws = torch.rand(B, generator=g) + 0.5
    d_ws = ws.to(DEV)
    vl = torch.full((B, 1, H, W), 9.0, dtype=dtype, device=DEV)
    wl = rp.lse_inputs(B, H, W, None, dtype, DEV)
    flat, rows = wl.view(B, -1), torch.arange(B, device=DEV)
    kw = dict(seg_thresh=0.5, sample=sample, top_left=top_left, quantile=0.0, square_weights=False, min_count=4, seed=3)
    same = torch.ones((), dtype=torch.bool, device=DEV)
    worst = torch.zeros((), dtype=torch.float64, device=DEV)
    kept = []
    for spikes in [None] + _spike_rounds(B, 2 * H * W)[::3]:
        if spikes is not None:
            flat[rows, torch.tensor(spikes, device=DEV)] = rp.SPIKE
        one = dense_front_end_select(None, wl, d_ws, None, vl, "quantile", split=False, **kw)
        many = dense_front_end_select(None, wl, d_ws, None, vl, "quantile", split=True, **kw)
        _, r, _ = dense_oracle.dense_front_end(None, rp.lse_inputs(B, H, W, spikes, torch.float64), ws.double(), None, sample, top_left)
        N = one[1].shape[1]
        cnt = one[3]
        live = torch.arange(N, device=DEV)[None, :] < cnt[:, None]
        same &= torch.equal(many[3], cnt) & torch.equal(many[4][live], one[4][live]) & torch.equal(many[1][live], one[1][live]) & torch.equal(many[0][live], one[0][live])
        ref = r.to(DEV).gather(1, one[4].long().clamp(0, N - 1)[..., None].expand(-1, -1, 2))
        err = ((one[1].double() - ref).abs() * live[..., None]).flatten(1).amax(1) / (ref.abs() * live[..., None]).flatten(1).amax(1)
        worst = torch.maximum(worst, err.max())
        kept.append(cnt.min())
        if spikes is not None:
            flat[rows, torch.tensor(spikes, device=DEV)] = 0
    assert bool(same) and int(torch.stack(kept).min()) > 0 and float(worst) <= 2e-6, (bool(same), float(worst))
