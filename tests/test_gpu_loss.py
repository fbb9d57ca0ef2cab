"""GPU parity of the fused LC-loss kernel (through the C ABI) against the oracle and the reference's golden vectors.

Tolerances: loss <= 1e-4 abs (relative to max(1,|loss|)), gradients <= 1e-3 rel-max -- the reference's
own fp32 path drifts 4.5e-5 / 7e-5 from its fp64 path; the kernel computes in fp64 internally and is compared with the
fp64 goldens at a tighter bound and with the fp32 goldens at the stated one.
"""
import numpy as np
import pytest
import torch

from tests import rowwise as rw
from tests.util import golden_files, case_name, load_loss_case, rel_err

pytestmark = pytest.mark.gpu
FILES = golden_files("lc_loss_")

# ROW-WISE TOLERANCE (tests/rowwise.py; every `_rowwise` call below): each point's gradient against the fp64 oracle on the identical inputs,
# max|kernel - fp64| over the point / max(the point's largest |fp64| entry, 1e-3 x its sample's largest), must not exceed
# max(2 x the same measure of the fp32 reference at that point, 4 x 2^-24); the loss and H^-1 likewise per sample.  The fp32 reference is the
# unmodified reference's own fp32 run where a fixture stores it (`f32_*`: it ran on these very fp32 inputs) and the oracle evaluated in
# torch.float32 elsewhere.  The kernel's own output never enters a bound.
SHAPES = [(1, 3, 0), (7, 5, 1), (3, 64, 2), (2, 65, 3), (2, 200, 4), (3, 255, 8), (16, 256, 9), (2, 257, 5), (1, 1849, 6), (33, 100, 7)]
COV2D_SHAPES = [(2, 257, 20), (3, 1024, 21), (2, 1849, 22)]
OUTLIER_SHAPES = [(8, 64, 30), (4, 1024, 31)]
CENSUS_MIN_POINTS = 64  # below this a sample has too few points for a stable share of small gradients (1 x 3 and 7 x 5 stay as edge shapes)


def fixture_has_fp32_reference(path):
    """False for the noise-free fixture: its fp64 gradients are exact zeros where its fp32 run is round-off noise (tests/test_rowwise.py)."""
    return "noisefree" not in path


def shape_inputs(B, N, seed, batch_seed=None, outlier_frac=0.05, camera="rot"):
    """CPU inputs of the shape tests: synth.make_batch, a seeded valid mask (about a fifth of the points out) and the narrow cotangent
    `rand + 0.5` every loss test has used so far.  `camera`: synth.CAMERAS (tests/test_gpu_cameras.py)."""
    from lc_amd import synth

    b = synth.make_batch(B, N, seed=seed if batch_seed is None else batch_seed, outlier_frac=outlier_frac, camera=camera)
    g = torch.Generator().manual_seed(seed)
    valid = (torch.rand(B, N, generator=g) > 0.2).float()
    valid[:, :3] = 1
    go = torch.rand(B, generator=g) + 0.5
    return dict(b, valid=valid, grad_out=go)


def wide_grad_out(B, seed):
    """A cotangent spread over six decades, 10^U(-3, 3): samples whose whole gradient is small sit in the same launch as large ones."""
    return 10 ** (torch.rand(B, generator=torch.Generator().manual_seed(7000 + seed)) * 6 - 3)


def oracle_run(ins, dtype, want3=True, **kwargs):
    """(loss, du, ds, dx) of the oracle evaluated in `dtype` on the (fp32-representable) inputs."""
    from oracle import lc_loss_oracle as orc

    i = {k: v.to(dtype) for k, v in ins.items()}
    return orc.loss_and_grads(i["K"], i["pose"], i["pts3d"], i["pts2d"], i["inv_std"], i.get("valid"), i["bbox_3d"], grad_out=i["grad_out"],
                              want_pts3d=want3, **kwargs)


def _rowwise(what, got, ref64, ref32, where=None, samples=False, floor_only=False):
    """got / ref64 / ref32: (loss, du, ds, dx); dx may be None.  Gradients point by point, with `samples` also sample by sample; the loss
    per sample.  floor_only: the fp32 reference has no stable value (noise-free fixture), only 4 x 2^-24 is allowed."""
    for name, g, r64, r32 in zip(("du", "ds", "dx"), got[1:], ref64[1:], ref32[1:]):
        if r64 is None:
            continue
        g, r64, r32 = g.cpu(), r64.cpu(), (r64.cpu() if floor_only else r32.cpu())
        rw.check(f"{what} {name} per point", g, r64, r32, point_dims=1, where=where)
        if samples:
            rw.check(f"{what} {name} per sample", g, r64, r32)
    if where is None:
        r32l = ref64[0] if floor_only else ref32[0]
        rw.check(f"{what} loss per sample", got[0].cpu()[:, None], ref64[0].cpu()[:, None], r32l.cpu()[:, None])


def census(ref_du):
    """The condition that makes a point-wise check say more than `rel_err`: the share of points whose d_pts2d is below 1 % of the batch's
    largest entry."""
    return (rw.batch_share(ref_du) < 1e-2).double().mean().item()


def _run(ins, kwargs, want3, use_autograd=True):
    from lc_amd.cov_mixed import Loss_cov_mixed, loss_cov_mixed_fused

    dev = torch.device("cuda:0")
    d = {k: v.to(dev) for k, v in ins.items()}
    if use_autograd:
        u = d["pts2d"].clone().requires_grad_(True)
        s = d["inv_std"].clone().requires_grad_(True)
        X = d["pts3d"].clone().requires_grad_(want3)
        loss = Loss_cov_mixed(d["K"], d["pose"], X, u, s, d.get("valid"), bbox_3d=d["bbox_3d"], **kwargs)
        gs = torch.autograd.grad(loss, [u, s] + ([X] if want3 else []), d["grad_out"])
        return loss.detach().cpu(), gs[0].cpu(), gs[1].cpu(), (gs[2].cpu() if want3 else None), None
    loss, du, ds, dx, aux = loss_cov_mixed_fused(d["K"], d["pose"], d["pts3d"], d["pts2d"], d["inv_std"], d.get("valid"),
                                                 d["bbox_3d"], grad_out=d["grad_out"], want_pts3d=want3, want_aux=True, **kwargs)
    return loss.cpu(), du.cpu(), ds.cpu(), (dx.cpu() if want3 else None), aux.cpu()


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "lc_loss_") for p in FILES])
@pytest.mark.parametrize("autograd", [True, False], ids=["autograd", "fused"])
def test_loss_kernel_vs_golden(path, autograd):
    from oracle import lc_loss_oracle as orc

    z, ins, kwargs, want3 = load_loss_case(path, torch.float32)
    loss, gu, gs, gx, aux = _run(ins, kwargs, want3, autograd)
    # (1) oracle in fp64 on the IDENTICAL (fp32-representable) inputs: isolates the kernel's own arithmetic
    i64 = {k: v.double() for k, v in ins.items()}
    rl, ru, rs, rx = orc.loss_and_grads(i64["K"], i64["pose"], i64["pts3d"], i64["pts2d"], i64["inv_std"], i64.get("valid"),
                                        i64["bbox_3d"], grad_out=i64["grad_out"], want_pts3d=want3, **kwargs)
    assert ((loss.double() - rl).abs() / rl.abs().clamp_min(1)).max().item() <= 1e-5
    assert rel_err(gu, ru) <= 1e-4 and rel_err(gs, rs) <= 1e-4
    if want3:
        assert rel_err(gx, rx) <= 1e-4
    # (1b) the same comparison row-wise, the bound from the reference's own fp32 run on these inputs.  The noise-free case has no such run to
    # speak of (81 % of its fp64 gradient points are exact zeros that are noise in fp32, tests/test_rowwise.py): the floor alone is allowed.
    f32 = tuple(None if (k == "g_pts3d" and not want3) else torch.from_numpy(z["f32_" + k]) for k in ("loss", "g_pts2d", "g_inv_std", "g_pts3d"))
    _rowwise(case_name(path, "lc_loss_"), (loss, gu, gs, gx), (rl, ru, rs, rx), f32, floor_only=not fixture_has_fp32_reference(path))
    # (2) the reference's own outputs.  The noise-free case is excluded here: with err == 0 the fp64 reference sits on
    # exact zeros (c = w = 0 -> SPD fallback) that do not survive rounding the inputs to fp32, and the fp32 reference's
    # err is pure round-off noise -- there is no stable value to compare with (the oracle check above covers it).
    golden_tols = () if "noisefree" in path else (("f64", 3e-5, 3e-4), ("f32", 1e-4, 1e-3))
    for tag, tl, tg in golden_tols:
        ref = torch.from_numpy(z[f"{tag}_loss"]).double()
        assert ((loss.double() - ref).abs() / ref.abs().clamp_min(1)).max().item() <= tl, tag
        assert rel_err(gu, z[f"{tag}_g_pts2d"]) <= tg, tag
        assert rel_err(gs, z[f"{tag}_g_inv_std"]) <= tg, tag
        if want3:
            assert rel_err(gx, z[f"{tag}_g_pts3d"]) <= tg, tag
    if aux is not None and "f64_Hinv" in z.files and golden_tols:
        Hinv = aux[:, 4:].reshape(-1, 6, 6).double()
        assert rel_err(Hinv, z["f64_Hinv"]) <= 1e-4
    if aux is not None and golden_tols:
        # (the noise-free case stays out as above: its H is round-off noise, its inverse has no stable value)
        # H^-1 per sample under the floor alone, against the oracle's H^-1 on the identical inputs.  The fixture's f64_Hinv was computed on the
        # unrounded fp64 inputs: rounding the inputs to fp32 alone moves H^-1 by up to 4.4e-7 of a sample's largest entry (n3_B3_N3; 2.8e-7 on
        # two samples of metric_B256_N64 -- the oracle in fp64 on both sets of inputs, on the CPU), which is above the floor and above twice
        # the f32_Hinv's own distance on those samples.  The oracle on the identical inputs pins the same quantity without that term.
        _, inter = orc.loss_cov_mixed(i64["K"], i64["pose"], i64["pts3d"], i64["pts2d"], i64["inv_std"], i64.get("valid"), bbox_3d=i64["bbox_3d"],
                                      return_intermediates=True, **kwargs)
        Hk, Ho = aux[:, 4:].reshape(-1, 6, 6), inter["Hinv"]
        rw.check(case_name(path, "lc_loss_") + " Hinv per sample vs oracle", Hk, Ho, Ho, bound=rw.FLOOR)


@pytest.mark.parametrize("B,N,seed", SHAPES)
def test_loss_kernel_vs_oracle_shapes(B, N, seed):
    """Ragged / odd sizes through both kernel variants (registers: N<=256, block-stride: N>256), with a valid mask.  255 / 256 / 257 sit on
    the switch between the two (`lc_loss.hip`: one workgroup with four points per lane up to N = 256, tiles beyond); B=16, N=256 is
    BASELINE configs[0]'s loss shape (16 crops, 32x32 maps, stride 2).  Row-wise (module comment) twice: with the narrow cotangent and with
    one spread over six decades, then also sample by sample so that the small-cotangent samples are judged on their own."""
    ins = shape_inputs(B, N, seed)
    loss, gu, gs, gx, _ = _run(ins, {}, True, True)
    rl, ru, rs, rx = oracle_run(ins, torch.float64)
    assert ((loss.double() - rl).abs() / rl.abs().clamp_min(1)).max().item() <= 3e-5
    assert rel_err(gu, ru) <= 3e-4 and rel_err(gs, rs) <= 3e-4 and rel_err(gx, rx) <= 3e-4
    if N >= CENSUS_MIN_POINTS:
        assert census(ru) >= 0.25
    _rowwise(f"{B}x{N}", (loss, gu, gs, gx), (rl, ru, rs, rx), oracle_run(ins, torch.float32))
    wide = dict(ins, grad_out=wide_grad_out(B, seed))
    got = _run(wide, {}, True, True)[:4]
    ref64 = oracle_run(wide, torch.float64)
    if N >= CENSUS_MIN_POINTS:
        assert census(ref64[1]) >= 0.25
    _rowwise(f"{B}x{N} wide grad_out", got, ref64, oracle_run(wide, torch.float32), samples=True)


@pytest.mark.parametrize("B,N,seed", OUTLIER_SHAPES)
def test_loss_kernel_each_side_of_the_robust_thresholds(B, N, seed):
    """30 % outliers (N(0, 20^2) px against N(0, 1)): the clamp of the error at max_err_len, the Huber knee of c at rel_thresh x the mean
    |error| and the knee of the weight at d_s each split the points of the batch.  The sides are counted with the oracle, both must be
    populated, and the row-wise check (module comment) is applied to each side by itself: a branch whose gradients are all small is not
    hidden behind the one whose gradients are large.  A point is on the far side of a knee if either coordinate is; points masked out by
    `valid` count on neither side.  N = 64 takes the one-workgroup form, N = 1024 the tiled one."""
    from oracle import lc_loss_oracle as orc

    ins = shape_inputs(B, N, seed, outlier_frac=0.3)
    i64 = {k: v.double() for k, v in ins.items()}
    _, inter = orc.loss_cov_mixed(i64["K"], i64["pose"], i64["pts3d"], i64["pts2d"], i64["inv_std"], i64["valid"], bbox_3d=i64["bbox_3d"],
                                  return_intermediates=True)
    live = ins["valid"] > 0
    sides = {"clamp": torch.linalg.vector_norm(inter["err"].detach(), dim=-1) + 1e-6 > 32,
             "huber": (inter["e"].detach().abs() > 3 * inter["mean_abs"][:, None, :]).any(-1),
             "weight": (i64["inv_std"] > inter["d_s"]).any(-1)}
    loss, gu, gs, gx, _ = _run(ins, {}, True, True)
    ref64, ref32 = oracle_run(ins, torch.float64), oracle_run(ins, torch.float32)
    assert rel_err(gu, ref64[1]) <= 3e-4 and rel_err(gs, ref64[2]) <= 3e-4 and rel_err(gx, ref64[3]) <= 3e-4
    assert census(ref64[1]) >= 0.25
    _rowwise(f"{B}x{N} outliers", (loss, gu, gs, gx), ref64, ref32, samples=True)
    for name, far in sides.items():
        for side, mask in (("beyond", far & live), ("within", ~far & live)):
            n = int(mask.sum())
            print(f"{B}x{N} {name} {side}: {n} points in {int(mask.any(1).sum())} of {B} samples")
            assert n >= 16 and bool(mask.any(1).all()), (name, side, n)  # both sides, in every sample
            _rowwise(f"{B}x{N} {name} {side}", (loss, gu, gs, gx), ref64, ref32, where=mask)


def test_loss_halves_equal_the_whole_batch():
    """BASELINE size (B=256,N=64) and beyond: size-independent properties of the path.
    (a) per-sample independence: a batch equals the concatenation of its halves, bit for bit;
    (b) the fused cotangent path equals autograd's two-launch path; (c) permutation of the points leaves the loss
    unchanged to rounding; (d) linearity of the gradient in grad_out."""
    from lc_amd import synth
    from lc_amd.cov_mixed import loss_cov_mixed_fused

    dev = torch.device("cuda:0")
    b = {k: v.to(dev) for k, v in synth.make_batch(4096, 64, seed=11).items()}
    args = (b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, b["bbox_3d"])
    loss, du, ds, dx, _ = loss_cov_mixed_fused(*args)
    assert torch.isfinite(loss).all()
    h = 2048
    l1, du1, _, _, _ = loss_cov_mixed_fused(*[a[:h] if a is not None else None for a in args])
    l2, du2, _, _, _ = loss_cov_mixed_fused(*[a[h:] if a is not None else None for a in args])
    assert torch.equal(torch.cat((l1, l2)), loss) and torch.equal(torch.cat((du1, du2)), du)
    go = (torch.rand(4096, generator=torch.Generator().manual_seed(4096)) + 0.5).to(dev)
    _, du_g, ds_g, dx_g, _ = loss_cov_mixed_fused(*args, grad_out=go)
    assert torch.allclose(du_g, du * go[:, None, None], rtol=1e-5, atol=1e-12)
    assert torch.allclose(dx_g, dx * go[:, None, None], rtol=1e-5, atol=1e-12)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(64)).to(dev)
    lp, dup, _, _, _ = loss_cov_mixed_fused(b["K"], b["pose"], b["pts3d"][:, perm], b["pts2d"][:, perm], b["inv_std"][:, perm],
                                            None, b["bbox_3d"])
    assert (lp - loss).abs().max().item() <= 1e-5
    assert rel_err(dup.cpu(), du[:, perm].cpu()) <= 1e-4


def test_loss_rejects_cpu_tensors():
    from lc_amd import synth
    from lc_amd.cov_mixed import Loss_cov_mixed

    b = synth.make_batch(2, 8, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Loss_cov_mixed(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, bbox_3d=b["bbox_3d"])


def test_loss_full_size_properties():
    """Size-independent properties at a size the fp64 oracle would take minutes for (B = 4096, N = 64):
    (a) gradients are linear in the cotangent; (b) a permutation of the points leaves the loss unchanged and permutes the
    gradients (all reductions are over N within a sample, cov_mixed.py:30-36); (c) `valid_factor = ones` is bit-identical to
    `None` (observed on the imported reference); (d) samples are independent: a slice of the batch alone gives
    the same rows bit for bit."""
    from lc_amd import synth
    from lc_amd.cov_mixed import loss_cov_mixed_fused

    dev = torch.device("cuda:0")
    B, N = 4096, 64
    b = {k: v.to(dev) for k, v in synth.make_batch(B, N, seed=123, outlier_frac=0.1).items()}
    go = (torch.rand(B, generator=torch.Generator().manual_seed(B)) + 0.5).to(dev)
    args = (b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"])
    loss, gu, gs, gx, _ = loss_cov_mixed_fused(*args, None, b["bbox_3d"], grad_out=go)
    assert torch.isfinite(loss).all() and torch.isfinite(gu).all() and torch.isfinite(gs).all() and torch.isfinite(gx).all()
    # (a)
    l2, gu2, gs2, gx2, _ = loss_cov_mixed_fused(*args, None, b["bbox_3d"], grad_out=2.5 * go)
    assert torch.equal(l2, loss)
    for a, c in ((gu2, gu), (gs2, gs), (gx2, gx)):
        assert (a - 2.5 * c).abs().max().item() <= 2e-6 * c.abs().max().item()
    # (b)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(dev)
    lp, gup, gsp, gxp, _ = loss_cov_mixed_fused(b["K"], b["pose"], b["pts3d"][:, perm], b["pts2d"][:, perm], b["inv_std"][:, perm], None,
                                               b["bbox_3d"], grad_out=go)
    assert ((lp - loss).abs() / loss.abs().clamp_min(1)).max().item() <= 1e-5
    for a, c in ((gup, gu[:, perm]), (gsp, gs[:, perm]), (gxp, gx[:, perm])):
        assert (a - c).abs().max().item() <= 1e-4 * c.abs().max().item()
    # (c)
    lo, guo, gso, gxo, _ = loss_cov_mixed_fused(*args, torch.ones(B, N, device=dev), b["bbox_3d"], grad_out=go)
    assert torch.equal(lo, loss) and torch.equal(guo, gu) and torch.equal(gso, gs) and torch.equal(gxo, gx)
    # (d)
    sl = slice(1000, 1037)
    ls, gus, gss, gxs, _ = loss_cov_mixed_fused(*(t[sl].contiguous() for t in args), None, b["bbox_3d"][sl].contiguous(), grad_out=go[sl].contiguous())
    assert torch.equal(ls, loss[sl]) and torch.equal(gus, gu[sl]) and torch.equal(gss, gs[sl]) and torch.equal(gxs, gx[sl])


TILED_SHAPES = [(2, 1024, 0), (3, 700, 1), (32, 1024, 2), (5, 1849, 3), (1, 4096, 4), (40, 600, 5),
                (64, 4096, 6), (60, 2048, 7), (70, 1500, 8), (3, 5000, 9), (4, 1025, 10), (2, 1023, 11)]  # 4, 8 and 16 tiles per workgroup; ragged slices; T > 64; a last tile of one point (17 tiles: uneven quarters, two rounds)


@pytest.mark.parametrize("B,N,seed", TILED_SHAPES)
def test_tiled_form_is_bit_identical_to_the_one_workgroup_form(B, N, seed):
    """Dense shapes (N > 256): the 64-point tiles of a sample dealt to several 256-thread workgroups that meet once through the
    workspace, against one 256-thread workgroup per sample.  Both add the per-sample sums in tile order, so every output --
    loss, the three gradients, H^-1 -- is bit-identical; the workspace is left zeroed; a second launch over the same workspace
    and a launch with the sample inside another batch give the same bits again."""
    from lc_amd import _lib, synth
    from lc_amd import cov_mixed as cm

    dev = torch.device("cuda:0")
    b = {k: v.to(dev) for k, v in synth.make_batch(B, N, seed=100 + seed, outlier_frac=0.1).items()}
    g = torch.Generator().manual_seed(seed)
    valid = (torch.rand(B, N, generator=g) > 0.2).float().to(dev) if seed % 2 else None
    go = (torch.rand(B, generator=g) + 0.5).to(dev)
    args = (b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], valid, b["bbox_3d"])
    assert _lib.load().lc_cov_loss_workspace_bytes(B, N) > 0  # (a sample is cut at least three ways: N >= 3 slices x 4 tiles - 3 tiles)
    one = cm.loss_cov_mixed_fused(*args, grad_out=go, want_aux=True, tiled=False)
    til = cm.loss_cov_mixed_fused(*args, grad_out=go, want_aux=True, tiled=True)
    for a, c in zip(one, til):
        assert torch.isfinite(a).all() and torch.equal(a, c)
    ws = cm.tiled_workspace(dev, B, N)
    torch.cuda.synchronize()
    assert int(ws.view(torch.int32)[: 4 + 2 * B].abs().sum().item()) == 0  # ticket, done, time-outs and every sample's counters
    again = cm.loss_cov_mixed_fused(*args, grad_out=go, want_aux=True, tiled=True)
    for a, c in zip(til, again):
        assert torch.equal(a, c)
    # the sample alone (another grid, another ticket order) gives the same rows
    k = B // 2
    solo = cm.loss_cov_mixed_fused(*(None if t is None else t[k:k + 1].contiguous() for t in args), grad_out=go[k:k + 1].contiguous(), want_aux=True)
    for a, c in zip(til, solo):
        assert torch.equal(a[k:k + 1], c)


def test_tiled_form_under_concurrency_and_replay():
    """The hand-off is an arrive-and-wait loop between workgroups: exercise it with more workgroups in flight than the chip holds
    at once (four streams x 240 workgroups, each stream with its own workspace: the tickets keep every sample's workgroups together
    whatever the dispatcher interleaves) and as a replayed hipGraph."""
    from lc_amd import _lib, synth
    from lc_amd import cov_mixed as cm

    dev = torch.device("cuda:0")
    B, N = 30, 2048
    assert _lib.load().lc_cov_loss_workspace_bytes(B, N) > 0 and _lib.load().lc_cov_loss_workspace_bytes(200, N) == 0
    b = {k: v.to(dev) for k, v in synth.make_batch(B, N, seed=9).items()}
    args = (b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, b["bbox_3d"])
    ref = cm.loss_cov_mixed_fused(*args, tiled=False)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    torch.cuda.synchronize()
    outs = []
    for _ in range(6):
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(cm.loss_cov_mixed_fused(*args))
    torch.cuda.synchronize()
    for o in outs:
        assert all(torch.equal(a, c) for a, c in zip(ref[:4], o[:4]))
    for st in streams:
        with torch.cuda.stream(st):
            ws = cm.tiled_workspace(dev, B, N)
        assert int(ws.view(torch.int32)[: 4 + 2 * B].abs().sum().item()) == 0
    small = tuple(None if t is None else t[:, :1024].contiguous() for t in args)
    want = cm.loss_cov_mixed_fused(*small, tiled=False)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        cm.loss_cov_mixed_fused(*small)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = cm.loss_cov_mixed_fused(*small)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(want[:4], got[:4]))


@pytest.mark.parametrize("B,N,seed", COV2D_SHAPES)
def test_cov2d_dense_forms_vs_oracle_and_each_other(B, N, seed):
    """cov_2d (the covariance of the projected points) beyond N = 256: tiled=False forces the workgroup-per-sample loop
    lc_cov_loss_kernel<false, true>; tiled=True takes lc_cov_loss_tiled_kernel<true> where the workspace query is positive (N = 1024 and
    1849: 16 / 29 tiles, cut at least three ways) and the loop form at N = 257 (five tiles).  Both against the fp64 oracle with
    cov_2d, and bit-identical to each other (lc_loss.hip: all forms add a sample's sums in tile order)."""
    from lc_amd import _lib, synth
    from lc_amd import cov_mixed as cm
    from oracle import lc_loss_oracle as orc

    dev = torch.device("cuda:0")
    b = synth.make_batch(B, N, seed=200 + seed, outlier_frac=0.1)
    g = torch.Generator().manual_seed(seed)
    valid = (torch.rand(B, N, generator=g) > 0.2).float()
    valid[:, :3] = 1
    go = torch.rand(B, generator=g) + 0.5
    assert (_lib.load().lc_cov_loss_workspace_bytes(B, N) > 0) == (N > 257)
    d = {k: v.to(dev) for k, v in b.items()}
    args = (d["K"], d["pose"], d["pts3d"], d["pts2d"], d["inv_std"], valid.to(dev), d["bbox_3d"])
    one = cm.loss_cov_mixed_fused(*args, grad_out=go.to(dev), want_aux=True, cov_2d=True, tiled=False)
    til = cm.loss_cov_mixed_fused(*args, grad_out=go.to(dev), want_aux=True, cov_2d=True, tiled=True)
    for a, c in zip(one, til):
        assert torch.isfinite(a).all() and torch.equal(a, c)
    b64 = {k: v.double() for k, v in b.items()}
    rl, ru, rs, rx = orc.loss_and_grads(b64["K"], b64["pose"], b64["pts3d"], b64["pts2d"], b64["inv_std"], valid.double(), b64["bbox_3d"],
                                        grad_out=go.double(), want_pts3d=True, cov_2d=True)
    loss, gu, gs, gx = (t.cpu() for t in one[:4])
    assert ((loss.double() - rl).abs() / rl.abs().clamp_min(1)).max().item() <= 3e-5
    assert rel_err(gu, ru) <= 3e-4 and rel_err(gs, rs) <= 3e-4 and rel_err(gx, rx) <= 3e-4
    # row-wise (module comment), with this cotangent and with one spread over six decades.  cov_2d flattens the gradient sizes within a sample:
    # under the narrow cotangent only 11 % / 35 % / 27 % of the d_pts2d points of these three batches are below 1 % of the batch's largest
    # entry, so the census is asserted on the wide run, where the smaller samples are (55 % and more).
    ins = dict(b, valid=valid, grad_out=go)
    _rowwise(f"cov_2d {B}x{N}", (loss, gu, gs, gx), (rl, ru, rs, rx), oracle_run(ins, torch.float32, cov_2d=True))
    wide = dict(ins, grad_out=wide_grad_out(B, seed))
    got = cm.loss_cov_mixed_fused(*args, grad_out=wide["grad_out"].to(dev), cov_2d=True, tiled=True)[:4]
    ref64 = oracle_run(wide, torch.float64, cov_2d=True)
    assert census(ref64[1]) >= 0.25
    _rowwise(f"cov_2d {B}x{N} wide grad_out", got, ref64, oracle_run(wide, torch.float32, cov_2d=True), samples=True)
