"""The pose-covariance kernel (lc_amd/csrc/posecov/lc_pose_cov.hip) and its Python surface on the MI355X.

Two compiled forms: `lc_pose_cov_kernel<1>` (one wave, N <= 64) and `lc_pose_cov_kernel<4>` (four waves, N > 64); 2D / 3D, the weight forms,
nan_to_num, counts and shared_poses are run-time options of both.  Which test reaches which form:
    <1>: test_kernel_against_the_reference_fixtures (every case but ragged_B4_N300), test_sweep (n <= 64), test_chain (the sparse chain and the
         stride-2 dense chains, N = 16 / 64), test_scaling_the_weights, test_no_torch_copies
    <4>: test_kernel_against_the_reference_fixtures[ragged_B4_N300], test_sweep (n > 64), test_exact_bits, test_chain (stride 1, N = 256)

TOLERANCE (every comparison below): per row, max|kernel - fp64 reference| over the row's cov (var, perr) entries divided by the row's largest
|reference| entry must not exceed  max(2 x the same measure of the fp32 reference against the fp64 reference, 4 x 2^-24).  The fp32 reference is
the unmodified reference's own fp32 run where a fixture stores it; at sizes without a fixture the fp32 evaluation of tests/posecov_oracle.py
stands in for it.  The floor: the kernel sums in fp64 and rounds each output once, so it is a few fp32 roundings of the output.  Where the fp32
reference disagrees with the fp64 one on `info` (its own overflow), only the floor is allowed.
"""
import numpy as np
import pytest
import torch

from tests import posecov_oracle as po
from tests.golden import gen_golden_posecov as gen

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EYE = torch.eye(6)


def _dev(args, kw):
    return [None if a is None else a.to(DEV) for a in args], {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def _check(got, ref64, ref32, rows=None, what=""):
    """`got` (PoseCov on the GPU) against the fp64 reference under the module's tolerance; rows: the rows whose SPD verdict is compared."""
    B = ref64.cov.shape[0]
    rows = torch.ones(B, dtype=torch.bool) if rows is None else torch.as_tensor(rows, dtype=torch.bool)
    gi, ri = got.info.cpu() != 0, ref64.info.cpu() != 0
    assert torch.equal(gi[rows], ri[rows]), (what, got.info.tolist(), ref64.info.tolist())
    assert torch.equal(got.cov.cpu()[gi], EYE.expand(int(gi.sum()), 6, 6)), what  # cov == I exactly on fallback rows
    same = rows & (gi == ri)  # (a rank-deficient row both sides judged alike is compared too)
    agree32 = (ref32.info.cpu() != 0) == ri
    for name, g, r64, r32 in (("cov", got.cov, ref64.cov, ref32.cov), ("var", got.var, ref64.var, ref32.var),
                              ("perr", got.pred_err[:, None], ref64.pred_err[:, None], ref32.pred_err[:, None])):
        err = po.row_error(g.cpu(), r64.cpu())
        own = torch.nan_to_num(po.row_error(r32.cpu(), r64.cpu()), nan=0.0, posinf=0.0)
        bound = torch.where(agree32, 2 * own, torch.zeros(())).clamp_min(po.FLOOR)
        print(f"{what} {name}: err {err[same].max().item() if same.any() else 0:.3e} bound min {bound.min().item():.3e}")
        assert bool((err[same] <= bound[same]).all()), (what, name, err.tolist(), bound.tolist())


@pytest.mark.parametrize("name", po.CASES)
def test_kernel_against_the_reference_fixtures(name):
    """Every fixture of tests/golden/posecov_*.npz: the unmodified reference's fp64 results, its own fp32 results setting the tolerance."""
    from lc_amd.posecov import pose_covariance

    d = po.load_fixture(name)
    args, kw = po.fixture_call(d)
    dargs, dkw = _dev(args, kw)
    got = pose_covariance(*dargs, **dkw)
    t = lambda k: torch.from_numpy(d[k])  # noqa: E731
    ref64 = po.PoseCovRef(t("f64_cov"), t("f64_var"), t("f64_perr"), t("f64_info"))
    ref32 = po.PoseCovRef(t("f32_cov"), t("f32_var"), t("f32_perr"), t("f32_info"))
    _check(got, ref64, ref32, rows=d["well_posed"] | (d["f64_info"] != 0), what=name)
    assert got.cov.dtype == got.var.dtype == got.pred_err.dtype == torch.float32 and got.info.dtype == torch.int32


SWEEP = [1, 3, 6, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 16384]


def _scene(B, N, seed):
    return gen.scene(np.random.default_rng(seed), B, N, skew=True)


@pytest.mark.parametrize("n", SWEEP)
def test_sweep(n):
    """Counts at the tile and width edges, several rows per size, against the fp64 oracle (its fp32 evaluation in the reference's role: these
    sizes have no fixture): 3D with inverse variances and counts inside a wider padded batch, 2D with standard deviations, 3D with one
    scalar per point and shared_poses (K, box and diameter of 2 objects shared by 4 rows; the pose shared too for odd n).  Rows of fewer
    than 6 points are rank-deficient: their SPD verdict is a rounding accident and is not compared (they must still not fault)."""
    from lc_amd.posecov import pose_covariance

    posed = n >= 6
    variants = []
    c = _scene(3, min(n + 70, 16384), 1000 + n)  # padded: the counts decide
    counts = torch.tensor([n, n, max(1, n // 2)], dtype=torch.int32)
    variants.append(("3d-icov-counts", (c["K"], c["pts3d"], c["pts2d"], c["weights"], c["pose"], counts), dict(bbox_3d=c["bbox_3d"], diameter=c["diameter"]),
                     [posed, posed, n // 2 >= 6]))
    c = _scene(3, n, 2000 + n)
    variants.append(("2d-std", (c["K"], c["pts3d"], c["pts2d"], c["weights"].rsqrt(), c["pose"], None), dict(bbox_3d=c["bbox_3d"], cov_2d=True, weights_are_std=True),
                     [posed] * 3))
    c = _scene(4, n, 3000 + n)
    pose = c["pose"][:2] if n % 2 else c["pose"]
    variants.append(("3d-scalar-shared", (c["K"][:2], c["pts3d"], c["pts2d"], c["weights"][..., 0].contiguous(), pose, None),
                     dict(bbox_3d=c["bbox_3d"][:2], diameter=c["diameter"][:2], shared_poses=2), [posed] * 4))
    for what, args, kw, rows in variants:
        dargs, dkw = _dev(args, kw)
        got = pose_covariance(*dargs, **dkw)
        _check(got, po.pose_covariance(*args, **kw), po.pose_covariance(*args, **kw, dtype=torch.float32), rows=rows, what=f"n={n} {what}")
        assert set(got.info.tolist()) <= {0, 1}


def test_exact_bits():
    """NaN-filled padding beyond `counts` gives the bits of zero padding; a row alone gives the bits it has at index 129 of 130 rows; two
    runs agree; a captured and replayed call equals the eager one."""
    from lc_amd.posecov import pose_covariance

    c = _scene(130, 300, 7)
    counts = torch.randint(1, 301, (130,), generator=torch.Generator().manual_seed(3)).to(torch.int32)
    counts[129], counts[0], counts[1] = 257, 300, 64
    (K, X, U, W, pose, cn), kw = _dev((c["K"], c["pts3d"], c["pts2d"], c["weights"], c["pose"], counts), dict(bbox_3d=c["bbox_3d"], diameter=c["diameter"]))
    one = pose_covariance(K, X, U, W, pose, cn, **kw)
    two = pose_covariance(K, X, U, W, pose, cn, **kw)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    pad = torch.arange(300, device=DEV)[None, :] >= cn[:, None]
    Xz, Uz, Wz = (torch.where(pad[..., None], torch.zeros((), device=DEV), t) for t in (X, U, W))
    Xn, Un, Wn = (torch.where(pad[..., None], torch.full((), float("nan"), device=DEV), t) for t in (X, U, W))
    zero, nans = pose_covariance(K, Xz, Uz, Wz, pose, cn, **kw), pose_covariance(K, Xn, Un, Wn, pose, cn, **kw)
    assert all(torch.equal(a, b) for a, b in zip(zero, nans)) and all(torch.equal(a, b) for a, b in zip(zero, one))
    assert not any(torch.isnan(t).any() for t in nans[:3])
    alone = pose_covariance(K[129:], X[129:], U[129:], W[129:], pose[129:], cn[129:], bbox_3d=kw["bbox_3d"][129:], diameter=kw["diameter"][129:])
    assert all(torch.equal(a[0], b[129]) for a, b in zip(alone, one))
    # plain capture and replay on a side stream
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        pose_covariance(K, X, U, W, pose, cn, **kw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = pose_covariance(K, X, U, W, pose, cn, **kw)
    for t in cap:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cap, one))


def test_scaling_the_weights():
    """Sanity of meaning: all inverse variances of a row times 4 -> cov times 1/4, to the tolerance (floor + the two calls' roundings)."""
    from lc_amd.posecov import pose_covariance

    c = _scene(4, 50, 11)
    (K, X, U, W, pose, _), kw = _dev((c["K"], c["pts3d"], c["pts2d"], c["weights"], c["pose"], None), dict(bbox_3d=c["bbox_3d"]))
    a, b = pose_covariance(K, X, U, W, pose, **kw), pose_covariance(K, X, U, 4 * W, pose, **kw)
    assert not a.info.any() and not b.info.any()
    assert bool((po.row_error(4 * b.cov.cpu(), a.cov.cpu()) <= po.FLOOR).all())
    assert bool((po.row_error(2 * b.pred_err.cpu()[:, None], a.pred_err.cpu()[:, None]) <= po.FLOOR).all())


def test_no_torch_copies():
    """No torch copy or cast launch on contiguous fp32 inputs (profiled as tests/test_gpu_map_dtypes.py does)."""
    from torch.profiler import ProfilerActivity, profile

    from lc_amd.posecov import pose_covariance

    c = _scene(4, 50, 12)
    counts = torch.tensor([50, 7, 33, 0], dtype=torch.int32)
    (K, X, U, W, pose, cn), kw = _dev((c["K"], c["pts3d"], c["pts2d"], c["weights"], c["pose"], counts), dict(bbox_3d=c["bbox_3d"], diameter=c["diameter"]))
    pose_covariance(K, X, U, W, pose, cn, **kw)
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        pose_covariance(K, X, U, W, pose, cn, nan_to_num=True, **kw)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    bad = [n for n in names if n in ("aten::_to_copy", "aten::clone", "aten::copy_")]
    assert not bad, bad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_covariance(K.cpu(), X, U, W, pose, cn, **kw)


def _chain_inputs(head, stride):
    from lc_amd import synth
    from lc_amd.config import AttrDict

    if head == "sparse":
        gt, out = synth.sparse_inputs(B=8, N=16, seed=4)
        gt["diameter"] = torch.linspace(0.2, 0.4, 8)
        return AttrDict(solvers=["weighted"]), gt, out
    gt, out = (synth.dense_inputs if head == "continuous" else synth.bin_inputs)(B=8, H=16, W=16, seed=4)
    gt["diameter"] = torch.linspace(80.0, 120.0, 8)
    cfg = AttrDict(dense_point_select="quantile", quantile=0.3, dense_sample=stride, solvers=["weighted", "weighted_filtered"])
    return cfg, gt, out


@pytest.mark.parametrize("head,stride", [("continuous", 1), ("continuous", 2), ("code", 1), ("code", 2), ("sparse", 0)])
def test_chain(head, stride, monkeypatch):
    """The test-time chain, scaled down (8 objects, 16x16 maps): `solve_pnp_with_cov` returns `solve_pnp`'s states bit for bit; every PoseCov
    meets the tolerance against the fp64 oracle on the rows, weights, counts and pose the chain handed to the kernel (recorded at the call),
    and those poses ARE the returned states; the graphed call and the two-stream call equal the eager one bit for bit."""
    from lc_amd import inference

    cfg, gt_c, out_c = _chain_inputs(head, stride)
    gt = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in gt_c.items()}
    out = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in out_c.items()}
    plain = inference.solve_pnp(cfg, out, gt)
    calls = []
    real = inference.pose_covariance

    def recording(*args, **kw):
        res = real(*args, **kw)
        calls.append((args, kw, res))
        return res

    monkeypatch.setattr(inference, "pose_covariance", recording)
    states, covs = inference.solve_pnp_with_cov(cfg, out, gt)
    monkeypatch.setattr(inference, "pose_covariance", real)
    assert list(states) == list(plain) and all(torch.equal(states[k], plain[k]) for k in plain)
    weighted = [k for k in states if k != "ransac"]
    assert sorted(covs) == sorted(weighted) and "ransac" not in covs
    assert len(calls) == 1  # both selections in ONE covariance launch
    args, kw, res = calls[0]
    pose = args[4]
    if len(weighted) == 2:
        assert kw["shared_poses"] == 8 and torch.equal(pose, torch.cat((states["weighted"], states["weighted-filtered"])))
        for i, k in enumerate(("weighted", "weighted-filtered")):
            assert all(torch.equal(a, b.chunk(2)[i]) for a, b in zip(covs[k], res))
    else:
        assert torch.equal(pose, states["weighted"]) and all(torch.equal(a, b) for a, b in zip(covs["weighted"], res))
    cargs = [None if a is None else a.cpu() for a in args] + [None] * (6 - len(args))  # (the sparse chain passes no counts)
    ckw = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    n = cargs[5] if cargs[5] is not None else torch.full((cargs[1].shape[0],), cargs[1].shape[1])
    _check(res, po.pose_covariance(*cargs, **ckw), po.pose_covariance(*cargs, **ckw, dtype=torch.float32), rows=n >= 6, what=f"{head}/{stride}")

    def same(a, b):
        (sa, ca), (sb, cb) = a, b
        return (list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa) and list(ca) == list(cb)
                and all(torch.equal(x, y) for k in ca for x, y in zip(ca[k], cb[k])))

    graphed = inference.GraphedSolvePnP(cfg, out, gt, with_cov=True)
    assert same(graphed(out, gt), (states, covs))
    if head != "sparse":
        monkeypatch.setenv("LC_AMD_TEST_TIME_STREAMS", "2")
        cut = inference.solve_pnp_with_cov(cfg, out, gt)
        torch.cuda.synchronize()
        assert same(cut, (states, covs))
