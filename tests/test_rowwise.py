"""tests/rowwise.py on the CPU: the row-wise measures see what `rel_err` does not, and the inputs of the GPU tests that use them have the
spread of gradient sizes that makes this matter.  Everything here is the fp64 oracle, its fp32 evaluation and the committed fixtures."""
import numpy as np
import pytest
import torch

from tests import rowwise as rw
from tests import test_gpu_loss as gl
from tests.util import GOLDEN, rel_err


@pytest.fixture(scope="module")
def batch16x64():
    """fp64 and fp32 oracle gradients of make_batch(16, 64, seed=1) under the suite's mask and cotangent -- computed once, never modified."""
    ins = gl.shape_inputs(16, 64, 1)
    return ins, gl.oracle_run(ins, torch.float64), gl.oracle_run(ins, torch.float32)


def test_point_error_definition():
    ref = torch.tensor([[[4.0, -2.0], [1e-5, 0.0], [0.5, 0.25]], [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]])
    got = ref.clone()
    got[0, 0, 1] += 0.04   # 1 % of the point's largest entry
    got[0, 1, 0] += 4e-5   # a point below eta x the sample's largest entry: judged against 4e-3
    e = rw.point_error(got, ref, 1)
    assert e.shape == (2, 3) and e.dtype == torch.float64
    assert e[0].tolist() == pytest.approx([0.01, 0.01, 0.0], rel=1e-6)
    assert e[1].tolist() == [0.0, 0.0, 0.0]  # an all-zero sample met exactly
    got[1, 2, 1] = 1e-30
    assert rw.point_error(got, ref, 1)[1].tolist() == [0.0, 0.0, float("inf")]  # ... and not met exactly
    assert rw.point_error(got[0:1], ref[0:1], 2).tolist() == [pytest.approx(0.01)]  # the whole sample as one point
    assert rw.sample_error is __import__("tests.posecov_oracle", fromlist=["row_error"]).row_error
    assert rw.sample_error(got[:1], ref[:1]).tolist() == [pytest.approx(0.01)]
    assert rw.bound_from_reference(1e-3) == 2e-3 and rw.bound_from_reference(0.0) == rw.FLOOR == 4 * 2.0 ** -24
    assert rw.bound_from_reference(torch.tensor([1e-3, float("nan"), float("inf"), 0.0], dtype=torch.float64)).tolist() == [2e-3, rw.FLOOR, rw.FLOOR, rw.FLOOR]


@pytest.mark.parametrize("which", [1, 2, 3], ids=["du", "ds", "dx"])
def test_one_percent_on_a_small_point_passes_rel_err_and_fails_point_error(batch16x64, which):
    _, r64, r32 = batch16x64
    ref, own = r64[which], rw.point_error(r32[which], r64[which])
    bound = rw.bound_from_reference(own)
    share = rw.batch_share(ref)
    sample_max = ref.abs().flatten(1).amax(1, keepdim=True)
    # a point rel_err cannot see (below 1 % of the batch's largest entry) that is no cancellation residue (above eta of its sample's largest)
    cand = (share < 1e-2) & (ref.abs().amax(-1) > 1e-3 * sample_max) & (bound < 5e-3)
    assert int(cand.sum()) >= 16
    b, n = cand.nonzero()[0].tolist()
    got = ref.clone()
    got[b, n] *= 1.01
    assert rel_err(got, ref) <= 3e-4  # the bound of test_loss_kernel_vs_oracle_shapes
    err = rw.point_error(got, ref)
    assert err[b, n].item() == pytest.approx(0.01, rel=1e-6) and err[b, n] > bound[b, n]
    assert int((err > bound).sum()) == 1
    with pytest.raises(AssertionError):
        rw.check("planted", got, ref, r32[which], point_dims=1)
    rw.check("clean", ref.float(), ref, r32[which], point_dims=1)  # the fp64 result rounded once passes everywhere


def test_one_percent_on_a_small_cotangent_sample_passes_rel_err_and_fails_sample_error():
    ins = gl.shape_inputs(16, 64, 1)
    ins["grad_out"] = gl.wide_grad_out(16, 1)
    r64, r32 = gl.oracle_run(ins, torch.float64), gl.oracle_run(ins, torch.float32)
    assert ins["grad_out"].max() / ins["grad_out"].min() > 1e4
    for ref, f32 in zip(r64[1:], r32[1:]):
        b = int(ref.abs().flatten(1).amax(1).argmin())  # the sample whose whole gradient is smallest
        assert rw.batch_share(ref)[b].max() < 1e-2
        got = ref.clone()
        got[b] *= 1.01
        assert rel_err(got, ref) <= 3e-4
        bound = rw.bound_from_reference(rw.sample_error(f32, ref))
        err = rw.sample_error(got, ref)
        assert err[b].item() == pytest.approx(0.01, rel=1e-6) and err[b] > bound[b] and int((err > bound).sum()) == 1
        with pytest.raises(AssertionError):
            rw.check("planted", got, ref, f32)


CENSUS = ([(B, N, s, {}) for B, N, s in gl.SHAPES if N >= gl.CENSUS_MIN_POINTS]
          + [(B, N, s, dict(batch_seed=200 + s, outlier_frac=0.1, cov_2d=True)) for B, N, s in gl.COV2D_SHAPES]
          + [(B, N, s, dict(outlier_frac=0.3)) for B, N, s in gl.OUTLIER_SHAPES])


@pytest.mark.parametrize("B,N,seed,opts", CENSUS, ids=[f"{B}x{N}" + ("-cov2d" if "cov_2d" in o else "-outliers" if o else "") for B, N, _, o in CENSUS])
def test_census_of_the_gpu_test_shapes(B, N, seed, opts):
    """On every shape the row-wise GPU tests of the LC loss use (tests/test_gpu_loss.py), with their inputs: at least a quarter of the points
    have a d_pts2d below 1 % of the batch's largest entry -- invisible to rel_err at its 3e-4 -- under both cotangents (cov_2d: the wide one), and fp32 arithmetic
    (the oracle in float32) stays below 1e-2 per point at eta = 1e-3, so a bound of twice its error still rejects a 2 % error on any point.
    (Worst fp32 values measured on make_batch inputs: 5.5e-3 for ds at 16 x 256, 9.5e-4 at 4 x 1024.)"""
    opts = dict(opts)
    kw = {"cov_2d": True} if opts.pop("cov_2d", False) else {}
    ins = gl.shape_inputs(B, N, seed, **opts)
    for wide, go in ((False, ins["grad_out"]), (True, gl.wide_grad_out(B, seed))):
        ins = dict(ins, grad_out=go)
        r64, r32 = gl.oracle_run(ins, torch.float64, **kw), gl.oracle_run(ins, torch.float32, **kw)
        assert gl.census(r64[1]) >= 0.25 or (kw and not wide)  # cov_2d: the GPU test asserts the census on its wide run only (its comment)
        for ref, f32 in zip(r64[1:], r32[1:]):
            assert rw.point_error(f32, ref).max().item() < 1e-2
            assert rw.point_error(ref.float(), ref).max().item() <= 2.0 ** -24  # what a kernel that rounds the fp64 value once shows


def test_noisefree_fixture_has_no_fp32_reference_to_take_a_bound_from():
    """lc_loss_noisefree_B2_N16: with err == 0 the fp64 reference sits on exact zeros (81 % of the d_pts2d points) where its fp32 run holds
    round-off noise, so neither a point-wise comparison with the fixture's outputs nor a bound from its f32_* arrays means anything --
    test_loss_kernel_vs_golden leaves it out of both (the oracle on the identical inputs still applies, under the floor alone)."""
    import os

    z = np.load(os.path.join(GOLDEN, "lc_loss_noisefree_B2_N16.npz"))
    zero = np.abs(z["f64_g_pts2d"]).max(-1) == 0
    assert zero.mean() >= 0.8
    assert (np.abs(z["f32_g_pts2d"]).max(-1)[zero] > 0).any()
    own = rw.point_error(torch.from_numpy(z["f32_g_pts2d"]), torch.from_numpy(z["f64_g_pts2d"]))
    assert own.max().item() > 1  # the fp32 run is further from the fp64 one than the gradient is large
    assert [p for p in gl.FILES if not gl.fixture_has_fp32_reference(p)] == [os.path.join(GOLDEN, "lc_loss_noisefree_B2_N16.npz")]
