"""CPU half of the camera tests (tests/camera_cases.py): the inputs discriminate, the oracles hold on them, the conditions of the GPU half.

(1) `synth`'s default camera is today's, bit for bit, and the new cameras change nothing but K and what is projected through it.
(2) The mutant table: the loss, keypoint-NLL and PnP oracles evaluated with a wrongly read camera (camera_cases.mutants) are pushed as "got"
    through the very checks tests/test_gpu_cameras.py applies to the kernels.  Every mutant must FAIL them on "stress", the principal-point
    swap also on "bop"; on "rot" -- all the suite had -- the two swaps and the orthogonal inverse pass: that was the gap.
(3) The oracles themselves were only ever held against the reference on "rot" cameras.  The loss oracle is pinned by the two reference
    fixtures lc_loss_bopK_B3_N16 / lc_loss_stressK_B3_N16 (tests/test_oracle_loss.py picks them up); the PnP oracle by the stationarity of
    a plainly written float64 reprojection cost at the pose it returns.
(4) Conditions checked where no GPU is needed: the oracle ends valid on >= 90 % of every LM case; the RANSAC band excludes <= 1 % of points.
"""
import os

import numpy as np
import pytest
import torch

from lc_amd import synth
from oracle import p3p_ransac_oracle as O
from tests import camera_cases as cc
from tests.util import GOLDEN

ALL = ("rot",) + cc.CAMERAS


# ---- (1) the generators ------------------------------------------------------------------------------------------------------------

def test_default_camera_keeps_the_bits_of_the_committed_fixtures():
    """No `camera` argument == the generator before the keyword existed: the inputs stored in fixtures that were cut from synth batches."""
    z = np.load(os.path.join(GOLDEN, "lc_loss_metric_B256_N64.npz"))
    b = synth.make_batch(256, 64, seed=0, dtype=torch.float64)
    for k in ("K", "pose", "pts3d", "pts2d", "inv_std", "bbox_3d", "start"):
        assert torch.equal(b[k], torch.from_numpy(z["in_" + k])), k
    z = np.load(os.path.join(GOLDEN, "ransac_outliers_B24_N64.npz"))
    b = synth.make_batch(24, 64, seed=6, outlier_frac=0.0, noise_px=0.5)  # tests/golden/gen_golden_ransac.py CASES
    assert torch.equal(b["K"], torch.from_numpy(z["in_K"])) and torch.equal(b["pts3d"], torch.from_numpy(z["in_pts3d"]))
    assert torch.equal(b["pose"], torch.from_numpy(z["in_pose_gt"]))
    keep = ~torch.from_numpy(z["in_outlier"])  # the generator overwrites the outliers' image points
    assert torch.equal(b["pts2d"][keep], torch.from_numpy(z["in_pts2d"])[keep])
    # the lossfn_* trajectories store the reference's outputs, not their inputs: the float64 reference's keypoint loss of step 0 is a function
    # of every tensor of sparse_inputs(seed=0) -- K, pose, model and image points, deviations -- and is met to rounding only by the same inputs
    from oracle import kpt_oracle

    z = np.load(os.path.join(GOLDEN, "lossfn_sparse_f64.npz"))
    gt, out = synth.sparse_inputs(seed=0)
    d = torch.float64
    nll = kpt_oracle.kpt_nll_per_sample(gt["out_K"].to(d), gt["pose_best"].to(d), gt["pts3d"].to(d), out["pts2d"].to(d), out["pts2d_std"].to(d))
    want = float(z["s0_loss_loss_kpts"])
    assert abs(nll.sum().item() / out["pts2d"].numel() - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("camera", ALL)
def test_cameras_change_k_and_what_is_projected_through_it_only(camera):
    base, b = synth.make_batch(7, 33, seed=5), synth.make_batch(7, 33, seed=5, camera=camera)
    for k in ("pose", "pts3d", "inv_std", "bbox_3d", "start"):
        assert torch.equal(b[k], base[k]), k
    assert torch.equal(b["K"], base["K"]) == (camera == "rot") and torch.equal(b["pts2d"], base["pts2d"]) == (camera == "rot")
    K = b["K"].double()
    scaled_rotation = bool((K[:, 0, 0] == K[:, 1, 1]).all() and (K[:, 0, 1] == -K[:, 1, 0]).all() and (K[:, 0, 2] == K[:, 1, 2]).all())
    assert scaled_rotation == (camera == "rot")
    if camera == "bop":  # K2 = f Rot diag(1, fy / fx) with LM-O's ratio: singular values in that ratio, no skew beyond it
        s = torch.linalg.svdvals(K[:, :2, :2])
        assert torch.allclose(s[:, 0] / s[:, 1], torch.full((7,), 573.57043 / 572.4114, dtype=torch.float64), rtol=1e-6)
    # the correspondences stay consistent with `pose`: the noise-free twin projects onto its own image points
    clean = synth.make_batch(7, 33, seed=5, camera=camera, noise_px=0.0, outlier_frac=0.0)
    from oracle import kpt_oracle

    proj = kpt_oracle.project(clean["K"].double(), clean["pose"].double(), clean["pts3d"].double())
    assert (proj - clean["pts2d"].double()).abs().max() < 1e-3  # float32 image points of a few tens of pixels
    with pytest.raises(ValueError):
        synth.make_batch(2, 4, camera="fisheye")
    # the test-time generator: same draws, K and the ray-cast maps differ
    _, gt0, out0 = synth.test_time_inputs("plumb", B=3, seed=2)
    _, gt, out = synth.test_time_inputs("plumb", B=3, seed=2, camera=camera)
    for k in ("pose_best", "noc_scale", "bbox_3d", "out_pix_scale"):
        assert torch.equal(gt[k], gt0[k]), k
    assert torch.equal(out["xyz_weights_scale"], out0["xyz_weights_scale"])
    assert torch.equal(gt["out_K"], gt0["out_K"]) == (camera == "rot") and torch.equal(out["xyz_noc"], out0["xyz_noc"]) == (camera == "rot")
    assert 0.1 < gt["msk_vis"].mean() < 0.5  # the object is still in the crop
    # ... and consistent with the pose: a visible pixel's model point projects back onto the pixel (the xyz head carries 1 % noise of ~40 mm)
    X = (out["xyz_noc"].double() * gt["noc_scale"].double()[:, :, None, None]).permute(0, 2, 3, 1).reshape(3, -1, 3)
    back = kpt_oracle.project(gt["out_K"].double(), gt["pose_best"].double(), X).reshape(3, 32, 32, 2)
    ys, xs = torch.meshgrid(torch.arange(32.0, dtype=torch.float64), torch.arange(32.0, dtype=torch.float64), indexing="ij")
    err = (back - torch.stack((xs, ys), -1)).norm(dim=-1)[gt["msk_vis"] > 0]
    assert err.median() < 0.5, err.median()


# ---- (2) the mutant table ----------------------------------------------------------------------------------------------------------

def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _loss_mutant_fails(camera, name):
    ins, kw, ref64, ref32 = cc.loss_case("registers", camera)[:4]
    got = cc.oracle_run(dict(ins, K=cc.mutants(ins["K"])[name]), torch.float64, **kw)
    return _fails(cc.check_loss, f"loss {camera} {name}", got, ref64, ref32)


def _kpt_mutant_fails(camera, name):
    b, std, pose, ref64, ref32 = cc.kpt_case(*cc.KPT_CASES[0], camera)
    got = cc.kpt_oracle_run(cc.mutants(b["K"])[name], pose, b, std, torch.float64)
    return _fails(cc.check_kpt, f"kpt {camera} {name}", got, ref64, ref32)


def _pnp_mutant_fails(camera, name):
    b = cc.pnp_batch("B16_N64", camera)
    got = cc.pnp_oracle_solve(b, K=cc.mutants(b["K"])[name])
    return _fails(cc.check_pnp, f"pnp {camera} {name}", got, cc.pnp_reference("B16_N64", camera))


@pytest.mark.parametrize("what,fails", [("loss", _loss_mutant_fails), ("kpt", _kpt_mutant_fails), ("pnp", _pnp_mutant_fails)])
def test_wrongly_read_cameras_fail_the_gpu_checks(what, fails):
    table = {cam: {m: fails(cam, m) for m in cc.MUTANTS} for cam in ALL}
    for cam in ALL:
        print(f"{what:4s} on {cam:6s}: " + ", ".join(f"{m} {'FAILS' if f else 'passes'}" for m, f in table[cam].items()))
    assert all(table["stress"].values()), table["stress"]
    assert table["bop"]["swap_principal"], table["bop"]
    # the gap: a scaled rotation with a centred principal point cannot tell these three apart from the right camera
    assert not table["rot"]["swap_focal"] and not table["rot"]["swap_principal"] and not table["rot"]["as_rotation"], table["rot"]
    assert table["rot"]["transpose"]  # (the rotation's sign was the one thing the old inputs did pin)


@pytest.mark.parametrize("camera", ALL)
def test_the_true_camera_passes_the_gpu_checks(camera):
    """The other half of the table: the checks pass what they should -- the fp32 evaluation of each oracle with the right camera."""
    ins, kw, ref64, ref32 = cc.loss_case("registers", camera)[:4]
    cc.check_loss("loss fp32", ref32, ref64, ref32)
    b, std, pose, k64, k32 = cc.kpt_case(*cc.KPT_CASES[0], camera)
    cc.check_kpt("kpt fp64", k64, k64, k32)
    cc.check_pnp("pnp", cc.pnp_reference("B16_N64", camera), cc.pnp_reference("B16_N64", camera))


# ---- (3) the PnP oracle on the new cameras -----------------------------------------------------------------------------------------

def _predicted_decrease(b, states):
    """Per job: the share of the weighted reprojection cost a Gauss-Newton step from the returned pose would still remove,
    g^T (J^T J)^-1 g / (2 cost), with the cost written out in float64 torch on the full K and differentiated by autograd with respect to a
    6-vector perturbation (rotation vector applied on the left, translation).  Zero at a stationary point; scale-free."""
    out = []
    for i in range(len(states)):
        K, X, u, s = (b[k][i].double() for k in ("K", "pts3d", "pts2d", "inv_std"))
        q, t = torch.from_numpy(states[i, :4]).double(), torch.from_numpy(states[i, 4:]).double()
        R = synth._quat_to_R(q)

        def residual(d):
            W = torch.zeros(3, 3, dtype=torch.float64)
            W[0, 1], W[0, 2], W[1, 0], W[1, 2], W[2, 0], W[2, 1] = -d[2], d[1], d[2], -d[0], -d[1], d[0]
            c = (X @ (torch.linalg.matrix_exp(W) @ R).T + t + d[3:]) @ K.T
            return ((c[:, :2] / c[:, 2:3] - u) * s).reshape(-1)

        J = torch.autograd.functional.jacobian(residual, torch.zeros(6, dtype=torch.float64), vectorize=True, strategy="forward-mode")
        r = residual(torch.zeros(6, dtype=torch.float64))
        g = J.T @ r
        out.append(float(g @ torch.linalg.solve(J.T @ J, g) / (r @ r)))
    return np.array(out)


@pytest.mark.parametrize("name", ["B16_N64", "B4_N300"])
def test_pnp_oracle_returns_a_stationary_pose_on_every_camera(name):
    """The solve stops when a step lowers the cost by less than ftol = 1e-6 of it and returns a float32 state, so the pose it returns is
    stationary only to that order: on the "rot" twins of these cases -- the cameras on which the oracle is pinned to the reference's solver
    -- a further Gauss-Newton step would remove up to 1.0e-6 (B16_N64) and 2.1e-7 (B4_N300) of the cost, medians 1.1e-7 and 3.7e-8 (measured first).  The
    same jobs under another camera follow the same trajectory through another projection and must stop at that level: the bound is twice
    the worst job of the "rot" twin.  A camera entry read wrongly inside the oracle would leave the pose at the optimum of another cost,
    where a step removes percents of it (asserted below by judging the returned poses with the mutants' cost: the median job above 1e-3)."""
    level = {}
    for cam in ALL:
        b = cc.pnp_batch(name, cam)
        st, _, ret = cc.pnp_reference(name, cam)
        assert (ret == 0).all()
        level[cam] = _predicted_decrease(b, st)
        print(f"{name} {cam}: predicted relative decrease at the returned pose max {level[cam].max():.2e} median {np.median(level[cam]):.2e}")
    for cam in cc.CAMERAS:
        assert level[cam].max() <= 2 * level["rot"].max(), (cam, level[cam].max(), level["rot"].max())
    # the measure does see a wrong camera: the stress pose judged by the cost of a mutant camera
    b = cc.pnp_batch(name, "stress")
    for m, Km in cc.mutants(b["K"]).items():
        assert np.median(_predicted_decrease(dict(b, K=Km), cc.pnp_reference(name, "stress")[0])) > 1e-3, m


# ---- (4) conditions of the GPU half ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("camera", cc.CAMERAS)
@pytest.mark.parametrize("name", list(cc.PNP_CASES))
def test_lm_cases_end_valid_on_nine_jobs_in_ten(name, camera):
    ret = cc.pnp_reference(name, camera)[2]
    assert (ret == 0).mean() >= 0.9, (name, camera, int((ret == 0).sum()), len(ret))


@pytest.mark.parametrize("camera", cc.CAMERAS)
@pytest.mark.parametrize("form", list(cc.LOSS_CASES))
def test_loss_cases_keep_the_census(form, camera):
    """A point-wise check says more than `rel_err` only if a fair share of the points has a small gradient (tests/test_gpu_loss.py: census)."""
    case = cc.loss_case(form, camera)
    assert cc.census(case[5][1]) >= 0.25, cc.census(case[5][1])


def _ransac_sides(camera):
    """The float64 oracle's RANSAC (the kernel's scoring rule: isotropic threshold thr_px sqrt|1 / det K2| in normalised coordinates) on
    camera_cases.ransac_case against the pixel test of its winner -> (points, points in the band, points outside the band whose side differs,
    points whose side differs at all)."""
    b, counts, thr = cc.ransac_case(camera)
    K, X, U = b["K"].numpy(), b["pts3d"].numpy(), b["pts2d"].numpy()
    n_all = n_band = n_bad = n_diff = 0
    for i in range(len(K)):
        n = int(counts[i])
        r = O.ransac(K[i], X[i], U[i], n, float(thr[i]), cc.RANSAC_ITERS, cc.RANSAC_SEED, i)
        if r["invalid"]:
            continue
        px, band = cc.pixel_band(K[i], X[i, :n], U[i, :n], r["R"].astype(np.float32), r["t"].astype(np.float32), float(thr[i]), cc.band_half_width(K[i]))
        mine = np.zeros(n, bool)
        mine[r["inliers"]] = True
        n_all, n_band, n_bad, n_diff = n_all + n, n_band + int(band.sum()), n_bad + int((mine != px)[~band].sum()), n_diff + int((mine != px).sum())
    return n_all, n_band, n_bad, n_diff


def test_ransac_threshold_is_the_pixel_test_within_the_band_on_bop():
    """tests/test_gpu_cameras.py::test_ransac_inliers_are_opencvs_outside_the_band, on the oracle: the seed keeps the band under its cap."""
    n_all, n_band, n_bad, n_diff = _ransac_sides("bop")
    print(f"bop: {n_band} of {n_all} points in the band, {n_diff} differ from the pixel test, {n_bad} of them outside the band")
    counts = cc.ransac_case("bop")[1]
    assert n_all == int(counts[counts >= 4].sum()) and n_band <= 0.01 * n_all and n_bad == 0  # every pose with four points found a consensus
    n_all, n_band, n_bad, n_diff = _ransac_sides("stress")
    print(f"stress: {n_diff} of {n_all} points ({n_diff / n_all:.2%}) on the other side of the pixel test")
