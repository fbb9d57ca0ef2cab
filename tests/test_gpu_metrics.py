"""GPU parity of the batched pose-error kernel against goldens from the reference's error6d.py and the numpy oracle."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import pose_error_oracle as orc
from tests import metrics_cases as mc
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


def test_pose_errors_vs_reference_golden():
    from lc_amd.metrics import compute_pose_errors

    z = np.load(os.path.join(GOLDEN, "pose_err_b12_m700.npz"))
    dev = torch.device("cuda:0")
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    e = compute_pose_errors(t("in_R_est"), t("in_t_est"), t("in_R_gt"), t("in_t_gt"), t("in_pts"))
    for k in ("adi", "add", "te"):
        ref = z["ref_" + k]
        assert np.abs(e[k].cpu().numpy() - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), k
    # re: acos near 0 amplifies the fp32 rounding of R (1e-7 in the trace -> ~0.03 deg); compare away from 0 tightly
    ref = z["ref_re"]
    got = e["re"].cpu().numpy()
    assert np.abs(got - ref)[ref > 0.5].max() <= 1e-3 and np.abs(got - ref).max() <= 0.05


def test_pose_errors_packed_objects_and_large_cloud():
    """Two objects with different vertex counts packed back to back (per-pose offset/count), M > one LDS tile."""
    from lc_amd.metrics import compute_pose_errors
    from oracle import pose_error_oracle as orc
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(3)
    cnt = [1500, 2300]
    pts = (rng.random((sum(cnt), 3)).astype(np.float32) * 2 - 1) * 40
    B = 6
    obj = np.array([0, 1, 1, 0, 1, 0])
    off = np.array([0, cnt[0]])[obj].astype(np.int32)
    num = np.array(cnt)[obj].astype(np.int32)
    Rg = Rotation.random(B, random_state=4).as_matrix().astype(np.float32)
    Re = (Rg @ Rotation.from_rotvec(rng.normal(size=(B, 3)) * 0.1).as_matrix()).astype(np.float32)
    tg = rng.normal(size=(B, 3)).astype(np.float32) * 30 + np.array([0, 0, 800], np.float32)
    te = tg + rng.normal(size=(B, 3)).astype(np.float32) * 5
    dev = torch.device("cuda:0")
    e = compute_pose_errors(*(torch.from_numpy(a).to(dev) for a in (Re, te, Rg, tg, pts)), pts_off=torch.from_numpy(off),
                            pts_cnt=torch.from_numpy(num))
    for i in range(B):
        p = pts[off[i]:off[i] + num[i]].astype(np.float64)
        r = orc.compute_pose_errors(Re[i].astype(np.float64), te[i].astype(np.float64), Rg[i].astype(np.float64), tg[i].astype(np.float64), p)
        for k in ("adi", "add", "te"):
            assert abs(float(e[k][i]) - r[k]) <= 2e-5 * max(1.0, r[k]), (i, k)
        assert abs(float(e["re"][i]) - r["re"]) <= 1e-3


# ---- the paths inside lc_pose_errors_kernel: tests/metrics_cases.py builds the inputs, oracle/pose_error_oracle.py (fp64) judges ----------

_KEYS = ("adi", "add", "re", "te")


@functools.lru_cache(maxsize=None)
def _witness_case():
    return mc.packed_witness_case()


def _launch(s, pts, column_t=False, **kw):
    """One launch over the poses of a set (packed if it has offsets) -> dict of (B,) float32 numpy arrays."""
    from lc_amd.metrics import compute_pose_errors

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tc = (lambda a: t(a).reshape(-1, 3, 1)) if column_t else t
    if "off" in s:
        kw.update(pts_off=torch.from_numpy(s["off"]), pts_cnt=torch.from_numpy(s["cnt"]))
    e = compute_pose_errors(t(s["R_est"]), tc(s["t_est"]), t(s["R_gt"]), tc(s["t_gt"]), t(pts), **kw)
    torch.cuda.synchronize()
    out = {k: e[k].cpu().numpy() for k in _KEYS}
    assert all(v.shape == (len(s["R_est"]),) and v.dtype == np.float32 for v in out.values())
    return out


def _check_vs_oracle(e, s, pts, label):
    """adi, add, te at the project's tolerance; re at 1e-3 deg against the reference formula (0.05 deg within half a degree of 0 and 180,
    as in the golden test) and at RE_TOL against the form the kernel documents.  Every figure is printed before anything is asserted."""
    rows = []
    for i in range(len(s["R_est"])):
        a = mc.pose_of(s, i, pts)
        r = orc.compute_pose_errors(*a)
        rt = orc.re_transposed(a[0], a[2])
        rows.append((i, r, rt))
        print(f"{label} pose {i}: M={len(a[4])} " + " ".join(f"{k} {float(e[k][i]):.7g} (ref {r[k]:.9g}, off {abs(float(e[k][i]) - r[k]) / mc.tol(r[k]):.3f} tol)"
                                                              for k in ("adi", "add", "te"))
              + f" re {float(e['re'][i]):.7g} (ref {r['re']:.9g}, transposed {rt:.9g})")
    for i, r, rt in rows:
        for k in ("adi", "add", "te"):
            assert abs(float(e[k][i]) - r[k]) <= mc.tol(r[k]), (label, i, k, float(e[k][i]), r[k])
        assert abs(float(e["re"][i]) - r["re"]) <= (1e-3 if 0.5 < r["re"] < 179.5 else 0.05), (label, i, float(e["re"][i]), r["re"])
        assert abs(float(e["re"][i]) - rt) <= RE_TOL, (label, i, float(e["re"][i]), rt)


# re against oracle.re_transposed on the same float32 matrices, in degrees: the kernel rounds an output of up to 180 to float32 (half a
# float32 step at 180: 7.6e-6, bounded by 1.1e-5), and both sides sum the trace in fp64 in their own order, a difference of a few 1e-16
# that acos magnifies most at c = 1, to at most sqrt(2 * 1e-15) rad = 2.6e-6 deg.
RE_TOL = 2e-5


@pytest.mark.parametrize("which", ["disjoint", "overlap"])
def test_witness_clouds_in_one_packed_launch(which):
    """Every tile, pair-slot, query-slot and query-group edge of the ADI search, in one launch over one packed buffer.  `disjoint`: 18 clouds
    of 1 ... 5000 vertices back to back, offsets of both parities; `overlap`: five poses reading the largest cloud from three starts at five
    counts.  The vertices at the edge indices are witnesses (tests/metrics_cases.py): before the GPU result is looked at, the oracle shows
    that a kernel which skips any one of them, as a search target or as a query, is off by 20 tolerances or more, and that float32
    coordinates cost under 1/20 of a tolerance, for every pose and every edge index."""
    c = _witness_case()
    s, pts = c[which], c["pts"]
    assert (s["off"] % 2 == 1).any() and (s["off"] % 2 == 0).any() and (12 * s["off"] % 16 != 0).any()
    mc.assert_witness_conditions(s, pts, which)
    _check_vs_oracle(_launch(s, pts), s, pts, which)


def test_packed_poses_equal_their_own_launches_and_repeat_bit_for_bit():
    """A pose's result depends on nothing but its own slice: each pose of the two packed launches equals, bit for bit, the same pose launched
    alone (B = 1) on a copy of its vertices (no offsets: the M of the call, another alignment), and a second run of the whole launch equals
    the first."""
    c = _witness_case()
    for which in ("disjoint", "overlap"):
        s, pts = c[which], c["pts"]
        first, second = _launch(s, pts), _launch(s, pts)
        for k in _KEYS:
            assert np.array_equal(first[k].view(np.int32), second[k].view(np.int32)), (which, k)
        for i in range(len(s["cnt"])):
            one = {k: s[k][i:i + 1] for k in ("R_est", "t_est", "R_gt", "t_gt")}
            alone = _launch(one, pts[s["off"][i]:s["off"][i] + s["cnt"][i]].copy())
            for k in _KEYS:
                assert alone[k].view(np.int32)[0] == first[k].view(np.int32)[i], (which, i, k, float(alone[k][0]), float(first[k][i]))


@pytest.mark.parametrize("n_fold,base", [(6, 171), (8, 288)])
def test_symmetric_object_adi_finds_another_vertex(n_fold, base):
    """The case ADI exists for.  A ring with an n-fold symmetry (1026 and 2304 vertices), every estimate a symmetry element away from the
    ground truth plus a small error: ADD is tens of units, ADI a fraction of one, and the oracle's nearest est-pose vertex is the image of
    another vertex for (nearly) every query, so a search that favours the query's own index cannot pass."""
    s = mc.symmetric_case(n_fold, base, seed=50 + n_fold)
    for i in range(len(s["R_est"])):
        a = mc.pose_of(s, i, s["pts"])
        d, idx = orc.nearest(*a)
        share = (idx != np.arange(len(idx))).mean()
        print(f"{n_fold}-fold pose {i}: neighbour is another vertex for {share:.3f}, adi {d.mean():.4f}, add {orc.add(*a):.4f}")
        assert share >= 0.9 and 20 * d.mean() < orc.add(*a)
    _check_vs_oracle(_launch(s, s["pts"]), s, s["pts"], f"{n_fold}-fold")


@pytest.mark.parametrize("M", [1025, 2300])
def test_large_random_rotation_errors(M):
    """Estimate and ground truth uniform over SO(3), one cloud for the whole batch (no offsets: M comes from the call)."""
    s = mc.random_rotation_case(M, 4, seed=60 + M)
    for i in range(4):
        _, idx = orc.nearest(*mc.pose_of(s, i, s["pts"]))
        assert (idx != np.arange(M)).mean() >= 0.9
    _check_vs_oracle(_launch(s, s["pts"]), s, s["pts"], f"random rotations M={M}")


def test_identical_poses_give_exact_zeros():
    """R_est = R_gt, t_est = t_gt: adi, add and te are exactly 0 for every pose.  For adi that needs the query and the tile load to transform
    a vertex to the same bits (the reference and the float32 restatement both return exactly 0 for adi).

    re is exactly 0 wherever the form the kernel documents, acos((sum R_ij^2 - 1) / 2) in fp64, is: for the 24 rotations float32 holds
    exactly, and for the random ones whose float32 rounding has a squared norm of 3 or more.  Rounding leaves the others up to 1e-7 short
    of 3 and acos turns that into up to 0.02 deg (oracle figures: 0.0189, 0.0047 and 0.0163 deg for three of the first eight matrices of
    this test); there re must equal that form to RE_TOL, and stays under the 0.05 deg the golden test allows.  The reference's own
    inv(R_gt) is not exact either: fp64 rounding of R inv(R) leaves its re at 0 or at 1.2e-6 deg."""
    exact = mc.proper_signed_permutations()
    rnd = mc.random_rotation_case(3, 16, seed=5)["R_gt"]
    Rg = np.concatenate((exact, rnd))
    B = len(Rg)
    rng = np.random.default_rng(6)
    counts = (1, 2, 255, 1025, 2300)
    cnt = np.array([counts[i % len(counts)] for i in range(B)], np.int32)
    off = (np.arange(B) % 7).astype(np.int32)
    pts = ((rng.random((int((off + cnt).max()), 3)) * 2 - 1) * 40).astype(np.float32)
    tg = (rng.normal(size=(B, 3)) * 30 + np.array([0, 0, 800.0])).astype(np.float32)
    s = dict(R_est=Rg.copy(), t_est=tg.copy(), R_gt=Rg, t_gt=tg, off=off, cnt=cnt)
    e = _launch(s, pts)
    want_re = np.array([orc.re_transposed(R.astype(np.float64), R.astype(np.float64)) for R in Rg])
    for i in range(B):
        a = mc.pose_of(s, i, pts)
        assert orc.adi(*a) == 0 and mc.adi_float32(*a) == 0 and orc.add(*a) == 0 and orc.re(a[0], a[2]) <= 2e-6
        print(f"identical pose {i}: M={cnt[i]} " + " ".join(f"{k} {float(e[k][i])!r}" for k in _KEYS) + f" (re of the transposed form {want_re[i]!r})")
    assert (want_re[:len(exact)] == 0).all() and (want_re[len(exact):] == 0).any() and (want_re[len(exact):] > 0).any()
    for k in ("adi", "add", "te"):
        assert (e[k] == 0).all(), (k, e[k])
    assert (e["re"][want_re == 0] == 0).all(), e["re"]
    assert np.abs(e["re"] - want_re).max() <= RE_TOL and e["re"].max() <= 0.05, (e["re"], want_re)


def test_without_adi_the_other_outputs_keep_their_bits():
    """want_adi=False skips the search: the adi column is 0 and add, re, te are the bits of the want_adi=True launch."""
    c = _witness_case()
    s, pts = c["disjoint"], c["pts"]
    full, lean = _launch(s, pts), _launch(s, pts, want_adi=False)
    assert (full["adi"] > 1).all()
    assert (lean["adi"].view(np.int32) == 0).all(), lean["adi"]
    for k in ("add", "re", "te"):
        assert np.array_equal(full[k].view(np.int32), lean[k].view(np.int32)), (k, full[k], lean[k])


def test_rotation_error_to_the_last_float32_digit():
    """re against the form the kernel documents (R_gt^T for inv(R_gt)) on the same float32 matrices, to RE_TOL = 2e-5 deg: 0, 1e-3 rad,
    1 deg, 90 deg, 179.9 deg and 180 deg, each about six random axes from random ground truths (float32 rounding leaves neither matrix
    orthonormal, so near 0 and 180 the form itself is up to 0.03 deg from the angle asked for) and about the coordinate axes from the
    identity (180 deg exactly).  The looser comparison with the reference's formula stays: 1e-3 deg away from 0 and 180, 0.05 deg overall."""
    names, Re, Rg = mc.re_angle_cases()
    B = len(names)
    z = np.zeros((B, 3), np.float32)
    e = _launch(dict(R_est=Re, t_est=z, R_gt=Rg, t_gt=z), np.ones((4, 3), np.float32), want_adi=False)
    want = np.array([orc.re_transposed(Re[i].astype(np.float64), Rg[i].astype(np.float64)) for i in range(B)])
    ref = np.array([orc.re(Re[i].astype(np.float64), Rg[i].astype(np.float64)) for i in range(B)])
    for i in range(B):
        print(f"{names[i]}: re {float(e['re'][i])!r} transposed form {want[i]!r} (off {abs(e['re'][i] - want[i]):.2e}) reference {ref[i]!r}")
    assert {n.split(" about")[0].split(" random")[0] for n in names} == {n for n, _ in mc.RE_ANGLES}
    assert (e["re"][[n.startswith("180 deg about axis") for n in names]] == 180).all()
    assert (e["re"][[n.startswith("0 about axis") for n in names]] == 0).all()
    assert np.abs(e["re"] - want).max() <= RE_TOL
    mid = (ref > 0.5) & (ref < 179.5)
    assert mid.sum() >= B // 3 and np.abs(e["re"] - ref)[mid].max() <= 1e-3 and np.abs(e["re"] - ref).max() <= 0.05
    assert (e["te"] == 0).all()


def test_translations_as_columns():
    """t as (B,3,1), the reference's shape: the bits of the (B,3) launch, and the oracle's numbers."""
    s = mc.random_rotation_case(1025, 4, seed=70)
    flat, col = _launch(s, s["pts"]), _launch(s, s["pts"], column_t=True)
    for k in _KEYS:
        assert np.array_equal(flat[k].view(np.int32), col[k].view(np.int32)), k
    _check_vs_oracle(col, s, s["pts"], "column t")


def test_pose_errors_from_states_with_quaternions_of_any_length():
    """pose_errors_from_states on (B,7) states whose quaternions are not unit length, against the oracle on fp64 matrices built by the
    convention lc_amd/transforms.py documents (two_s = 2 / ||q||, the reference's: a quaternion of length s gives (1 - s) I + s R, not a
    rotation).  adi, add and te at the project's tolerance for every pose.  re: where the ground truth is a rotation (unit length, as a
    data set's is) R_gt^T is inv(R_gt) whatever the estimate, and re is held to the reference formula; where it is not, the two differ by
    tens of degrees and re is held to the form the kernel documents.  1e-3 deg, as for the other oracle comparisons: the float32 rounding
    of the matrices moves c by at most 9 * 1.2e-7 * 1.4^2 = 2.1e-6, which is 4e-4 deg for |c| <= 0.95 (checked), and c >= 1.01 is
    clamped on both sides."""
    from lc_amd.metrics import pose_errors_from_states

    c = mc.states_case()
    dev = torch.device("cuda:0")
    for a in (c["states_est"], c["states_gt"]):
        n = np.linalg.norm(a[:, :4], axis=1)
        print("quaternion lengths", n)
    assert (np.abs(np.linalg.norm(c["states_est"][2:, :4], axis=1) - 1) > 0.05).all()
    e = pose_errors_from_states(torch.from_numpy(c["states_est"]).to(dev), torch.from_numpy(c["states_gt"]).to(dev), torch.from_numpy(c["pts"]).to(dev))
    e = {k: v.cpu().numpy() for k, v in e.items()}
    Re, te = mc.quaternion_rep_to_RT_f64(c["states_est"])
    Rg, tg = mc.quaternion_rep_to_RT_f64(c["states_gt"])
    p = c["pts"].astype(np.float64)
    rows = []
    for i in range(len(Re)):
        r = orc.compute_pose_errors(Re[i], te[i], Rg[i], tg[i], p)
        cos = 0.5 * (np.sum(Re[i] * Rg[i]) - 1)
        want_re = r["re"] if i < c["unit_gt"] else orc.re_transposed(Re[i], Rg[i])
        rows.append((i, r, cos, want_re))
        print(f"states pose {i}: " + " ".join(f"{k} {float(e[k][i]):.7g} (ref {r[k]:.9g})" for k in _KEYS) + f" c {cos:.4f} re wanted {want_re:.9g}")
    for i, r, cos, want_re in rows:
        assert abs(cos) <= 0.95 or cos >= 1.01, (i, cos)
        for k in ("adi", "add", "te"):
            assert abs(float(e[k][i]) - r[k]) <= mc.tol(r[k]), (i, k, float(e[k][i]), r[k])
        assert abs(float(e["re"][i]) - want_re) <= 1e-3, (i, float(e["re"][i]), want_re)
