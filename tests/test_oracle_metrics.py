"""Pin oracle/pose_error_oracle.py against goldens from the reference's lib/utils/error6d.py, and the inputs of the GPU tests of the
pose-error kernel against that oracle."""
import glob
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

from oracle import pose_error_oracle as orc
from tests import metrics_cases as mc
from tests.util import GOLDEN


def test_pose_error_oracle_vs_reference():
    z = np.load(os.path.join(GOLDEN, "pose_err_b12_m700.npz"))
    pts = z["in_pts"].astype(np.float64)
    for i in range(len(z["in_R_est"])):
        e = orc.compute_pose_errors(z["in_R_est"][i].astype(np.float64), z["in_t_est"][i].astype(np.float64),
                                    z["in_R_gt"][i].astype(np.float64), z["in_t_gt"][i].astype(np.float64), pts)
        for k, v in e.items():
            assert abs(v - z["ref_" + k][i]) <= 1e-9 * max(1.0, abs(z["ref_" + k][i])), (i, k)


# ---- the inputs of the GPU tests of lc_pose_errors_kernel (tests/metrics_cases.py): what they can see, shown with the oracle alone --------

def test_edge_indices_are_the_loop_edges_of_the_kernel():
    assert mc.edge_indices(1) == mc.edge_indices(2) == mc.edge_indices(3) == []
    assert mc.edge_indices(9) == [0, 1, 2, 3, 7, 8]
    assert mc.edge_indices(257) == [0, 1, 2, 3, 254, 255, 256]
    assert mc.edge_indices(1025) == [0, 1, 2, 3, 254, 255, 256, 257, 510, 511, 512, 513, 766, 767, 768, 769, 1022, 1023, 1024]
    e = mc.edge_indices(5000)
    assert len(e) == 6 + 4 * 7 and {4094, 4095, 4096, 4097, 4998, 4999} <= set(e)
    # odd and even counts on both sides of a tile (1024) and of a query group
    assert mc.WITNESS_COUNTS == (1, 2, 3, 9, 255, 256, 257, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 4095, 4096, 4097, 5000)


def test_witness_clouds_layout():
    """One packed buffer; offsets of both parities, so slices start off 8- and 16-byte boundaries; the second set re-reads the largest cloud;
    every vertex at an edge index of every pose is a witness: WITNESS_RADIUS from the cloud and hundreds of units from any other vertex."""
    c = mc.packed_witness_case()
    pts, d, o = c["pts"], c["disjoint"], c["overlap"]
    assert pts.dtype == np.float32 and tuple(d["cnt"]) == mc.WITNESS_COUNTS
    assert (d["off"][1:] >= d["off"][:-1] + d["cnt"][:-1]).all() and d["off"][-1] + d["cnt"][-1] == len(pts)
    for s in (d, o):
        byte = 12 * s["off"].astype(np.int64)
        assert (s["off"] % 2 == 1).any() and (s["off"] % 2 == 0).any() and (byte % 8 != 0).any() and (byte % 16 != 0).any()
    assert (o["off"] >= d["off"][-1]).all() and (o["off"] + o["cnt"] <= len(pts)).all()
    assert len(set(zip(o["off"], o["cnt"]))) == len(o["cnt"]) >= 4 and len(set(o["off"])) >= 3
    for s in (d, o):
        for i in range(len(s["cnt"])):
            p = pts[s["off"][i]:s["off"][i] + s["cnt"][i]].astype(np.float64)
            edges = mc.edge_indices(len(p))
            if not edges:
                continue
            r = np.linalg.norm(p - np.delete(p, edges, axis=0).mean(0) if len(p) > len(edges) else p, axis=1)
            far = r > 0.9 * mc.WITNESS_RADIUS
            assert far[edges].all() and far.sum() <= 60, (i, far.sum())
            dist, _ = cKDTree(p).query(p[edges], k=2)
            assert dist[:, 1].min() > 300, (i, dist[:, 1].min())


@pytest.mark.parametrize("which", ["disjoint", "overlap"])
def test_witness_clouds_meet_both_conditions(which):
    """For every pose and every edge index, none exempt: ADI without that est-pose vertex, and ADI with that query's distance zeroed, are
    20 tolerances or more from ADI; and the float32 restatement of the reference formula is within 1/20 of a tolerance of the oracle."""
    c = mc.packed_witness_case()
    rows = mc.assert_witness_conditions(c[which], c["pts"], which)
    assert len(rows) == len(c[which]["cnt"]) and sum(r["edges"] for r in rows) >= 100
    print(f"{which}: least target x{min(r['target'] for r in rows):.0f}, least query x{min(r['query'] for r in rows):.0f}, "
          f"most float32 {max(r['f32'] for r in rows):.4f} tol")


def test_second_neighbour_stands_for_deleting_the_vertex():
    """witness_conditions reads 'ADI without est-pose vertex j' off the two nearest neighbours; here it is computed by deleting the vertex."""
    c = mc.packed_witness_case()
    for which, poses in (("disjoint", (3, 6, 9)), ("overlap", (4,))):
        s = c[which]
        rows = mc.witness_conditions(s, c["pts"])
        for i in poses:
            a = mc.pose_of(s, i, c["pts"])
            full = orc.adi(*a)
            shifts = [abs(orc.adi_without_target(*a, j) - full) for j in mc.edge_indices(len(a[4]))]
            assert len(shifts) >= 6 and abs(min(shifts) / mc.tol(full) - rows[i]["target"]) <= 1e-6 * rows[i]["target"]


def test_a_skipped_last_vertex_of_an_odd_tile_is_out_of_tolerance():
    """The fault the witnesses are for, by deleting the vertex: a search over pairs that drops the last vertex of a tile with an odd count
    (est-pose vertex M - 1 of an odd M) is 20 tolerances or more off on every odd cloud that has witnesses."""
    c = mc.packed_witness_case()
    s = c["disjoint"]
    odd = [i for i, M in enumerate(s["cnt"]) if M % 2 and M > 3]
    assert len(odd) == 9
    for i in odd:
        a = mc.pose_of(s, i, c["pts"])
        full = orc.adi(*a)
        assert abs(orc.adi_without_target(*a, len(a[4]) - 1) - full) >= mc.SENSITIVITY * mc.tol(full)


def test_symmetric_and_random_rotation_cases_search_for_another_vertex():
    for n_fold, base in ((6, 171), (8, 288)):
        s = mc.symmetric_case(n_fold, base, seed=50 + n_fold)
        assert len(s["pts"]) == n_fold * base
        for i in range(n_fold - 1):
            a = mc.pose_of(s, i, s["pts"])
            d, idx = orc.nearest(*a)
            assert (idx != np.arange(len(idx))).mean() >= 0.9 and 20 * d.mean() < orc.add(*a)
            assert abs(mc.adi_float32(*a) - d.mean()) <= mc.FLOAT32_SHARE * mc.tol(d.mean())
    for M in (1025, 2300):
        s = mc.random_rotation_case(M, 4, seed=60 + M)
        for i in range(4):
            a = mc.pose_of(s, i, s["pts"])
            d, idx = orc.nearest(*a)
            assert (idx != np.arange(M)).mean() >= 0.9
            assert abs(mc.adi_float32(*a) - d.mean()) <= mc.FLOAT32_SHARE * mc.tol(d.mean())


def test_re_transposed_is_re_for_rotations_and_the_sum_of_squares_for_identical_matrices():
    R = Rotation.random(32, random_state=1).as_matrix()
    E = R @ Rotation.from_rotvec(np.random.default_rng(2).normal(size=(32, 3))).as_matrix()
    for e, g in zip(E, R):
        assert abs(orc.re_transposed(e, g) - orc.re(e, g)) <= 1e-9 and 1 < orc.re(e, g) < 179
    # identical float32 matrices: the reference's inverse gives 0; the transposed form gives acos of ((sum of squares) - 1) / 2
    R32 = R.astype(np.float32).astype(np.float64)
    short = [(r * r).sum() < 3 for r in R32]
    assert any(short) and not all(short)
    for r, sh in zip(R32, short):
        assert orc.re(r, r) <= 1e-5 and (orc.re_transposed(r, r) > 1e-3) == sh and orc.re_transposed(r, r) <= 0.05
    for r in mc.proper_signed_permutations().astype(np.float64):
        assert abs(np.linalg.det(r) - 1) == 0 and orc.re_transposed(r, r) == 0 and mc.adi_float32(r, np.ones(3), r, np.ones(3), np.eye(3)) == 0


def test_re_angle_cases_cover_the_angles():
    names, Re, Rg = mc.re_angle_cases()
    want = dict(mc.RE_ANGLES)
    assert set(want) == {"0", "1e-3 rad", "1 deg", "90 deg", "179.9 deg", "180 deg"} and len(names) == 9 * len(want)
    for n, e, g in zip(names, Re, Rg):
        angle = np.degrees(want[n.split(" about")[0].split(" random")[0]])
        assert abs(orc.re_transposed(e.astype(np.float64), g.astype(np.float64)) - angle) <= 0.05, n
        if "identity" in n and n.startswith(("0 ", "180 deg")):
            assert orc.re_transposed(e.astype(np.float64), g.astype(np.float64)) == angle


def test_state_convention_is_the_one_transforms_documents():
    """quaternion_rep_to_RT_f64 (the oracle side of the from-states GPU test) equals lc_amd.transforms.quaternion_rep_to_RT in float64, and
    a quaternion of length s gives (1 - s) I + s R(q / s)."""
    import torch

    from lc_amd.transforms import quaternion_rep_to_RT

    c = mc.states_case()
    for key in ("states_est", "states_gt"):
        R, t = mc.quaternion_rep_to_RT_f64(c[key])
        Rt, tt = quaternion_rep_to_RT(torch.from_numpy(c[key]).double())
        assert np.abs(R - Rt.numpy()).max() <= 1e-14 and np.array_equal(t, tt.numpy())
        q = c[key][:, :4].astype(np.float64)
        s = np.linalg.norm(q, axis=1)
        rot = Rotation.from_quat((q / s[:, None])[:, [1, 2, 3, 0]]).as_matrix()
        assert np.abs(R - ((1 - s)[:, None, None] * np.eye(3) + s[:, None, None] * rot)).max() <= 1e-12
    n_est, n_gt = (np.linalg.norm(c[k][:, :4], axis=1) for k in ("states_est", "states_gt"))
    assert (np.abs(n_est[2:] - 1) > 0.05).all() and (np.abs(n_gt[:c["unit_gt"]] - 1) < 1e-6).all() and (np.abs(n_gt[c["unit_gt"]:] - 1) > 0.005).all()
