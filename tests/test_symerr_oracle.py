"""The symmetry-aware pose errors without a GPU: the numpy oracle (tests/symerr_oracle.py) against the unmodified reference's mssd, mspd and
proj (tests/golden/sym_err_b12_m700.npz), and the conditions under which the inputs of tests/test_gpu_symerr.py can see the faults they
are built for -- shown with the oracle alone, for every pose, none left out."""
import numpy as np

from tests import symerr_cases as C
from tests import symerr_oracle as orc
from tests.util import GOLDEN


def _golden():
    return np.load(f"{GOLDEN}/sym_err_b12_m700.npz")


def test_golden_holds_what_the_issue_asks_for():
    z = _golden()
    assert z["R_est"].shape == (12, 3, 3) and z["pts"].shape == (700, 3) and z["cam_K"].shape == (12, 3, 3)
    assert all(z[k].dtype == np.float32 for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts"))
    case = C.golden_case(z)
    assert [len(R) for R, _ in case["transforms"]] == [1, 2, 4, 36] and sorted(set(z["obj_index"].tolist())) == [0, 1, 2, 3]
    import json

    cont = json.loads(str(z["models_info"]))[3]["symmetries_continuous"][0]
    assert any(cont["offset"]) and min(abs(a) for a in cont["axis"]) > 0.2
    assert z["mssd_sym"].max() > 4 and (z["mssd_sym"] != 0).sum() >= 6  # the minimum is not always the identity
    # the inputs the generator would draw today are the stored ones
    again, _ = C.golden_inputs()
    for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts", "obj_index"):
        assert np.array_equal(again[k], z[k]), k


def test_oracle_vs_reference_golden():
    z = _golden()
    case = C.golden_case(z)
    err, arg = orc.batch(case)
    for j, name in enumerate(("mssd", "mspd", "proj")):
        rel = np.abs(err[:, j] - z[name]) / np.abs(z[name])
        print(f"{name}: largest relative difference {rel.max():.2e}")
        assert (rel <= 1e-9).all(), name
    assert np.array_equal(arg[:, 0], z["mssd_sym"]) and np.array_equal(arg[:, 1], z["mspd_sym"])
    # arg is decidable: the runner-up lies at least 20 tolerances above the winner in every pose with more than one symmetry
    for b in range(12):
        for e in orc.per_symmetry(*C.pose_args(case, b)):
            s = np.sort(e)
            assert len(s) == 1 or (s[1] - s[0]) / C.tol(s[0]) >= C.SENSITIVITY, b


def test_edge_lists_follow_the_kernel_s_constants():
    src = open(f"{GOLDEN}/../../lc_amd/csrc/symerr/lc_sym_metrics.hip").read() + open(f"{GOLDEN}/../../lc_amd/csrc/symerr/lc_sym_metrics_args.h").read()
    assert "constexpr int kThreads = 256;" in src and f"constexpr int kUnroll = {C.UNROLL};" in src and f"constexpr int kSymErrChunk = {C.CHUNK};" in src
    assert C.WAVES == 256 // C.WAVE and "__shared__ unsigned long long s_key[2][kWaves];" in src and src.count("__shared__") == 1  # no LDS tile
    assert C.vertex_edges(1) == [0] and C.vertex_edges(2) == [0, 1] and C.vertex_edges(65) == [0, 1, 63, 64]
    assert C.vertex_edges(133) == [0, 1, 63, 64, 65, 127, 128, 129, 131, 132]
    assert {1, 2, 63, 64, 65} <= set(C.VERTEX_COUNTS) and max(C.VERTEX_COUNTS) > 2 * C.WAVE * C.UNROLL
    assert any(C.WAVE * C.UNROLL < m < C.WAVE * C.UNROLL + 8 for m in C.VERTEX_COUNTS)  # a few vertices beyond a trip
    assert C.symmetry_edges(1) == [0] and C.symmetry_edges(17) == [0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16]
    want = {1, 2, 3} | {e + d for e in (C.WAVES, C.CHUNK, 2 * C.CHUNK) for d in (-1, 0, 1)}
    assert set(C.SYM_COUNTS) == want and max(C.SYM_COUNTS) == 2 * C.CHUNK + 1


def test_every_edge_vertex_decides_both_maxima():
    case = C.vertex_edge_case()
    rows = C.vertex_conditions(case)
    assert [(r["M"], r["edge"]) for r in rows] == [(M, e) for M in C.VERTEX_COUNTS for e in C.vertex_edges(M)]
    for b, r in enumerate(rows):
        print(f"pose {b}: M={r['M']} edge={r['edge']} off={int(case['pts_off'][b])} without it mssd moves x{r['mssd']:.0f} mspd x{r['mspd']:.0f} tolerances")
        assert r["mssd"] >= C.SENSITIVITY and r["mspd"] >= C.SENSITIVITY, (b, r)
    assert len({int(o) % 2 for o in case["pts_off"]}) == 2  # offsets of both parities in the one packed buffer
    assert sorted({len(case["transforms"][o][0]) for o in case["obj_index"]}) == [1, 2, 5]


def test_every_edge_symmetry_decides_both_minima():
    case = C.symmetry_edge_case()
    rows = C.symmetry_conditions(case)
    assert [(r["K"], r["win"]) for r in rows] == [(K, k) for K in C.SYM_COUNTS for k in C.symmetry_edges(K)]
    for b, r in enumerate(rows):
        print(f"pose {b}: K={r['K']} winner {r['win']}: without it (= the runner-up) mssd x{r['mssd']:.0f} mspd x{r['mspd']:.0f} tolerances above")
        assert r["k3"] == r["win"] and r["k2"] == r["win"], (b, r)
        assert r["mssd"] >= C.SENSITIVITY and r["mspd"] >= C.SENSITIVITY, (b, r)


def test_tie_cases_are_ties():
    case = C.tie_case()
    R, t = case["transforms"][0]
    assert np.array_equal(R[2], R[4]) and np.array_equal(t[2], t[4])
    for b in range(3):
        e3, e2 = orc.per_symmetry(*C.pose_args(case, b))
        assert e3[2] == e3[4] and e2[2] == e2[4] and int(np.argmin(e3)) == 2 and int(np.argmin(e2)) == 2
        assert np.sort(e3)[2] - e3[2] > C.SENSITIVITY * C.tol(e3[2]) and np.sort(e2)[2] - e2[2] > C.SENSITIVITY * C.tol(e2[2])
        assert C.lowest_fp32_winner(e3, np.float32(e3[2])) == 2
    near = C.tie_case(last_bit=True)
    Rn, tn = near["transforms"][0]
    assert (Rn[2] != Rn[4]).sum() == 1 and (tn[2] != tn[4]).sum() == 1
    assert np.abs(Rn[2] - Rn[4]).max() <= 2.3e-16 and np.abs(tn[2] - tn[4]).max() <= 1.8e-15  # one spacing of a float64 below 1 / below 10
    for b in range(3):
        e3, e2 = orc.per_symmetry(*C.pose_args(near, b))
        assert np.float32(e3[2]) == np.float32(e3[4]) and np.float32(e2[2]) == np.float32(e2[4])  # one fp32 error: the lower row wins


def test_zero_and_camera_cases():
    case = C.zero_case()
    assert np.array_equal(case["R_est"], case["R_gt"]) and np.array_equal(case["t_est"], case["t_gt"])
    assert sorted({len(R) for R, _ in case["transforms"]}) == [1, 4, 36] and len(case["obj_index"]) == 3 * 3 * 30
    for R, t in case["transforms"]:
        assert np.array_equal(R[0], np.eye(3)) and not t[0].any()
    perms = case["R_est"][:24].astype(np.float64)
    assert all(np.array_equal(np.abs(p).sum(0), np.ones(3)) and np.linalg.det(p) > 0 for p in perms)
    err, arg = orc.batch(C.take(case, range(0, 270, 7)))
    assert (err <= 1e-9).all()
    cams = C.cameras(12)
    assert (cams[2::3, 2] != [0, 0, 1]).all() and (cams[:, 0, 0] != cams[:, 1, 1]).all() and (np.abs(cams[:, 0, 1]) > 1).all()
    seen, plain = C.camera_case()
    a, b = orc.batch(seen)[0], orc.batch(plain)[0]
    assert np.array_equal(a[:, 0], b[:, 0]) and (np.abs(a[:, 1:] - b[:, 1:]) > 20 * 2e-5 * np.maximum(1, b[:, 1:])).all()  # a wrong camera entry shows
