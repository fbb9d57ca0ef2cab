"""Seeded inputs of the pose-error tests (lc_metrics.hip), shared by the GPU tests (tests/test_gpu_metrics.py) and the CPU test that
proves the inputs can see the faults they are built for (tests/test_oracle_metrics.py).  Inputs only, plus the two conditions on them that
need nothing but the fp64 oracle (oracle/pose_error_oracle.py).

Witness clouds.  ADI is a mean over M vertices, so a vertex the kernel never visits moves it by 1/M of one neighbour distance: below the
tolerance for a random cloud.  Here the vertices at the indices where the kernel's loops change state (EDGE_K) are witnesses: isolated
points on a sphere of radius WITNESS_RADIUS around the cloud.  A witness skipped as a search target sends its own query to a point about
a witness spacing away; a witness skipped as a query takes (rotation error) x WITNESS_RADIUS out of the sum.  `witness_conditions`
measures both with the oracle, and the tests demand SENSITIVITY x the tolerance for every (pose, edge index)."""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

from oracle import pose_error_oracle as orc

# lc_metrics.hip: 256 threads, a thread's queries are 256 apart (kThreads), it holds 4 (kQ: a query group is 1024), an LDS tile is 1024
# est-pose vertices (kTile), read as pairs (j, j + 1)
EDGE_K = (256, 512, 768, 1024, 2048, 3072, 4096)
WITNESS_COUNTS = (1, 2, 3, 9, 255, 256, 257, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 4095, 4096, 4097, 5000)
WITNESS_RADIUS = 1500.0
BOX = 40.0
SENSITIVITY = 20.0       # a skipped witness moves ADI by at least this many tolerances
FLOAT32_SHARE = 1 / 20   # float32 transforms move ADI by at most this share of the tolerance
# slices of the largest cloud read again by a second set of poses, (first vertex, count) inside that cloud: the same vertices at other
# counts, and at starts that shift the pair slot and the 8- and 16-byte alignment of the first vertex
OVERLAP_SLICES = ((0, 5000), (0, 4097), (0, 1025), (1, 2049), (3, 1026))
# The pose error and the distance.  Float32 rounding of a coordinate grows with the distance and the tolerance with ADI, so the float32
# condition wants a near object and a clear error: at twice the distance and half the rotation error the cloud of 257 vertices sat at
# 0.07 tolerances, over the 1/20 allowed; with these the worst pose sits at 0.012.
ROTVEC_ERR = (0.06, -0.08, 0.04)
T_ERR = (0.5, -0.3, 0.8)
T_GT = (30.0, -20.0, 400.0)
# Clouds of 1, 2 and 3 vertices have no witnesses and no mean to average float32 rounding away: a coordinate near 400 is rounded by up to
# 1.5e-5, a witness's by 6e-5, more than the tolerance of an ADI of a few units.  Their poses are wrong by hundreds of units, so that the tolerance (relative
# above 1) is 20 float32 roundings wide there too.
T_ERR_TINY = (200.0, -150.0, 300.0)


def tol(ref):
    """The project's tolerance for adi, add and te."""
    return 2e-5 * max(1.0, abs(float(ref)))


def edge_indices(M):
    """Indices of a cloud of M vertices at the ends of a thread's stride, a query slot, a tile and a query group, in both pair slots."""
    if M <= 3:
        return []
    idx = {0, 1, 2, 3, M - 2, M - 1}
    for k in EDGE_K:
        idx.update((k - 2, k - 1, k, k + 1))
    return sorted(i for i in idx if 0 <= i < M)


def fibonacci_sphere(n):
    """n unit vectors spread evenly; consecutive ones are a golden angle apart, so neighbours in index are not neighbours in space."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * np.pi * (3 - np.sqrt(5))
    r = np.sqrt(1 - z * z)
    return np.stack((r * np.cos(phi), r * np.sin(phi), z), -1)


def witness_cloud(M, rng, witnesses):
    """(M,3) float32: random in the +-BOX cube, the vertices at `witnesses` on the sphere of WITNESS_RADIUS around the centroid of the rest."""
    pts = (rng.random((M, 3)) * 2 - 1) * BOX
    w = np.asarray(sorted(witnesses), dtype=np.int64)
    if len(w):
        rest = np.delete(pts, w, axis=0)
        centre = rest.mean(0) if len(rest) else np.zeros(3)
        pts[w] = centre + WITNESS_RADIUS * fibonacci_sphere(len(w))
    return pts.astype(np.float32)


def _poses(cnt, seed):
    B = len(cnt)
    Rg = Rotation.random(B, random_state=seed).as_matrix()
    Re = Rg @ Rotation.from_rotvec(ROTVEC_ERR).as_matrix()
    tg = np.tile(np.array(T_GT), (B, 1))
    te = tg + np.where(np.asarray(cnt)[:, None] <= 3, np.array(T_ERR_TINY), np.array(T_ERR))
    return dict(R_est=Re.astype(np.float32), t_est=te.astype(np.float32), R_gt=Rg.astype(np.float32), t_gt=tg.astype(np.float32),
                cnt=np.asarray(cnt, np.int32))


def packed_witness_case():
    """-> dict(pts (P,3) float32, disjoint, overlap).  `disjoint`: one pose per cloud of WITNESS_COUNTS, all clouds in the one packed buffer
    `pts` with single filler vertices between some of them; `overlap`: poses that read OVERLAP_SLICES of the last cloud.  Each set is a
    dict(R_est, t_est, R_gt, t_gt, off (B,) int32, cnt (B,) int32); every vertex at a pose's edge index is a witness."""
    rng = np.random.default_rng(20)
    last = len(WITNESS_COUNTS) - 1
    assert WITNESS_COUNTS[last] == max(WITNESS_COUNTS) and all(s + c <= WITNESS_COUNTS[last] for s, c in OVERLAP_SLICES)
    parts, off, n = [], [], 0
    for i, M in enumerate(WITNESS_COUNTS):
        if i % 3 == 0:  # a filler vertex: the offsets that follow change parity
            parts.append(witness_cloud(1, rng, ()))
            n += 1
        w = set(edge_indices(M))
        if i == last:
            w.update(s + j for s, c in OVERLAP_SLICES for j in edge_indices(c))
        parts.append(witness_cloud(M, rng, w))
        off.append(n)
        n += M
    pts = np.concatenate(parts)
    disjoint = dict(_poses(WITNESS_COUNTS, 21), off=np.array(off, np.int32))
    overlap = dict(_poses([c for _, c in OVERLAP_SLICES], 22), off=np.array([off[last] + s for s, _ in OVERLAP_SLICES], np.int32))
    return dict(pts=pts, disjoint=disjoint, overlap=overlap)


def pose_of(s, i, pts):
    """Pose i of a set as the oracle's arguments: fp64 copies of the float32 inputs, the pose's own vertices."""
    f = lambda a: a[i].astype(np.float64)
    p = pts[s["off"][i]:s["off"][i] + s["cnt"][i]] if "off" in s else pts
    return f(s["R_est"]), f(s["t_est"]), f(s["R_gt"]), f(s["t_gt"]), p.astype(np.float64)


def transform_float32(pts, R, t):
    R, t, p = R.astype(np.float32), t.astype(np.float32), pts.astype(np.float32)
    return np.stack([R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1] + R[r, 2] * p[:, 2] + t[r] for r in range(3)], -1)


def adi_float32(R_est, t_est, R_gt, t_gt, pts):
    """The reference formula with both clouds transformed in float32, the search and the mean in float64: what float32 coordinates cost."""
    est, gt = transform_float32(pts, R_est, t_est), transform_float32(pts, R_gt, t_gt)
    assert est.dtype == np.float32 and gt.dtype == np.float32
    d, _ = cKDTree(est.astype(np.float64)).query(gt.astype(np.float64), k=1)
    return d.mean()


def witness_conditions(s, pts):
    """Per pose of a set, from the oracle alone: dict(M, adi, tol, target, query, f32).  `target`: the least |ADI without est-pose vertex j
    - ADI| over the pose's edge indices j, in tolerances (a gt-pose vertex whose nearest neighbour is j takes its second nearest);
    `query`: the least change of ADI when query j's distance is set to zero, in tolerances; `f32`: |adi_float32 - ADI| in tolerances.
    inf where a pose has no edge index."""
    out = []
    for i in range(len(s["cnt"])):
        a = pose_of(s, i, pts)
        M = len(a[4])
        edges = edge_indices(M)
        d, idx = orc.nearest(*a, k=2) if M > 1 else (orc.nearest(*a)[0][:, None], np.zeros((M, 1), np.int64))
        full = d[:, 0].mean()
        assert full == orc.adi(*a)
        t = tol(full)
        target = min((abs(np.where(idx[:, 0] == j, d[:, -1], d[:, 0]).mean() - full) / t for j in edges), default=np.inf)
        query = min((d[j, 0] / M / t for j in edges), default=np.inf)
        out.append(dict(M=M, adi=full, tol=t, target=target, query=query, f32=abs(adi_float32(*a) - full) / t, edges=len(edges)))
    return out


def assert_witness_conditions(s, pts, label=""):
    """Every pose, every edge index: none is exempt."""
    rows = witness_conditions(s, pts)
    for i, r in enumerate(rows):
        print(f"{label} pose {i}: M={r['M']} edges={r['edges']} adi={r['adi']:.6f} tol={r['tol']:.2e} target x{r['target']:.0f} "
              f"query x{r['query']:.0f} float32 {r['f32']:.4f} tol")
        assert r["edges"] == len(edge_indices(r["M"])) and (r["edges"] > 0) == (r["M"] > 3)
        assert r["target"] >= SENSITIVITY and r["query"] >= SENSITIVITY, (label, i, r)
        assert r["f32"] <= FLOAT32_SHARE, (label, i, r)
    return rows


def symmetric_case(n_fold, base, seed):
    """A jittered ring with an n-fold symmetry about z (vertex m * base + i is vertex i turned by m / n_fold of a turn) and n_fold - 1 poses
    whose estimate is the ground truth composed with each symmetry element but the identity, times a small error: ADD is about the ring's
    size, ADI is about the error, and the nearest est-pose vertex of a gt-pose vertex is another vertex's image."""
    rng = np.random.default_rng(seed)
    ang = rng.random(base) * (2 * np.pi / n_fold)
    rad = 25 + 15 * rng.random(base)
    wedge = np.stack((rad * np.cos(ang), rad * np.sin(ang), (rng.random(base) * 2 - 1) * 20), -1)
    turn = Rotation.from_rotvec(np.array([0, 0, 2 * np.pi / n_fold]))
    pts = np.concatenate([(turn ** m).apply(wedge) for m in range(n_fold)]).astype(np.float32)
    B = n_fold - 1
    Rg = Rotation.random(B, random_state=seed + 1)
    sym = Rotation.concatenate([turn ** m for m in range(1, n_fold)])
    err = Rotation.from_rotvec(rng.normal(size=(B, 3)) * 0.004)
    tg = rng.normal(size=(B, 3)) * 30 + np.array([0, 0, 800.0])
    te = tg + rng.normal(size=(B, 3)) * 0.1
    return dict(pts=pts, R_est=(Rg * sym * err).as_matrix().astype(np.float32), t_est=te.astype(np.float32),
                R_gt=Rg.as_matrix().astype(np.float32), t_gt=tg.astype(np.float32))


def random_rotation_case(M, B, seed):
    """Estimate and ground truth drawn independently and uniformly from SO(3) on a random cloud: the neighbour is never the query's image."""
    rng = np.random.default_rng(seed)
    pts = ((rng.random((M, 3)) * 2 - 1) * BOX).astype(np.float32)
    tg = rng.normal(size=(B, 3)) * 30 + np.array([0, 0, 800.0])
    return dict(pts=pts, R_est=Rotation.random(B, random_state=seed + 1).as_matrix().astype(np.float32),
                t_est=(tg + rng.normal(size=(B, 3)) * 5).astype(np.float32),
                R_gt=Rotation.random(B, random_state=seed + 2).as_matrix().astype(np.float32), t_gt=tg.astype(np.float32))


RE_ANGLES = (("0", 0.0), ("1e-3 rad", 1e-3), ("1 deg", np.deg2rad(1.0)), ("90 deg", np.pi / 2), ("179.9 deg", np.deg2rad(179.9)), ("180 deg", np.pi))


def re_angle_cases(per_angle=6, seed=30):
    """-> names, R_est, R_gt (float32).  Per angle of RE_ANGLES: `per_angle` random ground truths times that angle about a random axis,
    rounded to float32 (so neither matrix is exactly orthonormal), and the identity times that angle about each coordinate axis (a half
    turn about a coordinate axis is exact in float32: exactly 180 degrees)."""
    rng = np.random.default_rng(seed)
    names, Re, Rg = [], [], []
    for name, a in RE_ANGLES:
        g = Rotation.random(per_angle, random_state=int(rng.integers(1 << 30))).as_matrix()
        axes = rng.normal(size=(per_angle, 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        for k in range(per_angle):
            names.append(f"{name} random {k}")
            Rg.append(g[k])
            Re.append(g[k] @ Rotation.from_rotvec(axes[k] * a).as_matrix())
        for k in range(3):
            names.append(f"{name} about axis {k} from the identity")
            Rg.append(np.eye(3))
            Re.append(Rotation.from_rotvec(np.eye(3)[k] * a).as_matrix())
    return names, np.stack(Re).astype(np.float32), np.stack(Rg).astype(np.float32)


def proper_signed_permutations():
    """The 24 rotation matrices with entries in {0, 1, -1}: the only rotations float32 holds exactly."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = -1.0 if signs >> r & 1 else 1.0
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return np.stack(out).astype(np.float32)


def quaternion_rep_to_RT_f64(states):
    """(B,7) w,x,y,z,tx,ty,tz -> R (B,3,3), t (B,3) in float64 with the convention lc_amd/transforms.py documents: two_s = 2 / ||q||, the
    reference's own (not 2 / ||q||^2), so a quaternion of length s gives (1 - s) I + s R(q / s), a rotation only for s = 1."""
    q = states[:, :4].astype(np.float64)
    r, i, j, k = q.T
    two_s = 2.0 / np.linalg.norm(q, axis=1)
    R = np.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1).reshape(-1, 3, 3)
    return R, states[:, 4:7].astype(np.float64)


def states_case(B=8, M=900, seed=40):
    """(B,7) float32 estimates and ground truths and a cloud.  The estimates' quaternions have lengths in [0.7, 1.4] but for the first two;
    the ground truths' are unit length in the first `unit_gt` poses (what a data set holds, and where R_gt^T is inv(R_gt)) and have such
    lengths in the rest."""
    rng = np.random.default_rng(seed)
    qg = Rotation.random(B, random_state=seed + 1)
    qe = qg * Rotation.from_rotvec(rng.normal(size=(B, 3)) * 0.2)
    wxyz = lambda r: r.as_quat()[:, [3, 0, 1, 2]]
    sg, se = rng.uniform(0.7, 1.4, (B, 1)), rng.uniform(0.7, 1.4, (B, 1))
    unit_gt = B // 2
    sg[:unit_gt] = 1.0
    se[:2] = 1.0
    tg = rng.normal(size=(B, 3)) * 30 + np.array([0, 0, 800.0])
    te = tg + rng.normal(size=(B, 3)) * 5
    pts = ((rng.random((M, 3)) * 2 - 1) * BOX).astype(np.float32)
    return dict(pts=pts, states_est=np.concatenate((wxyz(qe) * se, te), 1).astype(np.float32),
                states_gt=np.concatenate((wxyz(qg) * sg, tg), 1).astype(np.float32), unit_gt=unit_gt)
