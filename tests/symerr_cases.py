"""Seeded inputs of the symmetry-aware pose-error tests (lc_sym_metrics.hip), shared by the GPU tests (tests/test_gpu_symerr.py), the CPU
tests that prove the inputs can see the faults they are built for (tests/test_symerr_oracle.py) and the golden generator
(tests/golden/gen_golden_symerr.py).  Inputs only, plus the conditions on them that need nothing but the fp64 oracle.

A case is a dict: R_est, R_gt (B,3,3), t_est, t_gt (B,3), cam_K (B,3,3), pts (P,3) float32; pts_off, pts_cnt, obj_index (B,) int32;
transforms: per object (R_s (K,3,3), t_s (K,3)) float64, object i being table index i (obj_ids = 0, 1, ...).

The edge lists are DERIVED from the constants of lc_sym_metrics.hip and lc_sym_metrics_args.h, restated here:
  WAVE = 64 lanes stride the vertices, UNROLL = 2 vertices per lane and trip (a trip covers 128), there is no LDS tile;
  WAVES = 4 wavefronts of a workgroup take the symmetries k0 + wave, k0 + wave + 4 of a chunk of CHUNK = 8."""
import numpy as np

from tests import symerr_oracle as orc

WAVE, UNROLL, WAVES, CHUNK = 64, 2, 4, 8
SENSITIVITY = 20.0  # a dropped vertex / symmetry moves the error by at least this many tolerances
BOX = 40.0
# vertex counts: the issue's 1, 2, 63, 64, 65, then each side of one trip (128) and of two (256), and one a few vertices beyond a trip
VERTEX_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 133, 257)
# symmetry counts: 1, 2, 3, each wave edge (4) and chunk edge (8, 16) +- 1, up to one beyond two chunks
SYM_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
ROTVEC_ERR = (0.06, -0.08, 0.04)
T_ERR = (0.5, -0.3, 0.8)


def tol(ref):
    """tests/metrics_cases.tol: the project's tolerance for a metric."""
    return 2e-5 * max(1.0, abs(float(ref)))


def vertex_edges(M):
    """Indices at which the kernel's vertex loop changes state: both ends, and each multiple of the lane stride (64: every second one is a
    multiple of the trip, 128) with its neighbours."""
    idx = {0, 1, M - 2, M - 1}
    for m in range(WAVE, M + WAVE, WAVE):
        idx.update((m - 1, m, m + 1))
    return sorted(i for i in idx if 0 <= i < M)


def symmetry_edges(K):
    """Symmetry indices at both ends of an object's rows and at each wave edge (multiples of 4: every second one a chunk edge) +- 1."""
    idx = {0, 1, K - 2, K - 1}
    for m in range(WAVES, K + WAVES, WAVES):
        idx.update((m - 1, m, m + 1))
    return sorted(k for k in idx if 0 <= k < K)


def rodrigues(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    n = v / a
    Kx = np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_transforms(rng, K):
    """The identity and K - 1 random rigid transforms: far from each other, so the runner-up of a pose is far from its winner."""
    R = np.stack([np.eye(3)] + [rot(rng) for _ in range(K - 1)])
    t = np.concatenate((np.zeros((1, 3)), rng.uniform(-10, 10, (K - 1, 3))))
    return R, t


def lm_camera(B):
    return np.tile(np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]]), (B, 1, 1))


def _case(Re, te, Rg, tg, K, pts, off, cnt, obj, transforms):
    f = lambda a: np.ascontiguousarray(a, np.float32)
    i = lambda a: np.ascontiguousarray(a, np.int32)
    return dict(R_est=f(Re), t_est=f(te), R_gt=f(Rg), t_gt=f(tg), cam_K=f(K), pts=f(pts), pts_off=i(off), pts_cnt=i(cnt), obj_index=i(obj),
                transforms=[(np.asarray(R, np.float64), np.asarray(t, np.float64)) for R, t in transforms])


def compose_estimate(Rg, tg, Rs, ts, rotvec_err, t_err):
    """The ground truth composed with a symmetry, then a small error: the symmetry is the one the minimum picks."""
    return Rg @ Rs @ rodrigues(rotvec_err), Rg @ ts + tg + np.asarray(t_err)


def pose_args(case, b, drop_vertex=None, drop_symmetry=None):
    """Pose b as the oracle's arguments: float64 copies of the float32 inputs, the pose's own vertices and its object's transforms."""
    w = lambda a: a[b].astype(np.float64)
    p = case["pts"][case["pts_off"][b]:case["pts_off"][b] + case["pts_cnt"][b]].astype(np.float64)
    R_s, t_s = case["transforms"][case["obj_index"][b]]
    if drop_vertex is not None:
        p = np.delete(p, drop_vertex, axis=0)
    if drop_symmetry is not None:
        R_s, t_s = np.delete(R_s, drop_symmetry, axis=0), np.delete(t_s, drop_symmetry, axis=0)
    return w(case["R_est"]), w(case["t_est"]), w(case["R_gt"]), w(case["t_gt"]), w(case["cam_K"]), p, R_s, t_s


def take(case, idx):
    """The poses `idx` of a case, in that order (same buffers)."""
    idx = np.asarray(idx, np.int64)
    out = dict(case)
    for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts_off", "pts_cnt", "obj_index"):
        out[k] = np.ascontiguousarray(case[k][idx])
    return out


def merge(a, b):
    """Both cases as one batch over one vertex buffer and one object list (a's poses first)."""
    out = {k: np.concatenate((a[k], b[k])) for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts", "pts_cnt")}
    out["pts_off"] = np.concatenate((a["pts_off"], b["pts_off"] + len(a["pts"]))).astype(np.int32)
    out["obj_index"] = np.concatenate((a["obj_index"], b["obj_index"] + len(a["transforms"]))).astype(np.int32)
    out["transforms"] = list(a["transforms"]) + list(b["transforms"])
    return out


def vertex_edge_case():
    """One pose per (M of VERTEX_COUNTS, edge index e of vertex_edges(M)): a cloud of M vertices whose far outlier (ten times as far from
    the origin as the rest) sits at e, so that e alone decides both maxima.  All clouds lie in one packed buffer; a filler vertex after every third cloud changes the parity of the
    offsets that follow.  Objects with 1, 2 and 5 transforms take turns."""
    rng = np.random.default_rng(501)
    transforms = [random_transforms(rng, K) for K in (1, 2, 5)]
    parts, off, cnt, obj, edge, Rg, n = [], [], [], [], [], [], 0
    axis = np.asarray(ROTVEC_ERR)
    for M in VERTEX_COUNTS:
        for e in vertex_edges(M):
            p = (rng.random((M, 3)) * 2 - 1) * BOX
            g = rot(rng)
            while True:  # the outlier: across the axis of the rotation error, and moved by that error mostly ACROSS the line of sight
                d = np.cross(axis, rng.normal(size=3))
                d *= 400.0 / np.linalg.norm(d)
                moved = g @ np.cross(axis, d)
                if np.hypot(moved[0], moved[1]) >= 0.7 * np.linalg.norm(moved):
                    break
            p[e] = d
            if len(off) % 3 == 2:
                parts.append((rng.random((1, 3)) * 2 - 1) * BOX)
                n += 1
            parts.append(p)
            off.append(n)
            cnt.append(M)
            obj.append(len(off) % 3)
            edge.append(e)
            Rg.append(g)
            n += M
    B = len(off)
    assert len({o % 2 for o in off}) == 2
    Rg = np.stack(Rg)
    tg = np.stack((rng.uniform(-60, 60, B), rng.uniform(-60, 60, B), rng.uniform(1400, 1600, B)), -1)
    Re, te = zip(*(compose_estimate(Rg[b], tg[b], np.eye(3), np.zeros(3), ROTVEC_ERR, T_ERR) for b in range(B)))
    case = _case(np.stack(Re), np.stack(te), Rg, tg, lm_camera(B), np.concatenate(parts), off, cnt, obj, transforms)
    case["edge"] = np.asarray(edge)
    return case


def vertex_conditions(case):
    """Per pose: by how many tolerances dropping its edge vertex moves mssd and mspd (a cloud of one vertex: down to 0)."""
    rows = []
    for b, e in enumerate(case["edge"]):
        full = orc.errors(*pose_args(case, b))
        less = orc.errors(*pose_args(case, b, drop_vertex=int(e))) if case["pts_cnt"][b] > 1 else (0.0, 0.0)
        rows.append(dict(M=int(case["pts_cnt"][b]), edge=int(e), mssd=abs(full[0] - less[0]) / tol(full[0]), mspd=abs(full[1] - less[1]) / tol(full[1])))
    return rows


def symmetry_edge_case():
    """One pose per (K of SYM_COUNTS, edge index k of symmetry_edges(K)): the estimate is the ground truth composed with symmetry k of an
    object of K random rigid transforms, plus a small error, so symmetry k wins both minima.  One cloud of 37 vertices for every pose."""
    rng = np.random.default_rng(502)
    M = 37
    pts = (rng.random((M, 3)) * 2 - 1) * BOX
    transforms = [random_transforms(rng, K) for K in SYM_COUNTS]
    Re, te, Rg, tg, obj, win = [], [], [], [], [], []
    for o, K in enumerate(SYM_COUNTS):
        for k in symmetry_edges(K):
            g, t = rot(rng), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(700, 900)])
            e = compose_estimate(g, t, transforms[o][0][k], transforms[o][1][k], rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.4)
            Re.append(e[0]); te.append(e[1]); Rg.append(g); tg.append(t); obj.append(o); win.append(k)
    B = len(obj)
    case = _case(np.stack(Re), np.stack(te), np.stack(Rg), np.stack(tg), lm_camera(B), pts, [0] * B, [M] * B, obj, transforms)
    case["win"] = np.asarray(win)
    return case


def symmetry_conditions(case):
    """Per pose: the winner the oracle finds for each error, by how many tolerances dropping row `win` moves mssd and mspd, and how many
    tolerances the runner-up lies above the winner (inf for K = 1: there is nothing to confuse it with)."""
    rows = []
    for b, k in enumerate(case["win"]):
        e3, e2 = orc.per_symmetry(*pose_args(case, b))
        r = dict(K=len(e3), win=int(k), k3=int(np.argmin(e3)), k2=int(np.argmin(e2)))
        for name, e in (("mssd", e3), ("mspd", e2)):
            rest = np.delete(e, int(k))
            r[name] = (rest.min() - e[int(k)]) / tol(e[int(k)]) if len(rest) else np.inf  # dropping row k: the minimum becomes the runner-up
        rows.append(r)
    return rows


def tie_case(last_bit=False):
    """An object of 6 transforms whose rows 2 and 4 are bit-identical copies (last_bit: row 4 differs from row 2 in the last bit of one
    rotation entry and of one translation entry) and win: three poses, estimate = ground truth composed with row 2 plus a small error."""
    rng = np.random.default_rng(503)
    R, t = random_transforms(rng, 6)
    R[4], t[4] = R[2], t[2]
    if last_bit:
        R[4, 1, 2] = np.nextafter(R[4, 1, 2], 2.0)
        t[4, 0] = np.nextafter(t[4, 0], -100.0)
    pts = (rng.random((150, 3)) * 2 - 1) * BOX
    Re, te, Rg, tg = [], [], [], []
    for _ in range(3):
        g, tt = rot(rng), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(700, 900)])
        e = compose_estimate(g, tt, R[2], t[2], rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.4)
        Re.append(e[0]); te.append(e[1]); Rg.append(g); tg.append(tt)
    return _case(np.stack(Re), np.stack(te), np.stack(Rg), np.stack(tg), lm_camera(3), pts, [0] * 3, [150] * 3, [0] * 3, [(R, t)])


def lowest_fp32_winner(e, got_bits):
    """The oracle evaluated on the bits the kernel returned: the lowest k whose fp64 error, rounded to fp32, is not above the returned
    error (the kernel's rule: least fp32 error, lowest k among equals)."""
    got = np.asarray(got_bits, np.float32)
    return int(np.nonzero(e.astype(np.float32) <= got)[0][0])


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
    return np.stack(out)


def bop_objects(steps=36):
    """Objects with K = 1, 2, 4 and `steps` transforms through lc_amd.symmetry.symmetry_transforms: none, a half turn with a shift, the
    quarter turns about z, and a continuous axis (off every coordinate axis) with an offset."""
    from lc_amd import symmetry

    def disc(R, t):
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = R, t
        return S.ravel().tolist()

    half = [disc(np.diag([-1.0, -1, 1]), [3.0, -2.0, 0.0])]
    quarter = [disc(rodrigues([0, 0, q * np.pi / 2]), [0.0, 0, 0]) for q in (1, 2, 3)]
    cont = [{"axis": [0.48, -0.6, 0.64], "offset": [4.0, -7.0, 11.0]}]
    infos = [{}, {"symmetries_discrete": half}, {"symmetries_discrete": quarter}, {"symmetries_continuous": cont}]
    return infos, [symmetry.symmetry_transforms(i, steps) for i in infos]


def golden_inputs():
    """The inputs of tests/golden/sym_err_b12_m700.npz: 12 poses, 700 vertices, objects with K = 1, 2, 4 and 36 (three poses each); the
    estimate is the ground truth composed with one of the object's symmetries plus an error of a few degrees and millimetres."""
    rng = np.random.default_rng(20261020)
    infos, transforms = bop_objects(36)
    M, B = 700, 12
    pts = (rng.random((M, 3)) * 2 - 1) * np.array([45.0, 30.0, 60.0])
    obj = np.repeat(np.arange(4), 3)
    Re, te, Rg, tg = [], [], [], []
    for b in range(B):
        R_s, t_s = transforms[obj[b]]
        k = int(rng.integers(len(R_s)))
        g, t = rot(rng), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1100)])
        e = compose_estimate(g, t, R_s[k], t_s[k], rng.normal(size=3) * 0.03, rng.normal(size=3) * 2.0)
        Re.append(e[0]); te.append(e[1]); Rg.append(g); tg.append(t)
    return _case(np.stack(Re), np.stack(te), np.stack(Rg), np.stack(tg), lm_camera(B), pts, [0] * B, [M] * B, obj, transforms), infos


def golden_case(z):
    """The case dict of a loaded sym_err_*.npz (its transforms formed again by lc_amd.symmetry from the stored model infos)."""
    import json

    from lc_amd import symmetry

    infos = json.loads(str(z["models_info"]))
    tr = [symmetry.symmetry_transforms(i, int(z["steps"])) for i in infos]
    B, M = z["R_est"].shape[0], z["pts"].shape[0]
    return _case(z["R_est"], z["t_est"], z["R_gt"], z["t_gt"], z["cam_K"], z["pts"], [0] * B, [M] * B, z["obj_index"], tr)


def zero_case():
    """est = gt: the 24 signed permutations and 6 random rotations, for each K in {1, 4, 36} and each M in {1, 255, 1025}."""
    rng = np.random.default_rng(504)
    _, transforms = bop_objects(36)
    transforms = [transforms[0], transforms[2], transforms[3]]
    counts = (1, 255, 1025)
    pts = (rng.random((sum(counts), 3)) * 2 - 1) * BOX
    starts = np.cumsum((0,) + counts[:-1])
    rots = np.concatenate((proper_signed_permutations(), np.stack([rot(rng) for _ in range(6)])))
    R, t, off, cnt, obj = [], [], [], [], []
    for o in range(3):
        for s, c in zip(starts, counts):
            for g in rots:
                R.append(g); off.append(s); cnt.append(c); obj.append(o)
                t.append([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(700, 900)])
    B = len(R)
    return _case(np.stack(R), np.asarray(t), np.stack(R), np.asarray(t), lm_camera(B), pts, off, cnt, obj, transforms)


def cameras(B):
    """(B,3,3) float64: the "bop" and "stress" cameras of lc_amd.synth (fx != fy, skew, principal point off the centre, behind an in-plane
    rotation) in turn with a K whose third row is not (0, 0, 1)."""
    import torch

    from lc_amd import synth

    rng = np.random.default_rng(505)
    f = torch.from_numpy(rng.uniform(500, 900, B))
    th = torch.from_numpy(rng.uniform(-0.5, 0.5, B))
    cx, cy = torch.from_numpy(rng.uniform(280, 360, B)), torch.from_numpy(rng.uniform(200, 280, B))
    K = np.stack([synth.crop_camera(f, th, cx, cy, camera=c).numpy() for c in ("bop", "stress")])
    out = np.stack([K[b % 2, b] for b in range(B)])
    for b in range(2, B, 3):
        out[b, 2] = [2e-4, -1e-4, 1.1]
    return out


def camera_case():
    """The poses of golden_inputs() seen through cameras(12)."""
    case, _ = golden_inputs()
    plain = dict(case)
    case = dict(case, cam_K=np.ascontiguousarray(cameras(12), np.float32))
    return case, plain
