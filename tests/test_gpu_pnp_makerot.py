"""make_rot (lc_pnp_body.h) takes the small-angle case of ceres/rotation.h by a scalar branch: the small arm sets the coefficients of
R = I + [aa]x, the large arm is the arithmetic without selects and with fast_sqrt_rsqrt_pos.  What such a change could get wrong is WHICH arm
an evaluation takes, what the arm taken leaves behind for the next evaluation, and the bits of either arm, so the cases are starts on both
sides of the threshold th2 > DBL_EPSILON, batches that mix the arms, and angles across the pi/2 reduction of sincos_small.  Every case
compares by bits the three builds of the one-correspondence-per-lane solve -- the team solve stand-alone, the team solve through
lc_pose_unit2_f32, the one-wave large-grid build (tests/test_gpu_pnp_lmstep.py: _three_builds) -- and then the CPU oracle with that file's
rule: rets, iters and result_tr EXACTLY on problems whose oracle result does not hang on its own rounding (CPU tests here check that for
every case), the poses at that file's POSE_TOL.

The problems are made for their starts: the true rotation is the start's angle-axis plus 0.05 rad about another axis, 1 px of noise, so the
solve is short and well conditioned from either arm.

  * "identity": the start quaternion is exactly (1, 0, 0, 0): th2 == 0, the small arm in evaluation 0, the large arm from the first
    candidate on;
  * "below" / "above": quaternions (1, q1, 0, 0) with q1 the fp32 numbers next to 2^-27 on either side; the angle-axis is 2 atan(q1) / q1 * q1,
    so th2 lies 1.2e-7 (relative) below and above DBL_EPSILON = 2^-52 -- a margin eight orders above the 7e-16 of the device's conversion
    (lc_common.h: atan_ratio_pos); test_the_starts_land_on_their_sides shows it with the conversion in fp64.  There is no "at" case:
    th2 == DBL_EPSILON needs q1 = 2^-27 (1 + 2^-55 / 3) to the last bit of the conversion, and fp32 has 2^-27 and its neighbours 6e-8 away;
  * "mixed-1" / "mixed-2": batches of three with one small and two large starts, and two small and one large: the arms do not leak between
    workgroups;
  * "q0", "q1", "q2": angles 0.7, 1.9 and 3.0 rad -- kf = rint(th 2 / pi) = 0, 1, 2 -- and "edge": an angle within 1e-6 of pi / 2.

Three cases of the issue cannot be built, for one reason: the API takes a quaternion, and its angle-axis has a norm of at most pi.  So no
start reaches the fourth quadrant of the reduction (th >= 5 pi / 4), and none reaches th >= 1e4, the full-range sincos call
(tests/test_gpu_pnp_onebody.py pins that call on a probe kernel, for the same reason); a candidate of the loop could, but only in a solve
that has left every basin.  A NaN and an inf in `start` are here: both make th2 NaN, which is the small arm, and fail the initial evaluation.

The exact comparison is made where it is fair, which the CPU tests of this file establish without the device: DATA_SEEDS has the two
criteria and the reason for the second one."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_pnp_lmstep import _assert_oracle, _oracle, _reordered, _three_builds

BS, NS, MAX_ITERS = (1, 3), (3, 4, 64), (1, 50)
EPS = float(np.finfo(np.float64).eps)
Q_BELOW, Q_ABOVE = float(np.nextafter(np.float32(2.0 ** -27), np.float32(0))), float(np.nextafter(np.float32(2.0 ** -27), np.float32(1)))


def _quat(aa):
    th = np.linalg.norm(aa)
    return np.array([1.0, 0, 0, 0]) if th == 0 else np.concatenate(([math.cos(th / 2)], np.asarray(aa) / th * math.sin(th / 2)))


# the start quaternions of a case, poses 0..2 (fp64 here, rounded to fp32 by _problem)
STARTS = {
    "identity": [np.array([1.0, 0, 0, 0])] * 3,
    "below": [np.array([1.0, Q_BELOW, 0, 0]), np.array([1.0, 0, Q_BELOW, 0]), np.array([1.0, 0, 0, -Q_BELOW])],
    "above": [np.array([1.0, Q_ABOVE, 0, 0]), np.array([1.0, 0, Q_ABOVE, 0]), np.array([1.0, 0, 0, -Q_ABOVE])],
    "mixed-1": [_quat([0.3, -0.2, 0.4]), np.array([1.0, 0, 0, 0]), _quat([-0.5, 0.1, 0.2])],
    "mixed-2": [np.array([1.0, Q_BELOW, 0, 0]), _quat([0.3, -0.2, 0.4]), np.array([1.0, 0, 0, 0])],
    "q0": [_quat(0.7 * np.array(a) / np.linalg.norm(a)) for a in ([1, 2, 2], [2, -1, 2], [-2, 2, 1])],
    "q1": [_quat(1.9 * np.array(a) / np.linalg.norm(a)) for a in ([1, 2, 2], [2, -1, 2], [-2, 2, 1])],
    "q2": [_quat(3.0 * np.array(a) / np.linalg.norm(a)) for a in ([1, 2, 2], [2, -1, 2], [-2, 2, 1])],
    "edge": [_quat((math.pi / 2 + d) * np.array(a) / np.linalg.norm(a)) for a, d in (([1, 2, 2], 4e-7), ([2, -1, 2], -4e-7), ([-2, 2, 1], 0.0))],
}
SMALL = {"identity": (True,) * 3, "below": (True,) * 3, "above": (False,) * 3, "mixed-1": (False, True, False), "mixed-2": (True, False, True)}


def _angle_axis(q):
    """ceres/rotation.h QuaternionToAngleAxis in fp64, of the fp32 quaternion the API is given"""
    q = np.asarray(q, np.float32).astype(np.float64)
    s = math.sqrt(q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
    if s == 0:
        return 2.0 * q[1:]
    return q[1:] * (2.0 * (math.atan2(-s, -q[0]) if q[0] < 0 else math.atan2(s, q[0])) / s)


def _rot(aa):
    th = np.linalg.norm(aa)
    if th == 0:
        return np.eye(3)
    k = np.asarray(aa) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


# The seed of the problem data per (B, N): the first for which the oracle qualifies for an exact comparison in EVERY case of that shape, by
# two criteria that need no device.  (1) As in tests/test_gpu_pnp_lmstep.py: the same rets, iters and result_tr under eight reorderings of
# the correspondences (sums that round differently).  (2) For the poses that start in the small arm: the same rets, iters and result_tr
# from each of the seven small starts NUDGES -- the identity and 2^-27 (1 - 2^-24) about +-x, +-y, +-z, 1.5e-8 rad apart.  The reason is
# a difference between the models, not between their roundings: in the small arm the oracle's Jacobian is -[X]x, the exact derivative of
# X + aa x X, and the device's is -[R X]x with R = I + [aa]x (lc_pnp_body.h: Rot), 1.5e-8 away for such a start; rho and the radius follow,
# and an ulp of the fp32 result_tr is 6e-8.  A problem whose oracle gives another result_tr when the start itself moves by that much sits
# next to a rounding boundary of result_tr, and an exact comparison on it tests the boundary, not the solve: seed 0 at (3, 3) is one
# (its oracle returns 22982.31, 22982.312 and 22982.314 for pose 2 over the seven starts).  test_the_oracle_does_not_depend_on_a_nudge_of_a_small_start checks (2).
DATA_SEEDS = {(3, 3): 1}  # every other shape: seed 0


@functools.lru_cache(maxsize=None)
def _problem(name, B, N, seed=None):
    """B poses started at STARTS[name]; the true pose of each lies 0.05 rad and 3 % of the distance away"""
    seed = DATA_SEEDS.get((B, N), 0) if seed is None else seed
    rng = np.random.default_rng(1000 * N + B + 100000 * seed)
    X = rng.uniform(-40, 40, (B, N, 3))
    K = np.tile(np.array([[300.0, 0, 32], [0, 300, 32], [0, 0, 1]]), (B, 1, 1))
    start, pose, U = np.zeros((B, 7)), np.zeros((B, 7)), np.zeros((B, N, 2))
    for i in range(B):
        q = STARTS[name][i]
        aa = _angle_axis(q)
        R = _rot(aa) @ _rot(0.05 * np.roll(np.array([0.6, -0.64, 0.48]), i))
        t = np.array([10.0 * i - 8, 5.0 - 7 * i, 700.0 + 90 * i])
        xc = X[i] @ R.T + t
        U[i] = (xc @ K[i].T)[:, :2] / xc[:, 2:3] + rng.normal(0, 1.0, (N, 2))
        start[i] = np.concatenate((q, t * 1.03))
        pose[i, 4:] = t
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(K=f32(K), pose=f32(start), pts3d=f32(X), pts2d=f32(U), inv_std=f32(rng.uniform(0.5, 1.5, (B, N, 2))),
                bbox_3d=f32(np.tile(np.array([[sx, sy, sz] for sx in (-40, 40) for sy in (-40, 40) for sz in (-40, 40)], float), (B, 1, 1))), start=f32(start))


CASES = [(name, B, N) for name in STARTS for B in BS for N in NS]
NUDGES = [np.array([1.0, 0, 0, 0])] + [np.array([1.0] + [sg * Q_BELOW if a == ax else 0.0 for a in range(3)]) for ax in range(3) for sg in (1, -1)]


def _nudged(case, k):
    """the problem of `case` with every small start replaced by NUDGES[k]; the correspondences stay"""
    b = {key: v.clone() for key, v in case[0](*case[1:]).items()}
    for i in range(b["start"].shape[0]):
        if SMALL[case[1]][i]:
            b["start"][i, :4] = torch.from_numpy(NUDGES[k].astype(np.float32))
    return b


def test_the_starts_land_on_their_sides():
    """CPU: th2 of every start of the threshold cases against DBL_EPSILON, by a margin far above the error of the device's conversion; the
    quadrants of the others"""
    for name, small in SMALL.items():
        for q, sm in zip(STARTS[name], small):
            th2 = float((_angle_axis(q) ** 2).sum())
            assert (not th2 > EPS) == sm and (th2 == 0 or abs(th2 / EPS - 1) > 1e-8), (name, th2)
    assert 0 < 1 - float((_angle_axis(STARTS["below"][0]) ** 2).sum()) / EPS < 2e-7 and 0 < float((_angle_axis(STARTS["above"][0]) ** 2).sum()) / EPS - 1 < 3e-7
    for name, kf in (("q0", 0), ("q1", 1), ("q2", 2), ("edge", 1)):
        for q in STARTS[name]:
            assert round(np.linalg.norm(_angle_axis(q)) * 2 / math.pi) == kf
    assert all(abs(np.linalg.norm(_angle_axis(q)) - math.pi / 2) < 1e-6 for q in STARTS["edge"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_oracle_does_not_depend_on_the_order_of_its_sums(case):
    """CPU: rets, iters and result_tr of the oracle are the same for eight reorderings of the correspondences, at both budgets -- what makes
    the exact comparison of the GPU tests a fair one"""
    N = case[-1]
    g = torch.Generator().manual_seed(1)
    perms = [tuple(torch.randperm(N, generator=g).tolist()) for _ in range(8)]
    for max_iter in MAX_ITERS:
        _, tr, ret, iters, _, _ = _oracle((_problem, *case), max_iter)
        assert max_iter == 1 or not ret.any()
        for perm in perms:
            _, tr2, ret2, iters2, _, _ = _oracle((_reordered, (_problem, *case), perm), max_iter)
            assert np.array_equal(ret, ret2) and np.array_equal(iters, iters2) and np.array_equal(tr, tr2), max_iter


def _nudge_stable(case):
    for max_iter in MAX_ITERS:
        _, tr, ret, iters, _, _ = _oracle((_problem, *case), max_iter)
        for k in range(len(NUDGES)):
            _, tr2, ret2, iters2, _, _ = _oracle((_nudged, (_problem, *case), k), max_iter)
            if not (np.array_equal(ret, ret2) and np.array_equal(iters, iters2) and np.array_equal(tr, tr2)):
                return False
    return True


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in SMALL and any(SMALL[c[0]][:c[1]])], ids=lambda c: "-".join(map(str, c)))
def test_the_oracle_does_not_depend_on_a_nudge_of_a_small_start(case):
    """CPU: criterion (2) of DATA_SEEDS"""
    assert _nudge_stable(case)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_both_arms(case, max_iter):
    team = _three_builds(_problem(*case), max_iter)
    _assert_oracle(team, _oracle((_problem, *case), max_iter))
    if max_iter == 50:
        assert not team[2].any() and int(team[3].min()) >= 2  # converged, past the first candidate: both arms where the start is small


@pytest.mark.gpu
@pytest.mark.parametrize("N", (4, 64))
def test_a_non_finite_start(N):
    """a NaN and an inf in the start's rotation: th2 is NaN, the small arm, the initial evaluation fails; rets = 1 after no iteration, the
    start comes back, and the pose between them is solved as if they were not there"""
    b = {k: v.clone() for k, v in _problem("mixed-1", 3, N).items()}
    b["start"][0, 1], b["start"][2, 3] = float("nan"), float("inf")
    team = _three_builds(b)
    ref = _three_builds(_problem("mixed-1", 3, N))
    assert team[2].tolist() == [1, int(ref[2][1]), 1] and team[3].tolist() == [0, int(ref[3][1]), 0]
    assert torch.equal(team[0].cpu().view(torch.int32), torch.cat((b["start"][:1], ref[0][1:2].cpu(), b["start"][2:])).view(torch.int32))
