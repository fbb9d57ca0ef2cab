"""The team solve sums each wave's 14 entries of J^T J | J^T r | r^T r over the 64 lanes and hands the totals to the sibling wave
(lc_common.h).  Whatever form that sum takes -- through LDS slots (block_sum_team2) or by cross-lane exchanges in registers
(block_sum_team2_reg over shared/lc_shared.h: wave_reduce_scatter_lds_order) -- every total must be added up in the one-wave LDS
tree's order: lane xor 16, 8, 4, 2, 1, then 32.  The large-grid build (one wavefront per pose, more than 1024 poses in a launch) runs that
tree, so the team results must be its results bit for bit: states, result_tr, rets, iters.

The team form is reached through the small-grid stand-alone solve and through lc_pose_unit2_f32.  Rows are cut short by `counts` in the
stand-alone solve; the pose unit's C ABI has no counts, there the same rows end in correspondences with a zero information factor
(pnp_sqrt_diag is an argument of its own), which is what the padding lanes of a short row are inside the kernel: exact zeros in every sum.
N takes every exchange width's edge from both sides (4, 8, 16, 32, 64 lanes), max_iter 1 and 50.

Probes: a single correspondence with information on lane 2^s and on lane 2^s - 1 for every exchange stage s (a lane dropped or taken twice
changes every total); information factors of 1e8 beside 1, so that J^T J has terms of 1e16 beside 1 and J^T r terms of +-1e16 beside +-1
-- a total then depends on which partial sums meet at which level, i.e. on the pairing, not only on the set of lanes; and a NaN, +inf or
-inf on each lane of one quad, which must fail the job exactly as the large-grid build fails it."""
import functools

import pytest
import torch

from tests.test_gpu_pnp_team_sum import _args, _assert_same, _batch, _cut, _dev, _solve, _solve_one_wave

pytestmark = pytest.mark.gpu

BS = (1, 3)
NS = (3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
MAX_ITERS = (1, 50)


def _zero_tail(W, counts):
    """the information factors with every correspondence behind counts[b] set to zero"""
    keep = torch.arange(W.shape[1], device=W.device)[None, :] < counts[:, None]
    return (W * keep[..., None]).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(B, N, cut, max_iter, by_weight):
    """the large-grid build's results, computed once per case and left unchanged"""
    K, X, U, W, start = _args(_batch(B, N))
    counts = _cut(B, N) if cut else None
    if by_weight and cut:
        W, counts = _zero_tail(W, counts), None
    return _solve_one_wave(K, X, U, W, start, counts, max_iter_count=max_iter)


def _pose_unit(b, W, max_iter):
    """lc_pose_unit2_f32 with the solve's information factors W (the loss half keeps the batch's own)"""
    from lc_amd import _lib
    from lc_amd.fused import PoseUnit

    B, N = W.shape[:2]
    u = PoseUnit(B, N, _dev())
    P = _lib.ptr
    rc = _lib.load().lc_pose_unit2_f32(P(b["K"]), P(b["pose"]), P(b["pts3d"]), P(b["pts2d"]), P(b["inv_std"]), None, P(b["bbox_3d"]), None, B, N,
                                       32.0, 3.0, 4.0, P(u.loss), P(u.d_pts2d), P(u.d_inv_std), P(u.d_pts3d), P(W), P(b["start"]), P(u.states),
                                       P(u.trust_radius), P(u.invalid), P(u.iters), int(max_iter), 1e-6, None, 0, _lib.stream_ptr(_dev()))
    _lib.check(rc, "lc_pose_unit2_f32")
    return u.states, u.trust_radius, u.invalid, u.iters


@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("cut", (False, True), ids=("full", "cut"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_stand_alone_solve_keeps_the_one_wave_bits(B, N, cut, max_iter):
    counts = _cut(B, N) if cut else None
    team = _solve(*_args(_batch(B, N)), counts, max_iter_count=max_iter)
    _assert_same(team, _reference(B, N, cut, max_iter, False))
    assert int(team[3].max()) == 1 if max_iter == 1 else int(team[3].max()) >= 1


@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("cut", (False, True), ids=("full", "cut"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_pose_unit_keeps_the_one_wave_bits(B, N, cut, max_iter):
    b = _batch(B, N)
    W = _zero_tail(b["inv_std"], _cut(B, N)) if cut else b["inv_std"]
    team = _pose_unit(b, W, max_iter)
    _assert_same(team, _reference(B, N, cut, max_iter, True))
    assert int(team[3].max()) == 1 if max_iter == 1 else int(team[3].max()) >= 1


def _both_ways(b, W, U=None):
    """stand-alone and pose unit against the large-grid build, both iteration budgets"""
    K, X, U0, _, start = _args(b)
    U = U0 if U is None else U
    out = []
    for max_iter in MAX_ITERS:
        ref = _solve_one_wave(K, X, U, W, start, max_iter_count=max_iter)
        team = _solve(K, X, U, W, start, max_iter_count=max_iter)
        _assert_same(team, ref)
        _assert_same(_pose_unit(dict(b, pts2d=U), W, max_iter), ref)
        out.append(team)
    return out


def test_every_lane_is_summed_exactly_once():
    """pose 2 s carries information on lane 2^s alone, pose 2 s + 1 on lane 2^s - 1 alone (s = 0 .. 5: the two sides of the 1-, 2-, 4-, 8-,
    16- and 32-lane exchange): every total is that lane's term; dropped it would be 0, taken twice its double"""
    lanes = [l for s in range(6) for l in (1 << s, (1 << s) - 1)]
    b = _batch(len(lanes), 64)
    W = torch.zeros_like(b["inv_std"])
    for pose, lane in enumerate(lanes):
        W[pose, lane] = b["inv_std"][pose, lane]
    _both_ways(b, W)


@pytest.mark.parametrize("N", (17, 64))
def test_the_pairing_shows_in_the_bits(N):
    """information factors of 1e8 on some lanes and 1 on the others: terms of ~1e16 and ~1 in J^T J and r^T r, of either sign in J^T r.  Whether
    a small term survives depends on the partial sum it meets first, so another pairing of the same lanes gives other bits.  The heavy lanes
    come every 2nd, 3rd, 5th lane and in runs of 4, 8 and 16: each exchange width meets both mixed and unmixed pairs."""
    heavy = [lambda l: l % 2 == 0, lambda l: l % 3 == 0, lambda l: l % 5 == 0, lambda l: (l // 4) % 2 == 0, lambda l: (l // 8) % 2 == 1,
             lambda l: (l // 16) % 2 == 0]
    b = _batch(len(heavy), N)
    W = b["inv_std"].clone()
    for pose, h in enumerate(heavy):
        for lane in range(N):
            if h(lane):
                W[pose, lane] *= 1e8
    _both_ways(b, W)


@pytest.mark.parametrize("N", (4, 64))
def test_non_finite_correspondences_fail_the_job_alike(N):
    """a NaN, +inf or -inf on each lane of one quad (the first; with N = 64 also the first of the upper half-wave, lanes 32 .. 35): the first
    evaluation fails in both builds alike, rets = 1 after no iteration"""
    b = _batch(3, N)
    U = b["pts2d"]
    for lane in [0, 1, 2, 3] + ([32, 33, 34, 35] if N > 32 else []):
        for bad in (float("nan"), float("inf"), float("-inf")):
            U2 = U.clone()
            U2[0, lane, 0] = bad
            U2[2, lane, 1] = bad
            for team in _both_ways(b, b["inv_std"], U2):
                assert team[2].tolist()[::2] == [1, 1] and team[3].tolist()[::2] == [0, 0]
