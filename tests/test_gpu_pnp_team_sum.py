"""The team solve's block sum deals every 32-double segment of an entry's LDS row to TWO lanes, one per component of the 16-byte pairs
(lc_common.h: block_sum_team2, block_sum_segment_component): each runs the levels of block_sum_segment's tree that stay inside its
component, one quad exchange joins the components where the one-wave form adds a[0].x + a[0].y, a second one joins the two segments.  The
order in which every total is added up is the one-wave form's, so the team results are the large-grid (one wavefront per pose) build's bit
for bit.  These are the inputs on which another order would show: noisy batches with many outliers (several iterations, sums whose 64
terms span many orders of magnitude), rows cut short by `counts` so that the last point and the first padding lane fall on either
component and on either side of the segment edge at lane 32, a budget of one iteration, and non-finite correspondences on each of the four
lanes of a quad.  The one-wave arithmetic is reached as tests/test_gpu_pnp_team.py reaches it: the poses repeated beyond 1024."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 1025  # poses in a launch that takes the large-grid (one wavefront per pose) build: kLatencyGridMax + 1
BS = (1, 3)
NS = (3, 4, 31, 32, 33, 63, 64)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch(B, N):
    """noise of 6 px and 30 % outliers of 20 px: far from the start's basin, residuals from 1e-2 to 1e2 px"""
    from lc_amd import synth

    return {k: v.to(_dev()) for k, v in synth.make_batch(B, N, seed=7000 + 100 * B + N, noise_px=6.0, outlier_frac=0.3).items()}


def _args(b):
    return b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"]


def _cut(B, N):
    """rows of N - 1, N - 2, ... points (at least 3): the padding lanes start on an odd lane, an even lane, ..."""
    return torch.tensor([max(3, N - 1 - i) for i in range(B)], dtype=torch.int32, device=_dev())


def _solve(K, X, U, W, start, counts=None, **kw):
    from lc_amd.pnp import pnp_ceres

    return pnp_ceres.solve_device(K, X, U, W, start, counts, return_iters=True, **kw)  # states, result_tr, rets, iters


def _solve_one_wave(K, X, U, W, start, counts=None, **kw):
    """The same poses through the large-grid build: repeated to BIG poses, the first B rows returned."""
    B = K.shape[0]
    reps = -(-BIG // B)
    rep = lambda t: None if t is None else t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()
    big = _solve(rep(K), rep(X), rep(U), rep(W), rep(start), rep(counts), **kw)
    assert big[0].shape[0] > 1024
    return tuple(t[:B] for t in big)


def _assert_same(team, one_wave):
    """exact: the integer outputs as they are, the float outputs as their bits (-0.0 is not 0.0, a NaN equals only itself)"""
    for name, a, c in zip(("states", "result_tr", "rets", "iters"), team, one_wave):
        assert a.dtype == c.dtype and a.shape == c.shape, name
        if a.dtype == torch.float32:
            a, c = a.view(torch.int32), c.view(torch.int32)
        assert torch.equal(a, c), name


@pytest.mark.parametrize("cut", (False, True), ids=("full", "cut"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_hard_batches_keep_the_one_wave_bits(B, N, cut):
    args = _args(_batch(B, N))
    counts = _cut(B, N) if cut else None
    team = _solve(*args, counts)
    _assert_same(team, _solve_one_wave(*args, counts))
    assert int(team[3].max()) >= 1


@pytest.mark.parametrize("N", NS)
def test_one_iteration_budget(N):
    """max_iter = 1: two evaluations, the start's and the first candidate's, and the exit through the budget"""
    args = _args(_batch(3, N))
    for counts in (None, _cut(3, N)):
        team = _solve(*args, counts, max_iter_count=1)
        _assert_same(team, _solve_one_wave(*args, counts, max_iter_count=1))
        assert int(team[3].max()) == 1


@pytest.mark.parametrize("N", (4, 33, 64))
def test_non_finite_correspondences(N):
    """a NaN or an infinity on each lane of a quad in turn (component .x / .y of segment 0, and of segment 1 where the row reaches it), and in
    the last point of the row: the first evaluation fails in both builds alike, rets = 1 after no iteration"""
    B = 3
    b = _batch(B, N)
    K, X, U, W, start = (t.clone() for t in _args(b))
    for lane in sorted({0, 1, 2, 3, N - 1} | ({32, 33 % N, 34 % N, 35 % N} if N > 32 else set())):
        for bad in (float("nan"), float("inf"), float("-inf")):
            U2 = U.clone()
            U2[0, lane, 0] = bad
            U2[2, lane, 1] = bad
            team = _solve(K, X, U2, W, start)
            _assert_same(team, _solve_one_wave(K, X, U2, W, start))
            assert team[2].tolist()[::2] == [1, 1] and team[3].tolist()[::2] == [0, 0]
