"""The latency build of the N <= 64 solve runs TWO wavefronts per pose (lc_pnp_body.h: TEAM): each forms, stores and sums the 14 of the 28
entries J^T J | J^T r | r^T r of its parity, one workgroup barrier per evaluation, everything else replicated.  Every total keeps the one-wave
form's summation order, so the results are the one-wave arithmetic's bit for bit.  The one-wave arithmetic is at hand in the same library: the
large-grid build (more than 1024 poses in a launch), reached here as tests/test_gpu_pnp.py::test_large_grid_build_equals_the_latency_build
reaches it -- the poses under test repeated into a batch beyond the threshold.  The pose unit's latency launch (team solve workgroups + loss
workgroups of two samples, one per wavefront) must return the bits of the two separate launches."""
import functools

import numpy as np
import pytest
import torch

from tests.pnp_cases import pnp_case

pytestmark = pytest.mark.gpu

BIG = 1025  # poses in a launch that takes the large-grid (one wavefront per pose) build: kLatencyGridMax + 1
SHAPES = [(B, N) for B in (1, 2, 3, 255, 256) for N in (3, 31, 32, 33, 63, 64)]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch(B, N):
    from lc_amd import synth

    return {k: v.to(_dev()) for k, v in synth.make_batch(B, N, seed=1000 * B + N).items()}


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
    for name, a, c in zip(("states", "result_tr", "rets", "iters"), team, one_wave):
        assert torch.equal(a, c), name


@pytest.mark.parametrize("B,N", SHAPES)
def test_team_solve_equals_the_one_wave_solve(B, N):
    """single pose, odd batches, the segment edge at lane 32, padding lanes"""
    b = _batch(B, N)
    args = (b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"])
    team = _solve(*args)
    _assert_same(team, _solve_one_wave(*args))
    assert int(team[3].max()) >= 1


@pytest.mark.parametrize("B,N", SHAPES)
def test_pose_unit_equals_the_two_launches(B, N):
    """team solve workgroups and two-sample loss workgroups in one grid (an odd B leaves the last loss workgroup one sample)"""
    from lc_amd.cov_mixed import loss_cov_mixed_fused
    from lc_amd.fused import PoseUnit

    b = _batch(B, N)
    go = (torch.rand(B, generator=torch.Generator().manual_seed(B + N)) + 0.5).to(_dev())
    unit = PoseUnit(B, N, _dev())(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], b["bbox_3d"], b["start"], grad_out=go)
    loss, du, ds, dx, _ = loss_cov_mixed_fused(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, b["bbox_3d"], grad_out=go)
    st, tr, ret, _ = _solve(b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"])
    for name, a, c in (("loss", unit.loss, loss), ("d_pts2d", unit.d_pts2d, du), ("d_inv_std", unit.d_inv_std, ds), ("d_pts3d", unit.d_pts3d, dx),
                       ("states", unit.states, st), ("trust_radius", unit.trust_radius, tr), ("invalid", unit.invalid, ret)):
        assert torch.equal(a, c), name


def test_poses_with_too_few_points_leave_before_any_barrier():
    """counts 0 and 2 (both waves return at once, outputs by wave 0) beside solving poses of 3, 17 and 64 points"""
    B, N = 10, 64
    b = _batch(B, N)
    counts = torch.tensor([0, 2, 3, 17, 64] * 2, dtype=torch.int32, device=_dev())
    args = (b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"], counts)
    team = _solve(*args)
    _assert_same(team, _solve_one_wave(*args))
    assert team[2].tolist() == [1, 1, 0, 0, 0] * 2 and team[3][:2].tolist() == [0, 0] and team[1][:2].tolist() == [1.0, 1.0]
    assert torch.equal(team[0][:2], b["start"][:2])


def test_every_branch_of_the_schedule_crosses_the_barrier():
    """pnp_cases' hard batch (far starts, outliers) with degenerate twins written over its first rows (coincident, collinear and origin
    points, information on u alone, a start behind the camera, gross outliers): rejected steps -- the extra evaluation at x --, failed
    evaluations, and, with the iteration budget cut to 12, solves that leave through max_iter (rets = 1); the diagnostic trace confirms
    that the rejected steps are there.
    HandleInvalidStep is NOT reached here, nor by anything else that was tried: the trace kernel reported no invalid step in 40 000 solves
    (this batch and the other cases of pnp_cases.py with function tolerance 1e-6 and 0, synthetic batches of 3 to 64 points with up to
    50 % outliers and starts 1 rad off, singular geometries) -- the damped pivots 1e-6 / radius keep the LDL^T positive unless a
    singular system meets a radius near its cap.  That branch has no barrier between the test and the `continue`, and both waves
    take it from the same bits."""
    from lc_amd.pnp import pnp_ceres

    c = pnp_case("hard_B512_N12")
    K, X, U, L, start = (torch.from_numpy(c[k]).clone() for k in ("K", "pts3d", "pts2d", "sqrtL", "start"))
    N = X.shape[1]
    X[0] = X[0, :1]                                                                              # all points coincide
    X[1] = X[1, :1] + torch.linspace(0, 1, N)[:, None] * torch.tensor([30.0, 10.0, -20.0])       # collinear points
    X[2] = 0.0                                                                                   # every point at the origin
    L[3, :, 1, 1] = 0.0                                                                          # information on u only
    start[4, 6] = -start[4, 6]                                                                   # start behind the camera
    U[5, ::2] += 500.0                                                                           # half of the points are gross outliers
    X[6, 3:] = X[6, :1]                                                                          # three distinct points, the rest coincide
    U[7, 3, 0] = float("nan")                                                                    # the first evaluation fails
    args = tuple(t.to(_dev()) for t in (K, X, U, L, start))
    for max_iter in (c["max_iter"], 12):
        kw = dict(max_iter_count=max_iter, function_tolerance=c["ftol"])
        team = _solve(*args, **kw)
        _assert_same(team, _solve_one_wave(*args, **kw))
        iters, rets = team[3].cpu().numpy(), team[2].cpu().numpy()
        if max_iter == 12:
            assert ((iters == 12) & (rets == 1)).any(), "no solve ran into max_iter"
        else:
            trace = pnp_ceres.solve_device(*args, trace_rows=max_iter, **kw)[-1].cpu().numpy()
            live = np.arange(trace.shape[1])[None, :] < iters[:, None]
            assert ((trace[:, :, 0] == 2) & live).any(), "no rejected step"
            assert rets[7] == 1 and iters[7] == 0 and int(iters.max()) > 12


def test_repeated_launches_and_graph_replay_on_the_same_buffers():
    """the totals' row toggle starts over in every launch: two launches back to back into the same outputs, then a captured graph of three"""
    from lc_amd.fused import PoseUnit

    B, N = 255, 33
    b = _batch(B, N)
    args = (b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], b["bbox_3d"], b["start"])
    outs = lambda u: (u.loss, u.d_pts2d, u.d_inv_std, u.d_pts3d, u.states, u.trust_radius, u.invalid, u.iters)
    want = tuple(t.clone() for t in outs(PoseUnit(B, N, _dev())(*args)))
    _assert_same((want[4], want[5], want[6], want[7]), _solve_one_wave(b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"]))
    unit = PoseUnit(B, N, _dev())
    unit(*args)
    unit(*args)
    for a, c in zip(outs(unit), want):
        assert torch.equal(a, c)
    side = torch.cuda.Stream(_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        unit(*args)
    torch.cuda.current_stream(_dev()).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            unit(*args)
    for t in outs(unit):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(outs(unit), want):
        assert torch.equal(a, c)
