"""The latency builds of the N <= 64 solve (stand-alone, and the pose unit's team workgroups) against the large-grid build of the same library,
on inputs that take every branch of the trust-region loop around its three inlined evaluations -- the start point's, a candidate's, the current
point's again after a rejected step.  The latency translation units differ from the rest of the library in how they are compiled (machine
scheduler, and the full-range sincos() fallback of every evaluation as a call: lc_common.h, LC_SINCOS_FALLBACK_CALL); the arithmetic must not.
The large-grid build (more than 1024 poses in a launch) is reached as tests/test_gpu_pnp_team.py reaches it: the poses under test repeated into
a batch beyond the threshold, the first rows compared.  Every comparison is torch.equal on states, trust radius, return code and iteration count.
(The file keeps the name of the change it was written for: one loop body for the three evaluations, which was measured slower and not
shipped, profiles/icache2/NOTES.md.  A kept copy of H, g instead of the re-evaluation would not pass the rejected-first-step rows below:
the start point's H, g are unscaled totals times scale_i scale_j, which an evaluation with scaled columns does not reproduce bit for bit.)

The inputs with rejected steps are built like that file's hard batch (far starts, outliers; here at N = 5 and N = 64) and their rows were chosen
with the CPU oracle's iteration trace: a rejected step behind an accepted one, rejections in a row, a rejected FIRST step, accepted-only solves.
test_chosen_rows_hold_the_paths pins that on the CPU; the diagnostic TRACE kernel must report the same kinds on the device.

A non-finite correspondence fails the START point's evaluation (every evaluation reads every correspondence, and nothing in it selects a
non-finite value away), so it can never fail a candidate's alone.  With finite fp32 inputs a candidate's evaluation behind a finite start
needs an accident of cancellation that no input can be built for, and no such row is here:
  * at a candidate the Jacobian columns are multiplied by the Jacobi scaling 1 / (1 + ||J_j|| at the start), so an entry of H overflows only
    if a column grows 1e154-fold between the start and the candidate; J goes as 1 / depth^2, so the depth R X + t of a correspondence
    would have to cancel to 1e-77 of its terms in one LM step;
  * the residuals are a (k x / z - u) with a, k, x, u <= 3.4e38: r^T r overflows only for a depth z < 3e-40, where the start's own UNSCALED
    H(t_z, t_z) = sum (dr/dt_z)^2 ~ (r / z)^2 is larger than r^T r and has failed the start already -- unless, again, z cancels by 40 decades;
  * the candidate's angle stays finite: a step is at most ~|R X + t| / |X| <= 1e83 per Jacobian column (the damping floor 1e-6 / radius
    bounds the rest), far from the 1e154 at which its squared norm overflows.
The CPU oracle agrees: 82 000 solves of hard N = 5 batches with K, pts2d, pts3d, t and the information factors scaled by random powers of ten
over the fp32 range (depths squeezed down to 1e-40 of the lateral extent) and 13 000 solves with the factors bisected to just below the start's
own overflow reported no candidate cost of DBL_MAX.  What the test does run behind `cost_c` is every rejected-step row below."""
import ctypes
import functools
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.pnp_cases import _perturbed_start

BIG = 1025  # poses in a launch that takes the large-grid build: kLatencyGridMax + 1
# rows of _hard(N) and the kinds the oracle reports for them (1 accepted, 2 rejected, 4 function tolerance)
ROWS = {5: {23: "1222211114", 33: "222211114", 36: "122222111114", 57: "22222111111114", 63: "1222211114"},
        64: {4: "222211114", 84: "1222211114", 0: "1114", 1: "11114"}}


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _hard(N):
    from lc_amd import synth

    b = synth.make_batch(96, N, seed=900 + N, outlier_frac=0.2, noise_px=2.0)
    b["start"] = _perturbed_start(b, 0.3, 0.1, torch.Generator().manual_seed(900 + N))
    return b


@functools.lru_cache(maxsize=None)
def _rows(N, B):
    """the first B chosen rows of _hard(N), on the host"""
    idx = list(ROWS[N])[:B]
    return {k: v[idx].contiguous() for k, v in _hard(N).items() if torch.is_tensor(v) and v.shape[:1] == (96,)}


@functools.lru_cache(maxsize=None)
def _plain(B, N):
    from lc_amd import synth

    return synth.make_batch(B, N, seed=7000 + 10 * B + N)


def _args(b):
    return tuple(b[k].to(_dev()) for k in ("K", "pts3d", "pts2d", "inv_std", "start"))


def _solve(K, X, U, W, start, counts=None, **kw):
    from lc_amd.pnp import pnp_ceres

    return pnp_ceres.solve_device(K, X, U, W, start, counts, return_iters=True, **kw)  # states, result_tr, rets, iters


def _solve_large_grid(K, X, U, W, start, counts=None, **kw):
    B = K.shape[0]
    reps = -(-BIG // B)
    rep = lambda t: None if t is None else t.repeat((reps,) + (1,) * (t.dim() - 1)).contiguous()
    big = _solve(rep(K), rep(X), rep(U), rep(W), rep(start), rep(counts), **kw)
    assert big[0].shape[0] > 1024
    return tuple(t[:B] for t in big)


def _assert_same(got, want):
    for name, a, c in zip(("states", "result_tr", "rets", "iters"), got, want):
        assert torch.equal(a, c), name


def _oracle_kinds(b, max_iter=50):
    from oracle import pnp_oracle

    L = torch.diag_embed(b["inv_std"]).numpy()
    _, _, _, iters, trace = pnp_oracle.solve_batched_trace(b["start"].numpy(), b["K"].numpy(), b["pts2d"].numpy(), b["pts3d"].numpy(), L,
                                                           max_iter=max_iter, ftol=1e-6, trace_rows=max_iter)
    return ["".join(str(int(k)) for k in trace[i, :iters[i], 0]) for i in range(len(iters))]


@pytest.mark.parametrize("N", sorted(ROWS))
def test_chosen_rows_hold_the_paths(N):
    """CPU: the oracle's kinds of the chosen rows -- rejected behind accepted, accepted behind rejected, rejections in a row, a rejected first step"""
    kinds = _oracle_kinds(_rows(N, len(ROWS[N])))
    assert kinds == list(ROWS[N].values())
    assert any("12" in k for k in kinds) and any("21" in k for k in kinds) and any("22" in k for k in kinds)
    assert any(k.startswith("2") for k in kinds) and (N == 5 or any(set(k[:-1]) == {"1"} for k in kinds))


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(ROWS))
def test_trace_kernel_reports_the_oracles_kinds(N):
    from lc_amd.pnp import pnp_ceres

    b = _rows(N, len(ROWS[N]))
    *_, iters, trace = pnp_ceres.solve_device(*_args(b), return_iters=True, trace_rows=50)
    iters, trace = iters.cpu().numpy(), trace.cpu().numpy()
    assert ["".join(str(int(k)) for k in trace[i, :iters[i], 0]) for i in range(len(iters))] == list(ROWS[N].values())


GRID = [(B, N) for B in (1, 3, 5) for N in (2, 3, 5, 63, 64)]


def _inputs(B, N):
    """the chosen rows where there are B of them, a plain batch otherwise"""
    return _rows(N, B) if N in ROWS and B <= len(ROWS[N]) else _plain(B, N)


@pytest.mark.parametrize("B,N", [(B, N) for B, N in GRID if N >= 3])
def test_plain_batches_hold_accepted_only_solves(B, N):
    """CPU: every plain batch has a solve of accepted steps alone, ended by a tolerance (some also hold rejected steps: (5, 3), (5, 5))"""
    kinds = _oracle_kinds(_plain(B, N))
    assert any(set(k[:-1]) == {"1"} and k[-1] in "134" for k in kinds), kinds


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", GRID)
def test_plain_batches(B, N):
    """plain batches (N = 2: every pose leaves before the first evaluation)"""
    args = _args(_plain(B, N))
    got = _solve(*args)
    _assert_same(got, _solve_large_grid(*args))
    assert (int(got[3].max()) >= 1) == (N >= 3)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(1, 5), (3, 5), (5, 5), (1, 64), (3, 64)])
@pytest.mark.parametrize("max_iter", [50, 1, 2])
def test_rejected_steps(B, N, max_iter):
    """the chosen rows (B = 1: the rejected first step alone at N = 64, rejected behind accepted at N = 5); max_iter 1 and 2 leave from the step loop
    behind one and two steps with rets = 1"""
    args = _args(_rows(N, B))
    got = _solve(*args, max_iter_count=max_iter)
    _assert_same(got, _solve_large_grid(*args, max_iter_count=max_iter))
    if max_iter < 50:
        assert got[2].tolist() == [1] * B and got[3].tolist() == [max_iter] * B
    else:
        assert got[2].tolist() == [0] * B and got[3].tolist() == [len(k) for k in list(ROWS[N].values())[:B]]


@pytest.mark.gpu
def test_counts_and_a_non_finite_correspondence():
    """counts 2, 3, 5, 63, 64 in one batch (rows of _hard(64), cut to their counts: whatever steps that leaves); then a NaN in a correspondence
    inside and one beyond the count"""
    b = _rows(64, 3)
    b = {k: torch.cat((v, v[:2])) for k, v in b.items()}
    counts = torch.tensor([2, 3, 5, 63, 64], dtype=torch.int32, device=_dev())
    args = _args(b)
    got = _solve(*args, counts)
    _assert_same(got, _solve_large_grid(*args, counts))
    assert got[2][0].item() == 1 and got[3][0].item() == 0
    U = args[2].clone()
    U[1, 1, 0] = float("nan")   # inside the count of 3: the start point's evaluation fails
    U[2, 7, 1] = float("nan")   # beyond the count of 5: never read
    args = args[:2] + (U,) + args[3:]
    bad = _solve(*args, counts)
    _assert_same(bad, _solve_large_grid(*args, counts))
    assert bad[2][1].item() == 1 and bad[3][1].item() == 0 and torch.equal(bad[0][2], got[0][2])


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,max_iter", [(B, N, 50) for B, N in GRID] + [(B, N, m) for B, N in ((5, 5), (3, 64)) for m in (1, 2)])
def test_pose_unit_equals_the_two_launches(B, N, max_iter):
    """team solve workgroups beside the loss workgroups: the bits of the stand-alone launches and of the large-grid build, on the rows with rejected
    steps where there are B of them ((1 | 3 | 5, 5), (1 | 3, 64); these also with max_iter 1 and 2) and on plain batches otherwise"""
    from lc_amd.cov_mixed import loss_cov_mixed_fused
    from lc_amd.fused import PoseUnit

    b = {k: v.to(_dev()) for k, v in _inputs(B, N).items() if torch.is_tensor(v)}
    go = (torch.rand(B, generator=torch.Generator().manual_seed(B + N)) + 0.5).to(_dev())
    unit = PoseUnit(B, N, _dev())(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], b["bbox_3d"], b["start"], grad_out=go, max_iter_count=max_iter)
    loss, du, ds, dx, _ = loss_cov_mixed_fused(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, b["bbox_3d"], grad_out=go)
    solve = (b["K"], b["pts3d"], b["pts2d"], b["inv_std"], b["start"])
    st, tr, ret, it = _solve(*solve, max_iter_count=max_iter)
    for name, a, c in (("loss", unit.loss, loss), ("d_pts2d", unit.d_pts2d, du), ("d_inv_std", unit.d_inv_std, ds), ("d_pts3d", unit.d_pts3d, dx),
                       ("states", unit.states, st), ("trust_radius", unit.trust_radius, tr), ("invalid", unit.invalid, ret), ("iters", unit.iters, it)):
        assert torch.equal(a, c), name
    _assert_same((unit.states, unit.trust_radius, unit.invalid, unit.iters), _solve_large_grid(*solve, max_iter_count=max_iter))
    if max_iter < 50:
        assert it.tolist() == [max_iter] * B and ret.tolist() == [1] * B


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _sincos_probe(call):
    """tests/native/sincos_probe.hip built with LC_SINCOS_FALLBACK_CALL = call (the library name carries the hash of its sources)"""
    srcs = [os.path.join(ROOT, "tests", "native", "sincos_probe.hip"), os.path.join(ROOT, "lc_amd", "csrc", "lc_common.h"),
            os.path.join(ROOT, "lc_amd", "csrc", "shared", "lc_shared.h")]
    digest = hashlib.sha256(b"".join(open(f, "rb").read() for f in srcs)).hexdigest()[:12]
    so = os.path.join(ROOT, "build", "tests", f"libsincos_probe_{call}_{digest}.so")
    if not os.path.exists(so):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        assert os.path.exists(hipcc), "hipcc is needed to build tests/native/sincos_probe.hip"
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + f".tmp{os.getpid()}"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "lc_amd", "csrc"),
                        f"-DLC_SINCOS_FALLBACK_CALL={call}", srcs[0], "-o", tmp], check=True, capture_output=True, timeout=300)
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.sincos_probe.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    lib.sincos_probe.restype = ctypes.c_int
    return lib


@pytest.mark.gpu
def test_full_range_fallback_as_a_call_and_inline():
    """sincos_small on both sides of its 1e4 threshold, with the fallback as the out-of-line function of the latency translation units and
    inline: the same bits, and sin / cos of the angle (the reduced branch is < 1 ulp; libm's sincos is the fallback itself).  One block
    mixes lanes of both branches, one takes the fallback with all lanes."""
    x = np.concatenate((np.linspace(0.0, 8.0, 23), [9999.5, np.nextafter(1e4, 0)], [1e4, 10000.5, 12345.678, 1e5 + 0.3, 7e5, 1e6 - 0.25, 1e6],
                        np.full(32, 3.0), 1e4 + 977.0 * np.arange(64)))
    xd = torch.from_numpy(x).to(_dev())
    out = {}
    for call in (1, 0):
        s, c = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
        assert _sincos_probe(call).sincos_probe(xd.data_ptr(), s.data_ptr(), c.data_ptr(), xd.numel(), torch.cuda.current_stream(_dev()).cuda_stream) == 0
        torch.cuda.synchronize()
        out[call] = (s.cpu().numpy(), c.cpu().numpy())
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    # the device library documents 2 ulp for the fp64 sincos and numpy's sin / cos are within 1 ulp; an ulp of a value below 1 is at most
    # 1.1e-16: 3.3e-16 in all, rounded up to 2 ulp of 1.0
    assert np.abs(out[1][0] - np.sin(x)).max() <= 4.5e-16 and np.abs(out[1][1] - np.cos(x)).max() <= 4.5e-16
