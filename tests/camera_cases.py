"""Inputs and checks shared by tests/test_oracle_cameras.py (CPU) and tests/test_gpu_cameras.py (GPU): the K-reading kernels on cameras that
are not a scaled rotation (lc_amd.synth.CAMERAS).

Every batch the suite fed the loss, the keypoint NLL, the LM solve, the pose unit, the RANSAC and the test-time chains before these two
modules had K[0,0] == K[1,1], K[0,1] == -K[1,0] and K[0,2] == K[1,2] ("rot").  A kernel that reads K[4] for K[0], K[5] for K[2], or treats
the 2x2 block as orthogonal returns on such a camera what the correct kernel returns.  `mutants` builds exactly those wrong cameras; the
`check_*` functions are the assertions of the GPU twin tests (same numbers), so the CPU module can push an oracle evaluated with a mutant
camera through them and show that they fail -- and the GPU module applies them to the kernels.
"""
import functools

import numpy as np
import torch

from oracle import kpt_oracle, pnp_oracle
from tests import rowwise as rw
from tests.pnp_cases import pose_err
from tests.test_gpu_loss import CENSUS_MIN_POINTS, _rowwise, census, oracle_run, shape_inputs, wide_grad_out  # noqa: F401
from tests.util import rel_err

CAMERAS = ("bop", "stress")
MUTANTS = ("swap_focal", "swap_principal", "transpose", "as_rotation")


def mutants(K):
    """name -> K read wrongly: K[0,0] <-> K[1,1]; K[0,2] <-> K[1,2]; the 2x2 block transposed; the 2x2 block replaced by
    sqrt|det| x its nearest rotation (the polar factor) -- what a kernel that inverts it as if it were orthogonal sees."""
    K = K.double()
    out = {}
    m = K.clone(); m[:, 0, 0], m[:, 1, 1] = K[:, 1, 1], K[:, 0, 0]; out["swap_focal"] = m
    m = K.clone(); m[:, 0, 2], m[:, 1, 2] = K[:, 1, 2], K[:, 0, 2]; out["swap_principal"] = m
    m = K.clone(); m[:, :2, :2] = K[:, :2, :2].mT; out["transpose"] = m
    U, _, Vh = torch.linalg.svd(K[:, :2, :2])
    flip = torch.ones_like(K[:, :2, :2]); flip[:, :, 1] = torch.linalg.det(U @ Vh)[:, None]
    m = K.clone(); m[:, :2, :2] = torch.linalg.det(K[:, :2, :2]).abs().sqrt()[:, None, None] * ((U * flip) @ Vh); out["as_rotation"] = m
    return {k: v.float() for k, v in out.items()}  # the kernels read float32 cameras


# ---- the LC loss -------------------------------------------------------------------------------------------------------------------
# (B, N, seed, kwargs): the launch forms of lc_loss_body.h -- registers (N <= 256), the workgroup-per-sample loop (N = 257: five tiles),
# tiled (N = 1024: the workspace query is positive), and cov_2d in the loop form
LOSS_CASES = {"registers": (3, 64, 2, {}), "loop": (2, 257, 5, {}), "tiled": (2, 1024, 31, {}), "cov2d": (2, 257, 20, dict(cov_2d=True))}


@functools.lru_cache(maxsize=None)
def loss_case(form, camera):
    """-> (inputs, kwargs, fp64 oracle, fp32 oracle, fp64 and fp32 oracle under the six-decade cotangent); computed once, never modified."""
    B, N, seed, kw = LOSS_CASES[form]
    ins = shape_inputs(B, N, seed, camera=camera)
    wide = dict(ins, grad_out=wide_grad_out(B, seed))
    return (ins, kw, oracle_run(ins, torch.float64, **kw), oracle_run(ins, torch.float32, **kw),
            wide, oracle_run(wide, torch.float64, **kw), oracle_run(wide, torch.float32, **kw))


def check_loss(what, got, ref64, ref32, samples=False):
    """tests/test_gpu_loss.py::test_loss_kernel_vs_oracle_shapes: 3e-5 on the loss, 3e-4 on each gradient, then row-wise."""
    loss, gu, gs, gx = got
    rl, ru, rs, rx = ref64
    assert ((loss.double() - rl).abs() / rl.abs().clamp_min(1)).max().item() <= 3e-5, what
    assert rel_err(gu, ru) <= 3e-4 and rel_err(gs, rs) <= 3e-4 and rel_err(gx, rx) <= 3e-4, what
    _rowwise(what, got, ref64, ref32, samples=samples)


# ---- the keypoint NLL --------------------------------------------------------------------------------------------------------------
KPT_CASES = [(5, 16, 1), (3, 100, 3)]
KPT_CT = 0.37


@functools.lru_cache(maxsize=None)
def kpt_case(B, N, seed, camera):
    """The inputs of tests/test_gpu_kpt.py::test_kpt_nll_vs_oracle on `camera` -> (batch, std, pose, fp64 oracle, fp32 oracle)."""
    from lc_amd import synth

    b = synth.make_batch(B, N, seed=seed, camera=camera)
    std = torch.rand(B, N, 2, generator=torch.Generator().manual_seed(seed)) * 2 + 0.3
    pose = b["pose"].clone()
    pose[0, :4] *= 1.7        # the reference does not normalise the quaternion
    pose[1, 6] = -400.0       # behind the camera: z clamp of project_apply
    return b, std, pose, kpt_oracle_run(b["K"], pose, b, std, torch.float64), kpt_oracle_run(b["K"], pose, b, std, torch.float32)


def kpt_oracle_run(K, pose, b, std, dtype):
    """(mean NLL, d/du, d/dstd of KPT_CT x the mean) of the oracle in `dtype`."""
    nll, du, ds = kpt_oracle.nll_and_grads(K.to(dtype), pose.to(dtype), b["pts3d"].to(dtype), b["pts2d"].to(dtype), std.to(dtype))
    cnt = std.numel()
    return nll.sum().item() / cnt, du * KPT_CT / cnt, ds * KPT_CT / cnt


def check_kpt(what, got, ref64, ref32):
    """tests/test_gpu_kpt.py::test_kpt_nll_vs_oracle: 2e-6 on the loss and both gradients, then keypoint by keypoint."""
    loss, gu, gs = got
    assert abs(loss - ref64[0]) <= 2e-6 * max(1.0, abs(ref64[0])), what
    assert rel_err(gu, ref64[1]) <= 2e-6 and rel_err(gs, ref64[2]) <= 2e-6, what
    rw.check_kept(f"{what} du", gu, ref64[1], ref32[1], 2e-6, point_dims=1)
    rw.check_kept(f"{what} dstd", gs, ref64[2], ref32[2], 2e-6, point_dims=1)


# ---- the LM solve ------------------------------------------------------------------------------------------------------------------
# name -> (B, N, make_batch keywords).  The shapes reach the forms tests/launch_forms.py lists for lc_pnp_lm_*: one wave and the two-wave
# team (N <= 64), the four wide widths (N <= 256, <= 1024, <= 2048, beyond), split + rescue at the smallest admissible row (kSplitMinPoints + 1).
PNP_CASES = {
    "hard_B64_N12": (64, 12, dict(seed=31, outlier_frac=0.2, noise_px=2.0)),
    "B16_N64": (16, 64, dict(seed=64)),
    "B4_N100": (4, 100, dict(seed=100)),
    "B4_N300": (4, 300, dict(seed=300)),
    "B2_N1100": (2, 1100, dict(seed=1100)),
    "B4_N2049": (4, 2049, dict(seed=2049, noise_px=0.7)),
    "B8_N48": (8, 48, dict(seed=48, outlier_frac=0.1)),   # the chained solves (N <= 64: lc_pnp_lm_chain_small_kernel)
}


@functools.lru_cache(maxsize=None)
def pnp_batch(name, camera):
    from lc_amd import synth

    B, N, kw = PNP_CASES[name]
    return synth.make_batch(B, N, camera=camera, **kw)


def pnp_oracle_solve(b, K=None, start=None, L=None, counts=None, **kw):
    """pnp_oracle.solve_batched on a synth batch (diagonal information inv_std unless L is given) -> (states, trust radii, flags)."""
    K = b["K"] if K is None else K
    L = torch.diag_embed(b["inv_std"]).numpy() if L is None else L
    start = b["start"].numpy() if start is None else start
    return pnp_oracle.solve_batched(start, K.numpy(), b["pts2d"].numpy(), b["pts3d"].numpy(), L, counts=counts, **kw)


@functools.lru_cache(maxsize=None)
def pnp_reference(name, camera):
    return pnp_oracle_solve(pnp_batch(name, camera))


def check_pnp(what, got, ref):
    """Flags equal, every pose within 1e-4 of the oracle's (max|dq| after sign alignment, ||dt|| / ||t||), trust radii to rtol 1e-6
    (tests/test_gpu_fused.py::test_pose_unit_vs_oracle_and_reference_golden)."""
    st, tr, ret = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in got[:3])
    so, tro, reto = ref
    np.testing.assert_array_equal(ret, reto, err_msg=what)
    dq, dt = pose_err(st, so)
    print(f"{what}: dq {dq.max():.2e} dt {dt.max():.2e}, {int((reto == 0).sum())} of {len(reto)} valid")
    assert dq.max() <= 1e-4 and dt.max() <= 1e-4, (what, dq.max(), dt.max())
    np.testing.assert_allclose(tr, tro, rtol=1e-6, err_msg=what)


# ---- the RANSAC --------------------------------------------------------------------------------------------------------------------
RANSAC_SHAPE = dict(B=8, N=200, seed=208, outlier_frac=0.3)
RANSAC_ITERS, RANSAC_SEED = 150, 11
F32_MARGIN = 1e-3  # oracle/p3p_ransac_oracle.py `margin`: the points float32 may put on either side of the threshold


@functools.lru_cache(maxsize=None)
def ransac_case(camera):
    """-> (batch, ragged counts (B,) int32 incl. a pose of three points, a threshold in pixels per pose)."""
    from lc_amd import synth

    s = RANSAC_SHAPE
    b = synth.make_batch(s["B"], s["N"], seed=s["seed"], outlier_frac=s["outlier_frac"], camera=camera)
    g = torch.Generator().manual_seed(s["N"])
    counts = torch.randint(s["N"] // 2, s["N"] + 1, (s["B"],), generator=g).to(torch.int32)
    counts[0] = 3   # too few -> invalid
    counts[1] = s["N"]
    thr = torch.rand(s["B"], generator=g) * 2 + 1
    return b, counts, thr


def pixel_band(K, X, U, R, t, thr_px, half_width):
    """OpenCV's test for one pose: e = |pi(K (R X + t)) - u| < thr_px in plain float64 -> (inlier (n,) bool, in_band (n,) bool: the points
    whose e / thr_px lies within `half_width` of 1, where the kernel's isotropic test in normalised coordinates may differ)."""
    K, X, U = (np.asarray(a, np.float64) for a in (K, X, U))
    c = (X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)) @ K.T
    e = np.linalg.norm(c[:, :2] / c[:, 2:3] - U, axis=1)
    return (c[:, 2] > 0) & (e < thr_px), np.abs(e / thr_px - 1) <= half_width


def band_half_width(K):
    """sqrt(cond(K2)) - 1 + the float32 margin.  For K2 = f Rot diag(1, r): sqrt(r) - 1 (r = fy / fx)."""
    s = np.linalg.svd(np.asarray(K, np.float64)[:2, :2], compute_uv=False)
    return float(np.sqrt(s[0] / s[1]) - 1 + F32_MARGIN)
