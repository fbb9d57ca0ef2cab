"""Writes tests/golden/posecov_*.npz: the unmodified reference's test-time pose covariance, evaluated on the CPU in float32 and float64,

    invalid, _, cov = pnp_auto.diff_pnp_perturb(pose, K, X, u, w, with_cov=True)
    jac  = cov_mixed.jac_update2alter(pose, xform_3d(bbox_3d) | xform_2d(K, bbox_3d))
    var  = cov_mixed.transformed_cov_from_jac(cov, jac=jac)
    perr = cov_mixed.loss_cov_3d(var, diameter) | loss_cov_2d(var)

on synthetic inputs built here: points in a 0.2 box at depth ~0.8, focal length 600, 0.5 px noise on the measurements, inverse variances
in (0.2 .. 1.2)^2, evaluated at the true pose (so r != 0).  Inputs are stored as `in_*` (float32 as the kernel reads them, BEFORE the
load-time options), the options as `opt_*`, the reference's float32 results as `f32_{cov,var,perr,info}` and its float64 results as
`f64_*`.  The reference knows neither `counts` nor the load-time options: they are applied here exactly as the solver's load applies
them (tests/posecov_oracle.prepare_inputs: 1/(s*s) in fp32, then torch.nan_to_num on the fp32 values), and a ragged row b is handed to
the reference as its own batch of counts[b] points (a row of count 0: its points with all-zero weights -- the same H = 0).
`well_posed` marks the rows whose SPD verdict is no rounding accident (at least 6 points, positive finite weights): the generator asserts
info == 0 on them, in both precisions.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_posecov.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import posecov_oracle as po  # noqa: E402

CASES = po.CASES


def scene(rng, B, N, skew=False):
    """K, pose (unit quaternion), X, noisy u, inverse variances, box corners, diameter -- float32 tensors."""
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = 600 + rng.uniform(-10, 10, B)
    K[:, 1, 1] = 600 + rng.uniform(-10, 10, B)
    K[:, 0, 2] = 320 + rng.uniform(-5, 5, B)
    K[:, 1, 2] = 240 + rng.uniform(-5, 5, B)
    K[:, 2, 2] = 1
    if skew:
        K[:, 0, 1] = rng.uniform(-1, 1, B)
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.75, 0.85, B)], -1)
    X = rng.uniform(-0.1, 0.1, (B, N, 3))
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(B, 3, 3)
    Xc = X @ R.transpose(0, 2, 1) + t[:, None]
    uvw = Xc @ K.transpose(0, 2, 1)
    u = uvw[..., :2] / uvw[..., 2:] + rng.normal(scale=0.5, size=(B, N, 2))
    icov = rng.uniform(0.2, 1.2, (B, N, 2)) ** 2
    half = rng.uniform(0.08, 0.12, (B, 1, 3))
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    bbox = signs[None] * half
    diameter = 2 * np.linalg.norm(half[:, 0], axis=1)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return dict(K=f(K), pose=f(np.concatenate([q, t], 1)), pts3d=f(X), pts2d=f(u), weights=f(icov), bbox_3d=f(bbox), diameter=f(diameter))


def cases():
    """name -> (inputs, options, well_posed rows)."""
    rng = np.random.default_rng(20261017)
    out = {}
    nan, inf = float("nan"), float("inf")

    c = scene(rng, 4, 16)
    c["weights"] = c["weights"].rsqrt()  # the sparse head predicts standard deviations (test.py:52)
    out["sparse_std_B4_N16"] = (c, dict(weights_are_std=True), [1, 1, 1, 1])

    c = scene(rng, 4, 300)
    c["counts"] = torch.tensor([300, 257, 64, 5], dtype=torch.int32)
    out["ragged_B4_N300"] = (c, dict(), [1, 1, 1, 0])  # 5 points: rank-deficient, out of the SPD comparison

    c = scene(rng, 3, 50, skew=True)
    c["diameter"] = None
    out["cov2d_B3_N50"] = (c, dict(cov_2d=True), [1, 1, 1])

    c = scene(rng, 3, 24)
    c["pose"][:, :4] *= torch.tensor([[0.7], [1.0], [1.6]])
    out["nonunit_quat_B3_N24"] = (c, dict(), [1, 1, 1])

    c = scene(rng, 3, 20)
    c["weights"] = c["weights"][..., 0].contiguous()  # one inverse variance per point
    c["diameter"] = None
    out["scalar_B3_N20"] = (c, dict(), [1, 1, 1])

    # nan_to_num: NaN -> 0 anywhere; +-inf -> +-FLT_MAX.  Rows 0-1: NaN in pts2d / pts3d / weights of live points (a zeroed point or weight
    # keeps H well-posed).  Row 2: +-inf in pts2d and pts3d of points whose weight is NaN (-> 0: in float64 they contribute exact zeros; the
    # reference's float32 run overflows on them, which its stored f32 results show).  Row 3: +inf and -inf among the weights: H has
    # eigenvalues of +-1e38 magnitude, robustly not positive definite.  Row 4: untouched.
    c = scene(rng, 5, 50)
    c["pts2d"][0, 3, 0] = nan
    c["pts2d"][0, 17] = nan
    c["pts3d"][0, 20, 1] = nan
    c["weights"][0, 30, 0] = nan
    c["weights"][1, 5] = nan
    c["pts3d"][1, 44] = nan
    c["pts2d"][2, 7, 0], c["pts2d"][2, 8, 1] = inf, -inf
    c["pts3d"][2, 9, 2], c["pts3d"][2, 10, 0] = inf, -inf
    c["weights"][2, 7:11] = nan
    c["weights"][3, 11, 0], c["weights"][3, 12, 1] = inf, -inf
    out["nan_to_num_B5_N50"] = (c, dict(nan_to_num=True), [1, 1, 1, 0, 1])

    c = scene(rng, 4, 16)
    c["weights"][1] = 0.0
    c["counts"] = torch.tensor([16, 16, 0, 9], dtype=torch.int32)
    out["fallback_B4_N16"] = (c, dict(), [1, 0, 0, 1])
    assert tuple(out) == CASES
    return out


def reference_modules(ref):
    sys.path.insert(0, ref)
    from lib import cov_mixed
    from lib.nll import pnp_auto
    return pnp_auto, cov_mixed


def evaluate(mods, c, opts, dtype):
    """The reference's composition, row by row where rows are ragged -> cov, var, perr, info in `dtype`."""
    pnp_auto, cov_mixed = mods
    K, X, u, w, pose = po.prepare_inputs(c["K"], c["pts3d"], c["pts2d"], c["weights"], c["pose"], nan_to_num=opts.get("nan_to_num", False),
                                         weights_are_std=opts.get("weights_are_std", False))
    K, X, u, w, pose, bbox = (v.to(dtype) for v in (K, X, u, w, pose, c["bbox_3d"]))
    B, N = X.shape[:2]
    counts = c.get("counts")
    covs, infos = [], []
    for b in range(B):
        n = N if counts is None else int(counts[b])
        wb = w[b:b + 1, :n] if n > 0 else torch.zeros_like(w[b:b + 1])
        m = n if n > 0 else N
        invalid, _, cov = pnp_auto.diff_pnp_perturb(pose[b:b + 1], K[b:b + 1], X[b:b + 1, :m], u[b:b + 1, :m], wb, with_cov=True)
        covs.append(cov)
        infos.append(invalid)
    cov, info = torch.cat(covs), torch.cat(infos)
    if opts.get("cov_2d", False):
        jac = cov_mixed.jac_update2alter(pose, lambda st: cov_mixed.xform_2d(st, K, bbox))
    else:
        jac = cov_mixed.jac_update2alter(pose, lambda st: cov_mixed.xform_3d(st, bbox))
    var = cov_mixed.transformed_cov_from_jac(cov, jac=jac)
    if opts.get("cov_2d", False):
        perr = cov_mixed.loss_cov_2d(var)
    else:
        perr = cov_mixed.loss_cov_3d(var, None if c["diameter"] is None else c["diameter"].to(dtype))
    return cov.detach(), var.detach(), perr.detach(), info


def generate(ref):
    """name -> dict of numpy arrays (what the fixture files hold)."""
    mods = reference_modules(ref)
    out = {}
    for name, (c, opts, well) in cases().items():
        d = {f"in_{k}": v.numpy() for k, v in c.items() if v is not None}
        d.update({f"opt_{k}": np.bool_(v) for k, v in opts.items()})
        d["well_posed"] = np.array(well, dtype=np.bool_)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            cov, var, perr, info = evaluate(mods, c, opts, dtype)
            d[f"{tag}_cov"], d[f"{tag}_var"], d[f"{tag}_perr"], d[f"{tag}_info"] = cov.numpy(), var.numpy(), perr.numpy(), info.numpy().astype(np.int32)
            if tag == "f64" or name != "nan_to_num_B5_N50":  # (the float32 run overflows on the +-FLT_MAX entries of that case's row 2)
                assert not d[f"{tag}_info"][d["well_posed"]].any(), (name, tag, d[f"{tag}_info"])
        assert d["f64_info"][~d["well_posed"]].all() or name == "ragged_B4_N300", (name, d["f64_info"])
        out[name] = d
    return out


def main(ref):
    if not ref or not os.path.isdir(ref):
        raise SystemExit(__doc__)
    for name, d in generate(ref).items():
        np.savez_compressed(os.path.join(HERE, f"posecov_{name}.npz"), **d)
        print(name, "info f32", d["f32_info"], "f64", d["f64_info"], "max rel f32-f64 cov", float(po.row_error(torch.from_numpy(d["f32_cov"]), torch.from_numpy(d["f64_cov"])).max()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LC_REFERENCE", ""))
