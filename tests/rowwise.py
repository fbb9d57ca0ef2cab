"""Row-wise comparison of a kernel's output with an fp64 reference (TEST INFRASTRUCTURE ONLY).

`tests/util.py:rel_err` is one number per tensor, max|a - b| / max|b|: an error shows only if it is large next to the largest entry of the
largest sample of the batch.  For the LC loss a third to a half of all points have a gradient below 1 % of that entry (the census in
tests/test_rowwise.py), so those points are unchecked by it.  The measures here judge every point against its own size and every sample
against its own largest entry:

    point_error(got, ref, point_dims, eta)   per point: max|got - ref| over the point's entries / max(max|ref| over the point,
                                             eta x max|ref| over the point's sample).  The eta floor is a CONDITION, not a measurement: a
                                             point whose gradient is below a thousandth of its sample's largest entry is cancellation
                                             residue and is judged against that thousandth.
    sample_error(got, ref)                   per sample (dim 0): max|got - ref| / the sample's own max|ref| -- posecov's `row_error`, shared.
    bound_from_reference(own, floor)         max(2 x own, floor): `own` is the same measure of the fp32 reference against the fp64 one.  The
                                             factor 2 and the floor 4 x 2^-24 are the rule of tests/test_gpu_posecov.py: a kernel that
                                             accumulates in fp64 and rounds each output once is a few fp32 roundings from the fp64 value.
                                             A kernel's own output never enters a bound.

`ref` is always the fp64 result.  Layout: dim 0 is the sample, the last `point_dims` dims are one point's entries, whatever lies between
indexes the points of a sample -- (B, N, 2) with point_dims = 1 is the LC loss's d_pts2d.
"""
from __future__ import annotations

import torch
from torch import Tensor

from tests.posecov_oracle import FLOOR, row_error

sample_error = row_error  # (B,): max|got - ref| over the sample / the sample's largest |ref| entry; 0/0 (a sample of exact zeros met exactly) is NaN


def point_error(got: Tensor, ref: Tensor, point_dims: int = 1, eta: float = 1e-3) -> Tensor:
    """-> float64 tensor of shape ref.shape[:-point_dims].  A point of a sample whose `ref` is zero throughout has denominator zero: its
    error is 0 where `got` is exactly zero and inf where it is not."""
    g, r = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert g.shape == r.shape and 0 < point_dims < r.dim(), (g.shape, r.shape, point_dims)
    lead = r.shape[:-point_dims]
    diff = (g - r).abs().reshape(lead + (-1,)).amax(-1)
    pmax = r.abs().reshape(lead + (-1,)).amax(-1)
    smax = r.abs().reshape(r.shape[0], -1).amax(1).reshape((-1,) + (1,) * (len(lead) - 1))
    den = torch.maximum(pmax, eta * smax)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(den > 0, diff / den, torch.where(diff > 0, torch.full((), float("inf"), dtype=torch.float64), zero))


def batch_share(ref: Tensor, point_dims: int = 1) -> Tensor:
    """Per point: its largest |ref| entry as a share of the whole batch's largest -- what `rel_err` judges it against."""
    r = torch.as_tensor(ref).double()
    return r.abs().reshape(r.shape[:-point_dims] + (-1,)).amax(-1) / r.abs().max()


def bound_from_reference(own, floor: float = FLOOR):
    """max(2 x own, floor), element-wise for a tensor of per-point / per-sample measures of the fp32 reference (NaN and inf of a degenerate
    reference row count as 0: only the floor is allowed there)."""
    if isinstance(own, Tensor):
        return (2 * torch.nan_to_num(own.double(), nan=0.0, posinf=0.0)).clamp_min(floor)
    return max(2 * float(own), floor)


def kept_bound(own: Tensor, tol: float) -> Tensor:
    """The bound of a kernel whose arithmetic is fp32: the test's present tolerance number `tol`, now applied row by row; on a row where the
    fp32 evaluation of the test's own reference already exceeds it, 2 x that row's measure of the fp32 reference instead."""
    own = torch.nan_to_num(own.double(), nan=0.0, posinf=0.0)
    return torch.where(own > tol, 2 * own, torch.full_like(own, tol))


def check_kept(what: str, got: Tensor, ref64: Tensor, ref32: Tensor, tol: float, point_dims: int | None = None, rows=None):
    """`check` under `kept_bound`: rows = a shape to view the tensors as, (rows, entries...), before measuring (a map, a sample and coordinate)."""
    got, ref64, ref32 = (torch.as_tensor(t).detach().cpu() for t in (got, ref64, ref32))
    if rows is not None:
        got, ref64, ref32 = (t.reshape(rows) for t in (got, ref64, ref32))
    measure = sample_error if point_dims is None else (lambda a, b: point_error(a, b, point_dims))
    return check(what, got, ref64, ref32, point_dims=point_dims, bound=kept_bound(measure(ref32, ref64), tol))


def check(what: str, got: Tensor, ref64: Tensor, ref32: Tensor, point_dims: int | None = None, eta: float = 1e-3, floor: float = FLOOR,
          where: Tensor | None = None, bound=None):
    """Assert got against ref64 point by point (point_dims given) or sample by sample (None), every point / sample under its own bound
    max(2 x the fp32 reference's measure there, floor), or under `bound` where the caller derived one.  `where` restricts the assertion to a
    subset of points (one side of a threshold).  Prints the worst value, the fp32 reference's worst and the smallest bound; returns them."""
    measure = (lambda a, b: sample_error(a, b)) if point_dims is None else (lambda a, b: point_error(a, b, point_dims, eta))
    err = measure(torch.as_tensor(got), torch.as_tensor(ref64))
    if point_dims is None:  # a sample of exact zeros met exactly is 0/0 in `row_error`
        same = (torch.as_tensor(got).double() == torch.as_tensor(ref64).double()).reshape(err.shape[0], -1).all(1)
        err = torch.where(same, torch.zeros((), dtype=torch.float64), err)
    own = measure(torch.as_tensor(ref32), torch.as_tensor(ref64))
    lim = bound_from_reference(own, floor) if bound is None else torch.as_tensor(bound, dtype=torch.float64).expand(err.shape)
    sel = torch.ones_like(err, dtype=torch.bool) if where is None else where
    assert bool(sel.any()), what
    e, o, b = err[sel], torch.nan_to_num(own[sel], nan=0.0, posinf=0.0), lim[sel]
    print(f"{what}: kernel {e.max().item():.3e}  fp32 reference {o.max().item():.3e}  bound min {b.min().item():.3e} max {b.max().item():.3e}")
    bad = ~(e <= b)
    assert not bool(bad.any()), (what, int(bad.sum()), e[bad][:8].tolist(), b[bad][:8].tolist())
    return e.max().item(), o.max().item(), b.min().item()
