"""GPU parity of the fused keypoint-NLL launch (losses.py:318-326) against the fp64 oracle."""
import pytest
import torch

from tests import rowwise as rw
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("B,N,seed", [(1, 1, 0), (5, 16, 1), (256, 64, 2), (3, 100, 3), (2, 1000, 4)])
def test_kpt_nll_vs_oracle(B, N, seed):
    from lc_amd import synth
    from lc_amd.kpt import kpt_nll_mean
    from oracle import kpt_oracle as orc

    b = synth.make_batch(B, N, seed=seed)
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(B, N, 2, generator=g) * 2 + 0.3
    pose = b["pose"].clone()
    pose[0, :4] *= 1.7        # the reference does not normalise the quaternion (two_s = 2/|q|)
    if B > 1:
        pose[1, 6] = -400.0   # behind the camera: z clamp of project_apply
    u = b["pts2d"].to(DEV).requires_grad_(True)
    s = std.to(DEV).requires_grad_(True)
    loss = kpt_nll_mean(b["K"].to(DEV), pose.to(DEV), b["pts3d"].to(DEV), u, s)
    ct = 0.37
    gu, gs = torch.autograd.grad(loss * ct, (u, s))
    d = torch.float64
    nll, du, ds = orc.nll_and_grads(b["K"].to(d), pose.to(d), b["pts3d"].to(d), b["pts2d"].to(d), std.to(d))
    cnt = B * N * 2
    assert abs(loss.item() - nll.sum().item() / cnt) <= 2e-6 * max(1.0, abs(nll.sum().item() / cnt))
    assert rel_err(gu.cpu(), du * ct / cnt) <= 2e-6 and rel_err(gs.cpu(), ds * ct / cnt) <= 2e-6
    # keypoint by keypoint (tests/rowwise.py): the same 2e-6 against the keypoint's own largest entry (floored at 1e-3 of its sample's), or twice
    # the fp32 evaluation of the oracle where that already exceeds 2e-6 on the keypoint
    f = torch.float32
    _, du32, ds32 = orc.nll_and_grads(b["K"].to(f), pose.to(f), b["pts3d"].to(f), b["pts2d"].to(f), std.to(f))
    rw.check_kept(f"kpt {B}x{N} du", gu, du * ct / cnt, du32 * ct / cnt, 2e-6, point_dims=1)
    rw.check_kept(f"kpt {B}x{N} dstd", gs, ds * ct / cnt, ds32 * ct / cnt, 2e-6, point_dims=1)


def test_kpt_nll_forward_only_and_errors():
    from lc_amd import synth
    from lc_amd.kpt import kpt_nll_mean

    b = {k: v.to(DEV) for k, v in synth.make_batch(4, 8, seed=0).items()}
    std = torch.ones(4, 8, 2, device=DEV)
    out = kpt_nll_mean(b["K"], b["pose"], b["pts3d"], b["pts2d"], std)
    assert out.dim() == 0 and not out.requires_grad and torch.isfinite(out)
    with pytest.raises(NotImplementedError):
        kpt_nll_mean(b["K"], b["pose"], b["pts3d"].clone().requires_grad_(True), b["pts2d"], std)
    with pytest.raises(ValueError):
        kpt_nll_mean(b["K"], b["pose"], b["pts3d"], b["pts2d"], std[:, :4])
