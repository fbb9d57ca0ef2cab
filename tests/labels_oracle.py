"""A float64 restatement of the two label-preparation kernels (lc_amd/csrc/lc_labels.hip), written from the formulas of
`losses.py:68-139` / `symmetry.py:8-56` / `floatbits.py:77-97`: candidate errors and selection, xyz_gt and the network targets.
Plain torch on any device and dtype (float64 on the CPU for the oracle, float32 for the fp32 restatement)."""
import torch


def gather_check_points(gt, out, H, W):
    """The 3D branch's inputs at the check pixels: (homo_z (B,N,3), predicted points (B,N,3) or None for a code head)."""
    ck = gt["sym_ck_pts2d"].long()
    x, y = ck[..., 0] % W, ck[..., 1] % H
    bi = torch.arange(ck.shape[0], device=ck.device)[:, None].expand_as(x)
    hz = gt["homo_z_out"][bi, y, x]
    p = None
    if "xyz_noc" in out:
        p = out["xyz_noc"][bi, :, y, x] * gt["noc_scale"][:, None, :]
    return hz, p, y * W + x


def candidate_errors(mode, cam_K, a, b, cand):
    """Mean error of every candidate, (B,K): mode 0 = ||pi(K (R p + t)) - uv||, a = pts3d, b = uv; mode 1 = ||p - R^T (K^-1 h - t)||,
    a = predicted points, b = homo_z at the points."""
    R, t = cand[..., :3, :3], cand[..., :3, 3]
    if mode == 0:
        X = torch.einsum("bkij,bnj->bkni", R, a) + t[:, :, None, :]
        h = torch.einsum("bij,bknj->bkni", cam_K, X)
        uv = h[..., :2] / h[..., 2:3]
        return torch.linalg.vector_norm(uv - b[:, None], dim=-1).mean(-1)
    q = torch.einsum("bij,bnj->bni", torch.linalg.inv(cam_K), b)
    ref = torch.einsum("bkji,bknj->bkni", R, q[:, None] - t[:, :, None, :])
    return torch.linalg.vector_norm(a[:, None] - ref, dim=-1).mean(-1)


def select(mode, cam_K, a, b, candis):
    """Per chunk of the ragged list: the errors (B_c,K) and torch.argmin's choice; concatenated over the batch (lists of rows)."""
    errs, idx, r = [], [], 0
    for c in candis:
        n = c.shape[0]
        e = candidate_errors(mode, cam_K[r:r + n], a[r:r + n], b[r:r + n], c)
        errs += list(e)
        idx += list(torch.argmin(e, -1))
        r += n
    return errs, torch.stack(idx) if idx else torch.zeros(0, dtype=torch.long)


def targets(homo_z, Rt, cam_K, msk, noc_scale, T=None, bit_cnt=None, black=True):
    """xyz_gt (B,H,W,3), then (noc_tgt (B,3,H,W), None, None, None) or (None, mod_bits, raw_bits (B,C,H,W) bool, quantiser arguments (B,C,H,W))."""
    R, t = Rt[:, :3, :3], Rt[:, :3, 3]
    q = torch.einsum("bij,bhwj->bhwi", torch.linalg.inv(cam_K), homo_z)
    m = msk.to(homo_z.dtype).unsqueeze(-1)
    xyz = torch.einsum("bji,bhwj->bhwi", R, q - t[:, None, None, :]) * m
    y = xyz
    if T is not None:
        y = (torch.einsum("bij,bhwj->bhwi", T[:, :3, :3], xyz) + T[:, None, None, :3, 3]) * m
    noc = y / noc_scale[:, None, None, :]
    if bit_cnt is None:
        return xyz, noc.permute(0, 3, 1, 2), None, None, None
    mods, raws, args = [], [], []
    for a, n in enumerate(bit_cnt):
        mx = 2 ** n - 1
        arg = (noc[..., a] + 1) * (mx * 0.5)
        v = torch.clamp(arg, 0, mx).round().to(torch.int64)
        sh = torch.arange(n - 1, -1, -1, device=v.device)
        raw = (v.unsqueeze(-1) >> sh) & 1
        g = ((v ^ (v >> 1)).unsqueeze(-1) >> sh) & 1
        if black:
            g[..., :2] ^= 1
        mods.append(g.bool())
        raws.append(raw.bool())
        args.append(arg.unsqueeze(-1).expand(*arg.shape, n))
    cat = lambda xs: torch.cat(xs, -1).permute(0, 3, 1, 2)
    return xyz, None, cat(mods), cat(raws), cat(args)


def near_tie(arg, margin=1e-3):
    """Pixels (per plane) whose quantiser argument lies within `margin` of a rounding tie (x.5) without being one exactly: an exact tie (the
    masked pixels: noc = 0, argument (2^n - 1) / 2) is computed exactly in every precision and must round the same way."""
    d = (arg - arg.floor() - 0.5).abs()
    return (d < margin) & (d > 0)
