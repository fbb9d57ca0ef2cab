"""GPU parity of the on-device label preparation (lc_amd.labels, lc_labels.hip) against the reference's own annots_on_the_fly
(tests/golden/labels_*.npz, written by gen_golden_labels.py) and the float64 restatement of tests/labels_oracle.py."""
import numpy as np
import pytest
import torch

from tests import labels_oracle as O
from tests.util import golden_files, case_name

pytestmark = pytest.mark.gpu
FILES = golden_files("labels_")
DEV = torch.device("cuda:0")
MARGIN = 1e-5  # relative gap between the best and the second-best fp64 mean error below which either is an acceptable choice


def _load(path):
    z = np.load(path)
    cand = [torch.from_numpy(z[k]) for k in sorted((k for k in z.files if k.startswith("in_Rt_candi_")), key=lambda k: int(k.rsplit("_", 1)[1]))]
    gt = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_") and not k.startswith("in_Rt_candi_")}
    gt["Rt_candi"] = cand
    if "bit_cnt" in z.files:
        gt["bit_cnt"] = [int(b) for b in z["bit_cnt"]]
    out = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out_")}
    cfg = {} if int(z["sym_aware_start"]) < 0 else {"sym_aware_start": int(z["sym_aware_start"])}
    return z, gt, out, cfg, int(z["step"])


def _dev(d):
    return {k: ([c.to(DEV) for c in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else (v.to(DEV) if torch.is_tensor(v) else v))
            for k, v in d.items()}


def _acceptable(errs, chosen):
    """Every row: the chosen candidate is the fp64 argmin, or within MARGIN (relative) of the fp64 minimum."""
    for e, k in zip(errs, chosen):
        e = e.double()
        best = torch.argmin(e)
        if int(k) == int(best):
            continue
        assert not torch.isnan(e).any(), "NaN error: the first NaN must win"
        assert (e[int(k)] - e[best]) <= MARGIN * e[best].abs() + 1e-300, (int(k), int(best), e[int(k)].item(), e[best].item())


def _clear(errs):
    """Rows whose fp64 best and second-best mean errors differ by more than MARGIN (relative)."""
    out = []
    for e in errs:
        e = e.double()
        if e.numel() < 2:
            out.append(True)
            continue
        s = torch.sort(e).values
        out.append(bool((s[1] - s[0]) > MARGIN * s[0].abs()))
    return out


def _check_bits(got, want, arg):
    bad = got.cpu() != want
    excused = O.near_tie(arg)
    assert not (bad & ~excused).any(), int((bad & ~excused).sum())
    assert bad.float().mean().item() < 1e-3


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "labels_") for p in FILES])
def test_annots_on_the_fly_vs_reference(path):
    from lc_amd import labels

    z, gt, out, cfg, step = _load(path)
    g = _dev(gt)
    o = _dev(out)
    labels.annots_on_the_fly(g, o, cfg, step)
    cand = gt["Rt_candi"]
    started = step >= cfg.get("sym_aware_start", 0)
    f64 = lambda k: torch.from_numpy(z["f64_" + k]).double()
    f32 = lambda k: torch.from_numpy(z["f32_" + k])
    B = g["Rt_best"].shape[0]
    # the selection: equal to the reference wherever the choice is clear, an fp64 minimiser within the margin elsewhere
    if started and not (len(cand) == 1 and cand[0].shape[1] == 1):
        if "pts2d" in out:
            a, b, mode = gt["pts3d"].double(), out["pts2d"].double(), 0
            K = gt["out_K"].double()
        else:
            H, W = gt["homo_z_out"].shape[1:3]
            hz, p, _ = O.gather_check_points({k: v.double() if v.is_floating_point() else v for k, v in gt.items() if torch.is_tensor(v)},
                                             {k: v.double() for k, v in out.items()}, H, W)
            if p is None:  # code head: the points the decode kernel reads at the check pixels (tested in test_gpu_bits)
                from lc_amd import floatbits

                ck = g["sym_ck_pts2d"]
                index = ((ck[..., 1] % H) * W + ck[..., 0] % W).int().contiguous()
                pts = torch.empty(B, ck.shape[1], 3, device=DEV)
                floatbits.decode_selected_rows(o["xyz_noc_bin"], gt["bit_cnt"], index, torch.full((B,), ck.shape[1], device=DEV, dtype=torch.int32),
                                               pts, noc_scale=g["noc_scale"], model_transform=g.get("model_transform"))
                p = pts.cpu().double()
            a, b, mode = p, hz, 1
            K = gt["K_no_aug"].double()
        errs, _ = O.select(mode, K, a, b, [c.double() for c in cand])
        chosen = []
        for c, r in zip(cand, np.cumsum([0] + [c.shape[0] for c in cand])):
            for i in range(c.shape[0]):
                hit = (c[i] == g["Rt_best"][r + i].cpu()).all(-1).all(-1).nonzero()
                chosen.append(int(hit[0]))
        _acceptable(errs, chosen)
        clear = torch.tensor(_clear(errs))
        assert torch.equal(g["Rt_best"].cpu()[clear], f32("Rt_best")[clear])
        assert torch.allclose(g["pose_best"].cpu()[clear], f32("pose_best")[clear], rtol=0, atol=1e-6)
    else:
        assert torch.equal(g["Rt_best"].cpu(), f32("Rt_best"))
        assert torch.allclose(g["pose_best"].cpu(), f32("pose_best"), rtol=0, atol=1e-6)
    # xyz_gt and the targets against the fp64 run (with the pose the kernel chose: the same wherever the choice is clear)
    Rt = g["Rt_best"].cpu().double()
    if len(cand) == 1 and cand[0].shape[1] == 1:
        Rt = torch.cat((gt["R_no_aug"], gt["t_no_aug"][..., None]), -1).double()
    T = gt.get("model_transform")
    xyz, noc, tgt, raw, arg = O.targets(gt["homo_z_out"].double(), Rt, gt["K_no_aug"].double(), gt["msk_noc"], gt["noc_scale"].double(),
                                        None if T is None else T.double(), gt.get("bit_cnt"))
    assert ((g["xyz_gt"].cpu().double() - xyz).abs().max() <= 1e-5 * xyz.abs().max())
    rows = torch.tensor(_clear(errs)) if started and not (len(cand) == 1 and cand[0].shape[1] == 1) else torch.ones(B, dtype=torch.bool)
    assert ((g["xyz_gt"].cpu().double()[rows] - f64("xyz_gt")[rows]).abs().max() <= 1e-5 * f64("xyz_gt").abs().max())
    if noc is not None:
        assert g["xyz_noc_tgt"].shape == f64("xyz_noc_tgt").shape and g["xyz_noc_tgt"].dtype == torch.float32
        assert ((g["xyz_noc_tgt"].cpu().double() - noc).abs().max() <= 1e-5 * noc.abs().max())
        assert "xyz_noc_bin_tgt" not in g
    else:
        assert g["xyz_noc_bin_tgt"].dtype == torch.bool and g["xyz_noc_bin_tgt"].shape == tgt.shape
        _check_bits(g["xyz_noc_bin_tgt"], tgt, arg)
        _check_bits(g["xyz_noc_bin_raw"], raw, arg)
        _check_bits(g["xyz_noc_bin_tgt"][rows], torch.from_numpy(z["f64_xyz_noc_bin_tgt"])[rows], arg[rows])
    # selete_best_pose alone: the same pose and xyz_gt
    g2 = _dev(gt)
    Rt_best, pose_best, xyz_gt = labels.selete_best_pose(g2, o, started)
    assert torch.equal(Rt_best, g["Rt_best"]) and torch.equal(xyz_gt, g["xyz_gt"]) and torch.equal(pose_best, g["pose_best"])


def _random_case(gen, B, K, N, mode, H=16, W=16):
    R = torch.linalg.qr(torch.randn(B, K, 3, 3, generator=gen, dtype=torch.float64))[0]
    t = torch.randn(B, K, 3, generator=gen, dtype=torch.float64) * 10 + torch.tensor([0, 0, 500.0], dtype=torch.float64)
    cand = torch.cat((R, t[..., None]), -1).float()
    Kc = torch.tensor([[100.0, 0.5, 8], [0, 95, 8], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    a = torch.randn(B, N, 3, generator=gen) * 30
    b = torch.randn(B, N, 2 if mode == 0 else 3, generator=gen) * (5 if mode == 0 else 200) + (8 if mode == 0 else 0)
    if mode == 1:
        b[..., 2] = b[..., 2].abs() + 400
    return cand, Kc, a, b


@pytest.mark.parametrize("mode", [0, 1])
def test_selection_sweep_vs_fp64_oracle(mode):
    from lc_amd.labels import _select

    gen = torch.Generator().manual_seed(7 + mode)
    for B in (1, 5, 32):
        for K in (1, 2, 384):
            for N in (1, 63, 64, 256, 1024):
                if B * K * N > 32 * 384 * 256:
                    continue
                cand, Kc, a, b = _random_case(gen, B, K, N, mode)
                if K == 384 and B > 1:
                    cand[1, 200] = cand[1, 3]  # an exact tie with an earlier candidate: the first index
                    cand[1, 5] = cand[1, 3]
                if K >= 2 and mode == 0 and B > 2:
                    cand[2, 1] = 0.0  # a candidate that projects every point to 0 / 0: a NaN error, which wins
                Rt, idx = _select(mode, [cand.to(DEV)], Kc.to(DEV), N, pts_a=a.to(DEV), pts_b=b.to(DEV))
                errs, want = O.select(mode, Kc.double(), a.double(), b.double(), [cand.double()])
                idx = idx.cpu().long()
                _acceptable(errs, idx)
                clear = torch.tensor(_clear(errs))
                assert torch.equal(idx[clear], want[clear]), (B, K, N)
                assert torch.equal(Rt.cpu(), cand[torch.arange(B), idx])
                if K == 384 and B > 1:
                    assert int(idx[1]) not in (5, 200)  # a duplicate never wins over its first occurrence
                if K >= 2 and mode == 0 and B > 2 and torch.isnan(errs[2]).any():
                    assert int(idx[2]) == int(torch.isnan(errs[2]).nonzero()[0])


def test_continuous_head_dtypes_match_fp32_on_upcast_values():
    from lc_amd import labels

    z, gt, out, cfg, step = _load(golden_files("labels_continuous3d")[0])
    res = {}
    for dt in (torch.float16, torch.bfloat16):
        lo = out["xyz_noc"].to(dt)
        g1, g2 = _dev(gt), _dev(gt)
        labels.annots_on_the_fly(g1, {"xyz_noc": lo.to(DEV)}, cfg, step)
        labels.annots_on_the_fly(g2, {"xyz_noc": lo.float().to(DEV)}, cfg, step)
        for k in ("Rt_best", "pose_best", "xyz_gt", "xyz_noc_tgt"):
            assert torch.equal(g1[k], g2[k]), (dt, k)
        res[dt] = g1["Rt_best"]
    # a channel slice of a wider head output is read where it lies
    wide = torch.cat((out["xyz_noc"], torch.zeros_like(out["xyz_noc"][:, :2])), 1).to(DEV)
    g1, g2 = _dev(gt), _dev(gt)
    labels.annots_on_the_fly(g1, {"xyz_noc": wide[:, :3]}, cfg, step)
    labels.annots_on_the_fly(g2, {"xyz_noc": out["xyz_noc"].to(DEV)}, cfg, step)
    assert torch.equal(g1["Rt_best"], g2["Rt_best"])


def test_graph_capture_replays_like_eager():
    from lc_amd import labels

    z, gt, out, cfg, step = _load(golden_files("labels_discrete3d")[0])
    g, o = _dev(gt), _dev(out)
    labels.annots_on_the_fly(g, o, cfg, step)  # warm-up (library load, allocator)
    torch.cuda.synchronize()
    gg = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        labels.annots_on_the_fly(g, o, cfg, step)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(gg):
        labels.annots_on_the_fly(g, o, cfg, step)
    # new inputs into the captured buffers
    gen = torch.Generator().manual_seed(3)
    new_logits = torch.randn(o["xyz_noc_bin"].shape, generator=gen)
    new_hz = gt["homo_z_out"] * (1 + 0.01 * torch.rand(gt["homo_z_out"].shape, generator=gen))
    o["xyz_noc_bin"].copy_(new_logits.to(DEV))
    g["homo_z_out"].copy_(new_hz.to(DEV))
    gg.replay()
    torch.cuda.synchronize()
    e, eo = _dev(gt), {"xyz_noc_bin": new_logits.to(DEV)}
    e["homo_z_out"] = new_hz.to(DEV)
    labels.annots_on_the_fly(e, eo, cfg, step)
    for k in ("Rt_best", "pose_best", "xyz_gt", "xyz_noc_bin_tgt", "xyz_noc_bin_raw"):
        assert torch.equal(g[k], e[k]), k


def _zlmo_batch(sym, gen, B=32, H=128, W=128, bits=(7, 7, 7)):
    """A zlmo-shaped step's ground truth (B = 32, 128 x 128, 21 code planes) with or without a K = 4 symmetric chunk."""
    K = torch.tensor([[300.0, 0, 64], [0, 300, 64], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0]
    R = (R * torch.sign(torch.det(R))[:, None, None]).float()
    t = torch.cat((torch.randn(B, 2, generator=gen) * 5, 600 + torch.rand(B, 1, generator=gen) * 50), -1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = t[:, 2, None, None] + torch.rand(B, H, W, generator=gen) * 60 - 30
    hz = torch.stack((u * z, v * z, z), -1)
    msk = ((u - 64) ** 2 + (v - 64) ** 2 < 45 ** 2).expand(B, H, W).contiguous()
    Rt = torch.cat((R, t[:, :, None]), -1)
    if sym:
        flip = torch.diag(torch.tensor([-1.0, -1, 1]))
        c4 = torch.stack([Rt[8:], torch.cat((R[8:] @ flip, t[8:, :, None]), -1), Rt[8:] * 1, torch.cat((R[8:] @ flip, t[8:, :, None]), -1)], 1)
        cand = [Rt[:8, None], c4]
    else:
        cand = [Rt[:, None]]
    T = torch.eye(4).expand(B, 4, 4).contiguous()
    ck = torch.stack((torch.randint(20, 108, (B, 256), generator=gen), torch.randint(20, 108, (B, 256), generator=gen)), -1)
    gt = dict(Rt_candi=cand, homo_z_out=hz, R_no_aug=R, t_no_aug=t, K_no_aug=K, msk_noc=msk, noc_scale=torch.full((B, 3), 120.0),
              model_transform=T, bit_cnt=list(bits), sym_ck_pts2d=ck, out_K=K)
    return gt


def _torch_restatement(gt, Rt):
    """The fp32 torch statement of the targets (labels_oracle in float32 on the device)."""
    xyz, _, tgt, raw, arg = O.targets(gt["homo_z_out"], Rt, gt["K_no_aug"], gt["msk_noc"], gt["noc_scale"], gt["model_transform"], gt["bit_cnt"])
    return xyz, tgt, raw, arg


@pytest.mark.parametrize("sym", [False, True], ids=["nosym", "sym"])
def test_zlmo_shape_feeds_loss_fn(sym):
    """B = 32, 128 x 128, 21 code planes: the native labels against the fp32 torch statement, then the same Loss_fn fed either set."""
    from lc_amd import labels, synth
    from lc_amd.config import AttrDict
    from lc_amd.losses import Loss_fn
    from tests.golden.gen_golden_lossfn import BIN_CFG

    gen = torch.Generator().manual_seed(11)
    base, out = synth.train_inputs("bin_zlmo", B=32)
    lab = _zlmo_batch(sym, gen)
    for k in ("noc_scale", "model_transform", "bit_cnt", "out_K"):
        lab.pop(k)
    gt = _dev({**{k: v for k, v in base.items() if k not in ("xyz_noc_bin_tgt", "xyz_noc_bin_raw", "pose_best")}, **lab})
    out = _dev(out)
    g = dict(gt)
    labels.annots_on_the_fly(g, {k: v.detach() for k, v in out.items()}, {"sym_aware_start": 0}, 1)
    Rt_xyz = torch.cat((gt["R_no_aug"], gt["t_no_aug"][..., None]), -1) if not sym else g["Rt_best"]
    xyz, tgt, raw, arg = _torch_restatement(gt, Rt_xyz)
    assert ((g["xyz_gt"] - xyz).abs().max() <= 1e-5 * xyz.abs().max()).item()
    excused = O.near_tie(arg.double()).to(DEV)
    for got, want in ((g["xyz_noc_bin_tgt"], tgt), (g["xyz_noc_bin_raw"], raw)):
        bad = got != want
        assert not (bad & ~excused).any() and bad.float().mean().item() < 1e-3
    if sym:  # rows 8.. chose among four candidates; the errors of the selection are checked against the oracle elsewhere
        assert torch.equal(g["Rt_best"][:8], gt["Rt_candi"][0][:, 0])
    else:
        assert torch.equal(g["Rt_best"], gt["Rt_candi"][0][:, 0])
    # the torch-fed step: the same pose, xyz_gt of the torch statement, its bits (the native ones only at the excused near-tie pixels)
    from lc_amd.transforms import RT_to_quaternion_rep

    t = dict(gt, Rt_best=g["Rt_best"].clone(), pose_best=RT_to_quaternion_rep(g["Rt_best"][..., :3, :3], g["Rt_best"][..., :, 3]), xyz_gt=xyz,
             xyz_noc_bin_tgt=torch.where(excused, g["xyz_noc_bin_tgt"], tgt), xyz_noc_bin_raw=torch.where(excused, g["xyz_noc_bin_raw"], raw))
    res = []
    for labels_dict in (g, t):
        fn = Loss_fn(AttrDict(BIN_CFG), AttrDict(), 21).to(DEV)
        o = {k: v.detach().clone().requires_grad_(True) for k, v in out.items()}
        np.random.seed(5)
        ld, wd = fn(labels_dict, o, 1, 1000, 10)
        total = sum(wd.values())
        grads = torch.autograd.grad(total, list(o.values()), allow_unused=True)
        res.append(({k: float(v.detach()) for k, v in ld.items()}, grads))
    (la, ga), (lb, gb) = res
    assert la.keys() == lb.keys()
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-6 * max(abs(lb[k]), 1e-12), (k, la[k], lb[k])
    for x, y in zip(ga, gb):
        assert (x is None) == (y is None)
        if x is not None:
            assert ((x - y).abs().max() <= 1e-6 * y.abs().max()).item()


def _posed_case(gen, B, K, N, mode):
    """_random_case whose observations come from candidate pose P0 (row b's pose), so copies of P0 are exact ties at error ~0."""
    cand, Kc, a, b = _random_case(gen, B, K, N, mode)
    P0 = cand[:, 0].double()
    R0, t0 = P0[..., :3], P0[..., 3]
    if mode == 0:
        h = torch.einsum("bij,bnj->bni", Kc.double(), torch.einsum("bij,bnj->bni", R0, a.double()) + t0[:, None])
        b = (h[..., :2] / h[..., 2:3]).float()
    else:
        q = torch.einsum("bij,bnj->bni", torch.linalg.inv(Kc.double()), b.double())
        a = torch.einsum("bji,bnj->bni", R0, q - t0[:, None]).float()
    return cand, Kc, a, b, P0.float()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [65, 128, 257, 512])
def test_selection_points_per_lane_2_and_8_vs_fp64_oracle(mode, N):
    """N = 65 / 128 select lc_sym_select_kernel<2, 512> and N = 257 / 512 select <8, 512> (launch_sym_select: PPL = the smallest of
    1, 2, 4, 8 with N <= 64 PPL, 512 threads), with the padded lanes of the last wave at N = 65 and 257.  Against the fp64 oracle,
    with an exact tie (first index wins) and a NaN candidate (its first occurrence wins)."""
    from lc_amd.labels import _select

    gen = torch.Generator().manual_seed(30 + N + mode)
    B, K = 4, 96
    cand, Kc, a, b, P0 = _posed_case(gen, B, K, N, mode)
    cand[1, 40] = P0[1]
    cand[1, 70] = P0[1]  # row 1: the pose at 40 and 70 (and 0): index 0
    cand[2, 0] = cand[2, 1]
    cand[2, 50, 0, 0] = float("nan")
    cand[2, 80, 1, 1] = float("nan")  # row 2: the first NaN wins
    Rt, idx = _select(mode, [cand.to(DEV)], Kc.to(DEV), N, pts_a=a.to(DEV), pts_b=b.to(DEV))
    errs, want = O.select(mode, Kc.double(), a.double(), b.double(), [cand.double()])
    idx = idx.cpu().long()
    _acceptable(errs, idx)
    clear = torch.tensor(_clear(errs))
    assert torch.equal(idx[clear], want[clear])
    assert torch.equal(Rt.cpu().view(torch.int32), cand[torch.arange(B), idx].view(torch.int32))  # bitwise: NaN entries included
    assert int(idx[1]) == 0 and int(idx[2]) == 50


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [1024, 1025, 1500])
def test_selection_beyond_the_lds_candidate_limit_vs_fp64_oracle(mode, K):
    """K > 1024 candidates per row are walked from global memory (lc_labels.hip: staged = K > 1 && K <= kSelLdsCands); K = 1024 is the
    last staged row.  Exact ties and NaN candidates on both sides of candidate 1024: row 0 holds the pose at 1010 and 1020 (1010 wins),
    row 1 at 1010 and K-1 (1010 wins), row 2 only beyond the limit (K-1 wins when K > 1024), row 3 a NaN at 1000 and K-1 (1000 wins),
    row 4 a NaN only at K-1 (it wins)."""
    from lc_amd.labels import _select

    gen = torch.Generator().manual_seed(K + mode)
    B, N = 5, 64
    cand, Kc, a, b, P0 = _posed_case(gen, B, K, N, mode)
    cand[:, 0] = cand[:, 1]  # P0 itself is not a candidate of any row unless placed
    cand[0, 1010], cand[0, 1020] = P0[0], P0[0]
    cand[1, 1010], cand[1, K - 1] = P0[1], P0[1]
    cand[2, K - 1] = P0[2]
    cand[3, 1000, 0, 0] = float("nan")
    cand[3, K - 1, 2, 2] = float("nan")
    cand[4, K - 1, 0, 1] = float("nan")
    Rt, idx = _select(mode, [cand.to(DEV)], Kc.to(DEV), N, pts_a=a.to(DEV), pts_b=b.to(DEV))
    errs, want = O.select(mode, Kc.double(), a.double(), b.double(), [cand.double()])
    idx = idx.cpu().long()
    _acceptable(errs, idx)
    clear = torch.tensor(_clear(errs))
    assert torch.equal(idx[clear], want[clear])
    assert torch.equal(Rt.cpu().view(torch.int32), cand[torch.arange(B), idx].view(torch.int32))
    assert idx[:5].tolist() == [1010, 1010, K - 1, 1000, K - 1]


def _label_inputs(gen, B, H, W):
    K = torch.tensor([[90.0, 0.3, W / 2], [0, 85, H / 2], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0]
    R = (R * torch.sign(torch.det(R))[:, None, None]).float()
    t = torch.cat((torch.randn(B, 2, generator=gen) * 5, 600 + torch.rand(B, 1, generator=gen) * 50), -1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = t[:, 2, None, None] + torch.rand(B, H, W, generator=gen) * 60 - 30
    hz = torch.stack((u * z, v * z, z), -1)
    msk = torch.rand(B, H, W, generator=gen) > 0.25
    T = torch.eye(4).expand(B, 4, 4).contiguous().clone()
    T[:, :3, 3] = torch.randn(B, 3, generator=gen) * 3
    sc = torch.full((B, 3), 40.0) + torch.rand(B, 3, generator=gen) * 10
    return hz, torch.cat((R, t[..., None]), -1), K, msk, sc, T


def _at_offset(t, off):
    """t's values in a fresh device buffer at storage offset `off` elements (a contiguous view: _f32 / .contiguous() keep it in place)."""
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t.to(DEV))
    return v


@pytest.mark.parametrize("bits", [None, (7, 6, 5)], ids=["noc", "code"])
@pytest.mark.parametrize("H,W", [(12, 13), (11, 13)], ids=["hw4mod8", "hwodd"])
def test_label_targets_pix4_and_pix1_vs_fp64_oracle(H, W, bits):
    """H W = 156 (= 4 mod 8) selects lc_label_targets_kernel<4>, H W = 143 (odd) <1> (launch_label_targets: PIX = 8 / 4 / 1, the widest
    that divides H W with every buffer aligned for it).  xyz_gt, the continuous target or the Gray-coded / raw planes with the black
    background inversion, against the fp64 oracle (quantiser near-ties excused as in test_annots_on_the_fly_vs_reference)."""
    from lc_amd import floatbits, labels

    assert floatbits._black_background
    gen = torch.Generator().manual_seed(H * W + (0 if bits is None else 1))
    hz, Rt, K, msk, sc, T = _label_inputs(gen, 3, H, W)
    xyz, noc, tgt, raw = labels._targets(hz.to(DEV), Rt.to(DEV), K.to(DEV), msk=msk.to(DEV), noc_scale=sc.to(DEV), xform=T.to(DEV),
                                         bit_cnt=None if bits is None else list(bits), want_targets=True)
    rxyz, rnoc, rtgt, rraw, arg = O.targets(hz.double(), Rt.double(), K.double(), msk, sc.double(), T.double(), None if bits is None else list(bits))
    assert ((xyz.cpu().double() - rxyz).abs().max() <= 1e-5 * rxyz.abs().max())
    if bits is None:
        assert ((noc.cpu().double() - rnoc).abs().max() <= 1e-5 * rnoc.abs().max())
    else:
        _check_bits(tgt, rtgt, arg)
        _check_bits(raw, rraw, arg)


@pytest.mark.parametrize("bits", [None, (7, 6, 5)], ids=["noc", "code"])
@pytest.mark.parametrize("mask", ["u8", "f32"])
def test_label_targets_forms_are_identical_on_the_same_pixels(bits, mask):
    """H W = 160 (a multiple of 8): aligned buffers take lc_label_targets_kernel<8>; a byte mask at storage offset 4 only allows 4-pixel
    accesses (<4>), a float mask at offset 4 floats keeps the 16-byte alignment (<8>), homo_z at an offset of one float defeats every vector
    access (<1>).  Every output is bit-identical across the forms (the per-pixel arithmetic does not depend on PIX) and matches the oracle."""
    from lc_amd import labels

    gen = torch.Generator().manual_seed(160 + (0 if bits is None else 1))
    hz, Rt, K, msk, sc, T = _label_inputs(gen, 2, 10, 16)
    m = msk if mask == "u8" else msk.float()
    kw = dict(noc_scale=sc.to(DEV), xform=T.to(DEV), bit_cnt=None if bits is None else list(bits), want_targets=True)
    res = []
    for hz_off, m_off in ((0, 0), (0, 4), (1, 0), (1, 4)):
        mm = _at_offset(m.to(torch.uint8) if mask == "u8" else m, m_off)
        res.append(labels._targets(_at_offset(hz, hz_off), Rt.to(DEV), K.to(DEV), msk=mm, **kw))
    for r in res[1:]:
        for a, c in zip(res[0], r):
            assert (a is None) == (c is None) and (a is None or torch.equal(a, c))
    rxyz, rnoc, rtgt, rraw, arg = O.targets(hz.double(), Rt.double(), K.double(), msk, sc.double(), T.double(), None if bits is None else list(bits))
    xyz, noc, tgt, raw = res[0]
    assert ((xyz.cpu().double() - rxyz).abs().max() <= 1e-5 * rxyz.abs().max())
    if bits is None:
        assert ((noc.cpu().double() - rnoc).abs().max() <= 1e-5 * rnoc.abs().max())
    else:
        _check_bits(tgt, rtgt, arg)
        _check_bits(raw, rraw, arg)
