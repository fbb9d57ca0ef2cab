"""GPU tests of the symmetry pose candidates formed on the device (lc_amd.symmetry, lc_labels.hip): lc_sym_candidates_f32 bit for bit
against the numpy restatement (tests/symcand_oracle.py) and within the rounding bound of the reference's own candidates;
lc_sym_select_table_f32 bit for bit against materialise-then-lc_sym_select_f32; annots_on_the_fly with a symmetry source against the
reference's label goldens with `Rt_candi` removed; one captured graph replayed on another mix of objects."""
import numpy as np
import pytest
import torch

from tests import labels_oracle as LO
from tests import symcand_oracle as SO
from tests.test_gpu_labels import _acceptable, _check_bits, _clear, _dev, _load
from tests.util import case_name, golden_files

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KS = [1, 2, 3, 4, 7, 384, 768, 1024, 1025]  # 1024 is the last count staged in LDS (kSelLdsCands)
MANY = list(range(2, 42))  # 40 distinct candidate counts: more than the 32 chunks lc_sym_select_f32 takes
_CACHE = {}


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _discrete(rng, D):
    out = []
    for _ in range(D - 1):
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = _rot(rng), rng.uniform(-30, 30, 3)
        out.append(S.ravel().tolist())
    return out


def _symset():
    """Objects K (id = K) for K in KS and 2000 + D for D in MANY.  384 = one continuous symmetry, 768 = the same with one discrete
    symmetry (the combined case), every other count the identity and D - 1 random rigid transforms."""
    if "set" not in _CACHE:
        from lc_amd import symmetry

        rng = np.random.default_rng(5)
        axis = np.array([0.48, -0.6, 0.64])
        cont = [{"axis": axis.tolist(), "offset": [4.0, -7.0, 11.0]}]
        info = {}
        for K in KS:
            info[K] = {384: {"symmetries_continuous": cont}, 768: {"symmetries_continuous": cont, "symmetries_discrete": _discrete(rng, 2)}}.get(
                K, {"symmetries_discrete": _discrete(rng, K)} if K > 1 else {})
        for D in MANY:
            info[2000 + D] = {"symmetries_discrete": _discrete(rng, D)}
        _CACHE["set"] = symmetry.SymmetrySet.from_models_info(info, device=DEV)
        assert _CACHE["set"].max_k == 1025
    return _CACHE["set"]


def _tr(symset, i):
    """Transforms of table index i, from the host copy of the table."""
    o, k = int(symset.obj_off_host[i]), int(symset.obj_k_host[i])
    T = symset.table_host[o:o + k].reshape(k, 3, 4)
    return T[:, :, :3], T[:, :, 3]


def _poses(rng, B):
    R = np.stack([_rot(rng) for _ in range(B)])
    t = np.stack([rng.uniform(-20, 20, B), rng.uniform(-20, 20, B), rng.uniform(550, 650, B)], -1)
    return np.concatenate((R, t[..., None]), -1).astype(np.float32)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _expected(symset, base, obj):
    idx = symset.host_index_of(obj)
    return [SO.compose(base[b:b + 1], *_tr(symset, i))[0] for b, i in enumerate(idx)]


@pytest.mark.parametrize("K", KS)
def test_candidates_bit_for_bit_vs_restatement(K):
    from lc_amd import labels

    symset = _symset()
    rng = np.random.default_rng(K)
    for B in (1, 5):
        base = _poses(rng, B)
        got = labels.symmetry_pose_candidates(torch.from_numpy(base[:, :, :3]).to(DEV), torch.from_numpy(base[:, :, 3]).to(DEV), symset, [K] * B)
        assert got.shape == (B, K, 3, 4) and got.dtype == torch.float32
        want = torch.from_numpy(np.stack(_expected(symset, base, [K] * B)))
        assert torch.equal(_bits(got), _bits(want)), (K, B)
        assert torch.equal(_bits(got[:, 0]), _bits(torch.from_numpy(base)))  # candidate 0 is the base pose


def test_candidates_of_a_mixed_batch_in_scrambled_object_order():
    from lc_amd import labels

    symset = _symset()
    rng = np.random.default_rng(77)
    obj = [384, 1, 1025, 2, 768, 3, 1024, 4, 7, 1, 384, 2002, 1025, 7]
    base = _poses(rng, len(obj))
    R, t = torch.from_numpy(base[:, :, :3]).to(DEV), torch.from_numpy(base[:, :, 3]).to(DEV)
    got = labels.symmetry_pose_candidates_list(R, t, symset, torch.tensor(obj, device=DEV))
    want = _expected(symset, base, obj)
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want]
    for b, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(_bits(g), _bits(torch.from_numpy(w))), b
    with pytest.raises(ValueError, match="symmetry_pose_candidates_list"):
        labels.symmetry_pose_candidates(R, t, symset, obj)
    with pytest.raises(KeyError, match="no object"):
        labels.symmetry_pose_candidates_list(R[:1], t[:1], symset, [5])
    # a row the table does not hold, or whose rows would leave the output, is not written (nothing is read for it)
    from lc_amd import _lib

    out = torch.full((8, 3, 4), -5.0, device=DEV)
    idx = torch.tensor([-1, 1, 99, 3], dtype=torch.int32, device=DEV)  # table indices: 1 -> K = 2, 3 -> K = 4
    row_off = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=DEV)  # the last row would need rows 6..9 of 8
    b4 = labels._base_pose(symset, R[:4], t[:4])
    rc = _lib.load().lc_sym_candidates_f32(_lib.ptr(b4), _lib.ptr(idx), *labels._table_args(symset), _lib.ptr(row_off), 4, _lib.ptr(out), 8,
                                           _lib.stream_ptr(DEV))
    assert rc == 0
    keep = torch.ones(8, dtype=torch.bool)
    keep[2:4] = False
    assert (out.cpu()[keep] == -5.0).all() and torch.equal(_bits(out[2:4]), _bits(torch.from_numpy(SO.compose(base[1:2], *_tr(symset, 1))[0])))


FILES = golden_files("symcand_")


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "symcand_") for p in FILES])
def test_candidates_vs_reference_goldens(path):
    """Within one fp32 spacing at the magnitude of the largest term of each entry (both sides: fp64, rounded once)."""
    from lc_amd import labels, symmetry

    z = np.load(path)
    info = SO.model_info_of(z)
    symset = symmetry.SymmetrySet.from_models_info({"3": info}, continuous_steps=int(z["steps"]), device=DEV)
    base = np.concatenate((z["base_R"], z["base_t"][..., None]), -1).astype(np.float32)
    got = labels.symmetry_pose_candidates(torch.from_numpy(z["base_R"]).to(DEV), torch.from_numpy(z["base_t"]).to(DEV), symset, [3] * len(base))
    R_s, t_s = symmetry.symmetry_transforms(info, int(z["steps"]))
    diff = np.abs(got.cpu().numpy().astype(np.float64) - z["cand"].astype(np.float64))
    print(f"{case_name(path, 'symcand_')}: {int((got.cpu().numpy() != z['cand']).sum())} of {diff.size} entries not identical")
    assert (diff <= SO.bound(base, R_s, t_s)).all()


def _scene(rng, symset, obj, N, mode, H=16, W=16):
    """Inputs of a selection whose observations follow candidate kt[b] of every row, plus noise."""
    B = len(obj)
    base = _poses(rng, B)
    cands = _expected(symset, base, obj)
    kt = [int(rng.integers(0, len(c))) for c in cands]
    P = np.stack([c[k] for c, k in zip(cands, kt)]).astype(np.float64)
    Kc = np.zeros((B, 3, 3))
    Kc[:, 0, 0], Kc[:, 1, 1], Kc[:, 0, 1] = rng.uniform(90, 110, B), rng.uniform(90, 110, B), rng.uniform(-1, 1, B)
    Kc[:, 0, 2], Kc[:, 1, 2], Kc[:, 2, 2] = W / 2 + rng.uniform(-2, 2, B), H / 2 + rng.uniform(-2, 2, B), 1
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    kw = dict(cam_K=f(Kc))
    if mode == 0:
        pts3d = rng.uniform(-50, 50, (B, N, 3))
        h = np.einsum("bij,bnj->bni", Kc, np.einsum("bij,bnj->bni", P[:, :, :3], pts3d) + P[:, None, :, 3])
        kw.update(pts_a=f(pts3d), pts_b=f(h[..., :2] / h[..., 2:] + rng.normal(scale=0.5, size=(B, N, 2))))
    else:
        v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        z = P[:, 2, 3, None, None] + rng.uniform(-40, 40, (B, H, W))
        hz = np.stack([u[None] * z, v[None] * z, z], -1)
        q = np.einsum("bij,bhwj->bhwi", np.linalg.inv(Kc), hz)
        xyz = np.einsum("bji,bhwj->bhwi", P[:, :, :3], q - P[:, None, None, :, 3])
        sc = rng.uniform(110, 140, (B, 3))
        noc = (xyz / sc[:, None, None]).transpose(0, 3, 1, 2) + rng.normal(scale=0.02, size=(B, 3, H, W))
        ck = np.stack((rng.integers(0, W, (B, N)), rng.integers(0, H, (B, N))), -1)
        kw.update(xyz_map=f(noc), noc_scale=f(sc), homo_z=f(hz), ck=torch.from_numpy(ck).to(DEV))
    return base, kw, kt


def _both(symset, base, obj, kw, mode, N):
    """(table launch, materialise + lc_sym_select_f32 on one-row chunks): each (Rt_best, best_idx)."""
    from lc_amd import labels

    K = kw.pop("cam_K")
    R, t = torch.from_numpy(base[:, :, :3]).to(DEV), torch.from_numpy(base[:, :, 3]).to(DEV)
    table = (symset, labels._base_pose(symset, R, t), symset.index_of(torch.tensor(obj, device=DEV)))
    got = labels._select(mode, None, K, N, table=table, **kw)
    rows = labels.symmetry_pose_candidates_list(R, t, symset, obj)
    want = labels._select(mode, [r[None] for r in rows], K, N, **kw)
    kw["cam_K"] = K
    return got, want


MIXED = [384, 1, 1025, 2, 768, 3, 1024, 4, 7, 1, 384, 1025]


@pytest.mark.parametrize("mode,N", [(1, 1), (1, 64), (1, 65), (1, 256), (0, 8)], ids=["3d-n1", "3d-n64", "3d-n65", "3d-n256", "2d-n8"])
def test_select_table_equals_materialise_then_select(mode, N):
    """Every K of KS in one scrambled batch, the 3D mode through ck + homo_z + the xyz map; row 3 has only -1 check points; then the same
    batch with a NaN in row 0's base pose (K = 384): that row chooses index 0 and no other row changes."""
    symset = _symset()
    rng = np.random.default_rng(100 * mode + N)
    base, kw, kt = _scene(rng, symset, MIXED, N, mode)
    if mode == 1:
        kw["ck"][3] = -1
    (Rt, idx), (Rt0, idx0) = _both(symset, base, MIXED, kw, mode, N)
    assert torch.equal(idx, idx0) and torch.equal(_bits(Rt), _bits(Rt0))
    want = _expected(symset, base, MIXED)
    for b, k in enumerate(idx.tolist()):
        assert 0 <= k < len(want[b]) and torch.equal(_bits(Rt[b]), _bits(torch.from_numpy(want[b][k])))
        if len(want[b]) == 1:
            assert k == 0 and torch.equal(_bits(Rt[b]), _bits(torch.from_numpy(base[b])))
    assert any(k > 0 for k in idx.tolist())  # the observations follow candidate kt of every row, not the base pose
    nan = base.copy()
    nan[0, 1, 2] = np.nan
    (Rn, idn), (Rn0, idn0) = _both(symset, nan, MIXED, kw, mode, N)
    assert torch.equal(idn, idn0) and torch.equal(_bits(Rn), _bits(Rn0))
    assert int(idn[0]) == 0 and torch.equal(_bits(Rn[0]), _bits(torch.from_numpy(nan[0])))
    assert torch.equal(idn[1:], idx[1:]) and torch.equal(_bits(Rn[1:]), _bits(Rt[1:]))


def test_select_table_with_more_distinct_counts_than_the_chunk_table_takes():
    """40 rows of 40 different K in one launch, against the fp64 oracle on the restated candidates; an unknown object gives NaN and -1."""
    from lc_amd import labels

    symset = _symset()
    rng = np.random.default_rng(9)
    obj = [2000 + D for D in rng.permutation(MANY)]
    N = 64
    base, kw, kt = _scene(rng, symset, obj, N, 0)
    K = kw.pop("cam_K")
    R, t = torch.from_numpy(base[:, :, :3]).to(DEV), torch.from_numpy(base[:, :, 3]).to(DEV)
    ids = torch.tensor(obj, device=DEV)
    ids[5] = 999999  # no such object
    Rt, idx = labels._select(0, None, K, N, table=(symset, labels._base_pose(symset, R, t), symset.index_of(ids)), **kw)
    want = _expected(symset, base, obj)
    assert int(idx[5]) == -1 and torch.isnan(Rt[5]).all()
    errs = []
    for b in range(len(obj)):
        e, _ = LO.select(0, K[b:b + 1].cpu().double(), kw["pts_a"][b:b + 1].cpu().double(), kw["pts_b"][b:b + 1].cpu().double(),
                         [torch.from_numpy(want[b]).double()[None]])
        errs += e
    rows = [b for b in range(len(obj)) if b != 5]
    got = idx.cpu().long()
    _acceptable([errs[b] for b in rows], got[rows])
    clear = torch.tensor(_clear([errs[b] for b in rows]))
    best = torch.stack([torch.argmin(errs[b]) for b in rows])
    assert torch.equal(got[rows][clear], best[clear])
    for b in rows:
        assert torch.equal(_bits(Rt[b]), _bits(torch.from_numpy(want[b][int(got[b])])))


LABEL_FILES = golden_files("labels_")


def _label_symset():
    if "labels" not in _CACHE:
        from lc_amd import symmetry

        info, rows = SO.labels_info()
        _CACHE["labels"] = (symmetry.SymmetrySet.from_models_info(info, device=DEV), info, rows)
    return _CACHE["labels"]


@pytest.fixture
def label_source():
    from lc_amd import labels

    symset, info, rows = _label_symset()
    labels.set_symmetry_source(symset)
    yield symset, info, rows
    labels.clear_symmetry_source()


def _without_candidates(gt, obj):
    g = {k: v for k, v in gt.items() if k != "Rt_candi"}
    g["obj_id"] = torch.tensor(obj)
    return g


@pytest.mark.parametrize("path", LABEL_FILES, ids=[case_name(p, "labels_") for p in LABEL_FILES])
def test_annots_on_the_fly_with_a_symmetry_source_vs_reference(path, label_source):
    """The reference's label goldens with `Rt_candi` taken out of gt_dict: Rt_best within the candidate bound of the reference's, exactly
    the base pose where nothing is chosen (no symmetry, not started), xyz_gt and the targets within test_gpu_labels' tolerances."""
    from lc_amd import labels, symmetry

    symset, info, rows = label_source
    name = case_name(path, "labels_")
    z, gt, out, cfg, step = _load(path)
    g, o = _dev(_without_candidates(gt, rows[name])), _dev(out)
    labels.annots_on_the_fly(g, o, cfg, step)
    f64 = lambda k: torch.from_numpy(z["f64_" + k]).double()
    want = torch.from_numpy(z["f32_Rt_best"])
    B = want.shape[0]
    base = torch.cat((gt["R_no_aug"], gt["t_no_aug"][..., None]), -1)
    got = g["Rt_best"].cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape
    if name in ("nosym", "notstarted"):
        assert torch.equal(_bits(got), _bits(base)) and torch.equal(got, want)
    else:
        cand = gt["Rt_candi"]
        chosen = [int((c[i] == want[r + i]).all(-1).all(-1).nonzero()[0]) for c, r in zip(cand, np.cumsum([0] + [c.shape[0] for c in cand])) for i in range(c.shape[0])]
        for b in range(B):
            tr = symmetry.symmetry_transforms(info[str(rows[name][b])], 384)
            bound = SO.bound(base[b:b + 1].numpy(), *tr)[0][chosen[b]]
            d = (got[b].double() - want[b].double()).abs().numpy()
            print(f"{name} row {b}: candidate {chosen[b]}, largest difference / bound {float((d / bound).max()):.3f}")
            assert (d <= bound).all(), (b, chosen[b])
    T = gt.get("model_transform")
    xyz, noc, tgt, raw, arg = LO.targets(gt["homo_z_out"].double(), got.double(), gt["K_no_aug"].double(), gt["msk_noc"], gt["noc_scale"].double(),
                                         None if T is None else T.double(), gt.get("bit_cnt"))
    assert ((g["xyz_gt"].cpu().double() - xyz).abs().max() <= 1e-5 * xyz.abs().max())
    assert ((g["xyz_gt"].cpu().double() - f64("xyz_gt")).abs().max() <= 1e-5 * f64("xyz_gt").abs().max())
    if noc is not None:
        assert ((g["xyz_noc_tgt"].cpu().double() - noc).abs().max() <= 1e-5 * noc.abs().max())
    else:
        _check_bits(g["xyz_noc_bin_tgt"], tgt, arg)
        _check_bits(g["xyz_noc_bin_raw"], raw, arg)
        _check_bits(g["xyz_noc_bin_tgt"], torch.from_numpy(z["f64_xyz_noc_bin_tgt"]), arg)
    g2 = _dev(_without_candidates(gt, rows[name]))
    Rt_best, pose_best, xyz_gt = labels.selete_best_pose(g2, o, step >= cfg.get("sym_aware_start", 0))
    assert torch.equal(Rt_best, g["Rt_best"]) and torch.equal(xyz_gt, g["xyz_gt"]) and torch.equal(pose_best, g["pose_best"])


def test_one_captured_graph_serves_another_mix_of_objects(label_source):
    from lc_amd import labels

    symset, info, rows = label_source
    z, gt, out, cfg, step = _load(golden_files("labels_discrete3d")[0])
    g, o = _dev(_without_candidates(gt, rows["discrete3d"])), _dev(out)  # objects 1 1 2 2 2
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
    # a second batch in the captured buffers: other objects per row (2 3 1 3 2: K = 4, 384, 1, 384, 4), other poses, depth and logits
    gen = torch.Generator().manual_seed(3)
    new = dict(obj_id=torch.tensor([2, 3, 1, 3, 2]), R_no_aug=gt["R_no_aug"].flip(0).contiguous(), t_no_aug=gt["t_no_aug"].flip(0).contiguous(),
               homo_z_out=gt["homo_z_out"] * (1 + 0.01 * torch.rand(gt["homo_z_out"].shape, generator=gen)))
    new_logits = torch.randn(o["xyz_noc_bin"].shape, generator=gen)
    for k, v in new.items():
        g[k].copy_(v.to(DEV))
    o["xyz_noc_bin"].copy_(new_logits.to(DEV))
    gg.replay()
    torch.cuda.synchronize()
    e = _dev({**_without_candidates(gt, rows["discrete3d"]), **new})
    labels.annots_on_the_fly(e, {"xyz_noc_bin": new_logits.to(DEV)}, cfg, step)
    for k in ("Rt_best", "pose_best", "xyz_gt", "xyz_noc_bin_tgt", "xyz_noc_bin_raw"):
        assert torch.equal(g[k], e[k]), k
    assert torch.equal(_bits(e["Rt_best"][2]), _bits(torch.cat((new["R_no_aug"], new["t_no_aug"][..., None]), -1)[2]))  # the K = 1 row
