"""Symmetry pose candidates without a GPU: the numpy restatement of the kernel's composition (tests/symcand_oracle.py) against the
reference's own candidates (tests/golden/symcand_*.npz), the per-object tables of lc_amd.symmetry, the combined continuous + discrete case
as a geometric property, the argument checks of the two C entry points, the drop-in's rebinding, and the selection the label goldens
made, repeated on table-made candidates."""
import ctypes
import importlib
import sys
import types

import numpy as np
import pytest
import torch

from tests import labels_oracle as LO
from tests import symcand_oracle as SO
from tests.util import case_name, golden_files

FILES = golden_files("symcand_")


def _transforms(z):
    from lc_amd import symmetry

    return symmetry.symmetry_transforms(SO.model_info_of(z), int(z["steps"]))


def _base32(z):
    return np.concatenate((z["base_R"], z["base_t"][..., None]), -1).astype(np.float32)


def test_goldens_cover_the_issue_s_cases():
    names = {case_name(p, "symcand_") for p in FILES}
    assert names == {"discrete2", "discrete4", "continuous384", "continuous7"}
    for p in FILES:
        z = np.load(p)
        assert z["base_R"].dtype == np.float64 and np.abs(z["base_t"]).max() > 1000
        if "axis" in z.files:
            assert abs(np.linalg.norm(z["axis"]) - 1) < 1e-12 and (np.abs(z["axis"]) >= 0.2).all() and z["offset"].any()


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "symcand_") for p in FILES])
def test_restatement_vs_reference_candidates(path):
    """Both sides are fp64 results rounded once to fp32 (summation order, Rodrigues against scipy: ~1e-16 relative apart), so an entry may
    differ only where its fp64 value sits on a rounding boundary: by one fp32 spacing at the magnitude of the largest of its terms."""
    z = np.load(path)
    R_s, t_s = _transforms(z)
    assert R_s.shape[0] == z["cand"].shape[1]
    base = _base32(z)
    got, want = SO.compose(base, R_s, t_s), z["cand"]
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case_name(path, 'symcand_')}: {int((got != want).sum())} of {got.size} entries not identical, largest difference / bound "
          f"{float((diff / SO.bound(base, R_s, t_s)).max()):.3f}")
    assert (diff <= SO.bound(base, R_s, t_s)).all()
    assert np.array_equal(got[:, 0], base)  # candidate 0 is the base pose


def test_table_indexing_identity_and_order():
    from lc_amd import symmetry

    rng = np.random.default_rng(1)
    S1, S2 = np.eye(4), np.eye(4)
    S1[:3, :3], S1[:3, 3] = np.diag([1.0, -1, -1]), [1.0, 2, 3]
    S2[:3, :3], S2[:3, 3] = np.diag([-1.0, 1, -1]), [0.0, -4, 0]
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    info = {"7": {"symmetries_discrete": [S1.ravel().tolist(), S2.ravel().tolist()]}, 2: {},
            "5": {"symmetries_continuous": [{"axis": axis.tolist(), "offset": [3.0, 0, -2]}]}}
    ids, tr = symmetry.models_info_transforms(info, continuous_steps=6)
    ids, table, off, k = symmetry.host_table(tr, ids)
    assert ids == [2, 5, 7] and k.tolist() == [1, 6, 3] and off.tolist() == [0, 1, 7] and table.shape == (10, 12) and table.dtype == np.float64
    ident = np.concatenate((np.eye(3), np.zeros((3, 1))), -1).ravel()
    for o in off:
        assert np.array_equal(table[o], ident) and not np.signbit(table[o]).any()  # the exact identity, bit for bit
    T = table.reshape(-1, 3, 4)
    assert np.array_equal(T[8], S1[:3]) and np.array_equal(T[9], S2[:3])  # discrete: the identity, then file order
    for c in range(1, 6):  # continuous: angle 2 pi c / C about the axis, t = -R offset + offset
        R = T[1 + c, :, :3]
        assert np.allclose(R @ axis, axis, atol=1e-15) and np.allclose(R @ R.T, np.eye(3), atol=1e-15)
        assert abs(np.trace(R) - (1 + 2 * np.cos(2 * np.pi * c / 6))) < 1e-14
        e1 = np.cross(axis, [1.0, 0, 0])  # a vector across the axis turns counter-clockwise about it (right-handed) for angles below pi
        assert np.sign(np.dot(axis, np.cross(e1, R @ e1))) == (1 if c < 3 else (0 if c == 3 else -1)) or abs(np.dot(axis, np.cross(e1, R @ e1))) < 1e-12
        assert np.allclose(T[1 + c, :, 3], -R @ [3.0, 0, -2] + [3.0, 0, -2], atol=1e-15)
    # a subset, in the caller's order: still sorted by id
    ids2, tr2 = symmetry.models_info_transforms(info, obj_ids=[7, 2])
    assert symmetry.host_table(tr2, ids2)[0] == [2, 7]
    assert symmetry.symmetry_transforms({}, 384)[0].shape == (1, 3, 3)


def test_table_refusals():
    from lc_amd import symmetry

    c = {"axis": [0.0, 0, 1], "offset": [0.0, 0, 0]}
    with pytest.raises(ValueError, match="one continuous"):
        symmetry.symmetry_transforms({"symmetries_continuous": [c, c]})
    with pytest.raises(ValueError, match="non-finite"):
        symmetry.symmetry_transforms({"symmetries_continuous": [{"axis": [0.0, float("nan"), 1], "offset": [0.0, 0, 0]}]})
    bad = np.eye(4)
    bad[1, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        symmetry.symmetry_transforms({"symmetries_discrete": [bad.ravel().tolist()]})
    with pytest.raises(ValueError, match="zero length"):
        symmetry.symmetry_transforms({"symmetries_continuous": [{"axis": [0.0, 0, 0], "offset": [0.0, 0, 0]}]})
    with pytest.raises(ValueError, match="continuous_steps"):
        symmetry.symmetry_transforms({"symmetries_continuous": [c]}, 0)
    with pytest.raises(ValueError, match=r"object 4"):
        symmetry.models_info_transforms({"4": {"symmetries_continuous": [c, c]}})
    with pytest.raises(KeyError, match="no object"):
        symmetry.models_info_transforms({"4": {}}, obj_ids=[4, 9])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        symmetry.SymmetrySet.from_models_info({"4": {}}, device="cpu")
    # an obj_id the set lacks: -1 from the device lookup (no read back; the kernels refuse the row), an error from the host lookup
    s = object.__new__(symmetry.SymmetrySet)
    s.obj_ids, s._lut_host = [2, 5], np.array([-1, -1, 0, -1, -1, 1, -1], np.int32)
    s._lut, s.device = torch.from_numpy(s._lut_host), torch.device("cpu")
    assert s.index_of(torch.tensor([5, 2, 3, 99, -1])).tolist() == [1, 0, -1, -1, -1] and s.index_of([5]).dtype == torch.int32
    assert s.host_index_of([5, 2]).tolist() == [1, 0]
    with pytest.raises(KeyError, match=r"no object \[3, 99\]"):
        s.host_index_of(torch.tensor([5, 3, 99]))
    from lc_amd import labels

    with pytest.raises(TypeError, match="SymmetrySet"):
        labels.set_symmetry_source({"4": {}})
    labels.clear_symmetry_source()
    assert labels._SYM_SOURCE is None


def test_combined_case_keeps_a_cylinder_with_flip_in_place():
    """A continuous z axis and a discrete rotation by pi about x (which the reference refuses): K = D C = 16 with k = d C + c.  Every
    transform maps the vertex set of an 8-sided cylinder with a flip onto itself: rings of 8 vertices at z = zc +- 20 (radius 30) and
    z = zc +- 35 (radius 12) about a centre off the model origin.  Bound 1e-9 of the diameter: fp64 products of a few
    orthonormal matrices and coordinates of the size of the diameter carry ~1e-16 relative error each."""
    from lc_amd import symmetry

    zc = 7.5  # the object's symmetry centre lies off the model origin
    flip = np.eye(4)
    flip[:3, :3] = np.diag([1.0, -1, -1])
    flip[:3, 3] = [0, 0, 2 * zc]  # x -> x, y -> -y, z -> 2 zc - z
    info = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, zc]}], "symmetries_discrete": [flip.ravel().tolist()]}
    R_s, t_s = symmetry.symmetry_transforms(info, 8)
    assert R_s.shape == (16, 3, 3)
    a = 2 * np.pi * np.arange(8) / 8
    V = np.concatenate([np.stack((r * np.cos(a), r * np.sin(a), np.full(8, zc + z)), -1) for r, z in ((30.0, 20.0), (30.0, -20.0), (12.0, 35.0), (12.0, -35.0))])
    diam = np.linalg.norm(V[:, None] - V[None], axis=-1).max()
    for k in range(16):
        W = V @ R_s[k].T + t_s[k]
        d = np.linalg.norm(W[:, None] - V[None], axis=-1)
        assert (d.min(1) <= 1e-9 * diam).all() and (d.min(0) <= 1e-9 * diam).all(), k
        assert len(set(d.argmin(1).tolist())) == len(V)  # a permutation of the set
    # the tables written out by hand: k = d C + c, R = R_c R_d, t = R_c t_d + t_c
    for d_, (Rd, td) in enumerate(((np.eye(3), np.zeros(3)), (flip[:3, :3], flip[:3, 3]))):
        for c in range(8):
            th = 2 * np.pi * c / 8
            Rc = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
            tc = -Rc @ [0, 0, zc] + [0, 0, zc]
            assert np.allclose(R_s[d_ * 8 + c], Rc @ Rd, atol=1e-15, rtol=0) and np.allclose(t_s[d_ * 8 + c], Rc @ td + tc, atol=1e-13, rtol=0), (d_, c)
    assert np.array_equal(R_s[0], np.eye(3)) and not t_s[0].any()
    # a transform that is no symmetry of the set is told apart by the same check
    W = V @ symmetry.rodrigues([0, 0, 1.0], 0.3).T
    assert np.linalg.norm(W[:, None] - V[None], axis=-1).min(1).max() > 1e-3 * diam


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 15) & ~15

    def cand(base=p, idx=p, tab=p, off=p, k=p, n_obj=3, rows=10, row_off=p, B=5, out=p, out_rows=40):
        return lib.lc_sym_candidates_f32(base, idx, tab, off, k, n_obj, rows, row_off, B, out, out_rows, None)

    def sel(base=p, idx=p, tab=p, off=p, k=p, n_obj=3, rows=10, mode=1, a=p, b=p, B=5, N=64, H=8, W=8, ck=p, xyz_map=None, noc_scale=None,
            homo_z=None, dtype=0, bs=0, out=p, K=p):
        return lib.lc_sym_select_table_f32(base, idx, tab, off, k, n_obj, rows, mode, K, a, b, xyz_map, dtype, bs, noc_scale, homo_z, ck, B, N, H, W,
                                           out, None, None)

    err = lib.lc_amd_last_error
    assert cand(B=-1) != 0 and b"size" in err()
    assert cand(n_obj=0) != 0 and b"at least one object" in err()
    assert cand(rows=1 << 28) != 0 and b"2^31" in err()
    assert cand(tab=None) != 0 and b"null" in err()
    assert cand(tab=p + 4) != 0 and b"8-byte" in err()
    assert cand(idx=p + 2) != 0 and b"4-byte" in err()
    assert cand(out_rows=0) != 0 and b"out_rows" in err()
    assert cand(out=None) != 0 and b"null" in err()
    assert cand(out=p + 2) != 0 and b"4-byte" in err()
    assert cand(row_off=p + 1) != 0 and b"row_off" in err()
    assert lib.lc_sym_candidates_f32(None, None, None, None, None, 0, 0, None, 0, None, 0, None) == 0  # an empty batch is a no-op
    assert sel(N=1025) != 0 and b"1024" in err()
    assert sel(mode=2) != 0 and b"mode" in err()
    assert sel(n_obj=0) != 0 and b"at least one object" in err()
    assert sel(base=None) != 0 and b"null" in err()
    assert sel(off=p + 2) != 0 and b"4-byte" in err()
    assert sel(mode=0, b=None) != 0 and b"2D" in err()
    assert sel(a=None) != 0 and b"noc_scale" in err()
    assert sel(b=None) != 0 and b"homo_z" in err()
    assert sel(b=None, homo_z=p, ck=None) != 0 and b"check pixels" in err()
    assert sel(a=None, xyz_map=p, noc_scale=p, dtype=3) != 0 and b"map_dtype" in err()
    assert sel(a=None, xyz_map=p, noc_scale=p, bs=10) != 0 and b"stride" in err()
    assert sel(out=None) != 0 and b"null" in err()
    assert sel(B=0, base=None, tab=None, out=None, K=None) == 0


_STAND_IN = ("import numpy as np\n\ndef symmetry_pose_candidates(base_R, base_t, model_info, continuous_steps=384):\n"
             "    return np.zeros((continuous_steps, 3, 4))\n")


def test_dropin_native_sym_rebinds_the_loader_s_candidates(monkeypatch, tmp_path):
    """A stand-in for the reference's `dataset` (which imports cv2) that calls `symmetry.symmetry_pose_candidates` as dataset.py:15,405 do."""
    from lc_amd import dropin, labels, symmetry as our_sym

    (tmp_path / "symmetry.py").write_text(_STAND_IN)
    monkeypatch.setattr(sys, "path", [str(tmp_path)] + list(sys.path))
    monkeypatch.delitem(sys.modules, "symmetry", raising=False)
    ref_sym = importlib.import_module("symmetry")
    monkeypatch.setitem(sys.modules, "symmetry", ref_sym)
    ds = types.ModuleType("dataset")
    ds.symmetry = ref_sym
    ds.item = lambda R, t: ds.symmetry.symmetry_pose_candidates(R, t, {"symmetries_discrete": []})
    monkeypatch.setitem(sys.modules, "dataset", ds)
    R, t = np.arange(9.0).reshape(3, 3), np.array([1.0, 2, 3])
    assert ds.item(R, t).shape == (384, 3, 4)
    seen = {}
    monkeypatch.setattr(our_sym.SymmetrySet, "from_models_info", classmethod(lambda cls, info, device=None: seen.update(info=info, device=device) or "SET"))
    monkeypatch.setattr(labels, "set_symmetry_source", lambda s: seen.update(source=s))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    assert dropin._install_sym("/data/models_info.json") is True
    assert seen == dict(info="/data/models_info.json", device=torch.device("cuda", 0), source="SET")
    got = ds.item(R, t)
    assert got.shape == (1, 3, 4) and np.array_equal(got[0], np.concatenate((R, t[:, None]), -1))
    fn = ref_sym.symmetry_pose_candidates
    assert dropin._detach_loader_from_candidates() is True and ref_sym.symmetry_pose_candidates is fn  # idempotent
    # without the loader module the top-level `symmetry` is the one the loader would call
    monkeypatch.setitem(sys.modules, "dataset", None)
    assert dropin._detach_loader_from_candidates() is True
    monkeypatch.setitem(sys.modules, "symmetry", None)
    assert dropin._detach_loader_from_candidates() is False


def test_dropin_takes_the_native_sym_flag(monkeypatch, tmp_path):
    from lc_amd import dropin

    seen = {}
    monkeypatch.setattr(dropin, "install", lambda **kw: seen.update(kw) or {})
    script = tmp_path / "train.py"
    script.write_text("import sys\nARGS = list(sys.argv)\n")
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    dropin.main(["--native-sym", "/data/models_info.json", str(script), "--cfg", "x.yaml"])
    assert seen == dict(native_labels=False, native_sym="/data/models_info.json") and sys.argv == [str(script), "--cfg", "x.yaml"]
    with pytest.raises(SystemExit):
        dropin.main(["--native-sym"])


def _label_case(name):
    """A labels_*.npz case as float64 tensors, its table-made candidates per row and the index the golden chose per row."""
    from lc_amd import symmetry

    z = np.load(golden_files("labels_" + name)[0])
    info, rows = SO.labels_info()
    tr = {int(o): symmetry.symmetry_transforms(m, 384) for o, m in info.items()}
    base = np.concatenate((z["in_R_no_aug"], z["in_t_no_aug"][..., None]), -1).astype(np.float32)
    cands = SO.batch_candidates(base, tr, rows[name])
    golden_idx, r = [], 0
    chunks = [z[k] for k in sorted((k for k in z.files if k.startswith("in_Rt_candi_")), key=lambda k: int(k.rsplit("_", 1)[1]))]
    for c in chunks:
        for i in range(c.shape[0]):
            hit = np.nonzero((c[i] == z["f32_Rt_best"][r + i]).all(-1).all(-1))[0]
            golden_idx.append(int(hit[0]))
            assert cands[r + i].shape == c[i].shape
            r_bound = SO.bound(base[r + i:r + i + 1], *tr[rows[name][r + i]])[0]
            # the stored candidates were formed from the fp64 base poses BEFORE their rounding to fp32: half a spacing of every product and of
            # t_b from that rounding (2 spacings of the largest term at most) next to the two final roundings (half a spacing each)
            assert (np.abs(cands[r + i].astype(np.float64) - c[i]) <= 3 * r_bound).all()
        r += c.shape[0]
    return z, cands, golden_idx


@pytest.mark.parametrize("name", ["discrete3d", "continuous3d", "pts2d"])
def test_fp64_oracle_on_table_made_candidates_picks_the_golden_s_index(name):
    """A condition, not a tolerance: no row of these files is a near-tie that a one-spacing change of a candidate flips (none is left out)."""
    from oracle import floatbits_oracle as FO

    z, cands, golden_idx = _label_case(name)
    T = lambda k: torch.from_numpy(z[k]).double() if z[k].dtype.kind == "f" else torch.from_numpy(z[k])
    B = len(cands)
    if name == "pts2d":
        mode, K, a, b = 0, T("in_out_K"), T("in_pts3d"), T("out_pts2d")
    else:
        H, W = z["in_homo_z_out"].shape[1:3]
        gt = {"sym_ck_pts2d": T("in_sym_ck_pts2d"), "homo_z_out": T("in_homo_z_out"), "noc_scale": T("in_noc_scale")}
        out = {"xyz_noc": T("out_xyz_noc")} if "out_xyz_noc" in z.files else {}
        hz, p, pix = LO.gather_check_points(gt, out, H, W)
        if p is None:  # code head: losses.py:17-45 at the check pixels
            lg = T("out_xyz_noc_bin").reshape(B, -1, H * W)
            lg = torch.gather(lg, 2, pix[:, None, :].expand(-1, lg.shape[1], -1))[..., None]  # (B,C,N,1)
            noc = FO.nn_logits2noc(lg, [int(n) for n in z["bit_cnt"]])[:, :, 0]  # (B,N,3)
            Tm = T("in_model_transform")
            p = (noc * gt["noc_scale"][:, None] - Tm[:, None, :3, 3]) @ Tm[:, :3, :3]
        mode, K, a, b = 1, T("in_K_no_aug"), p, hz
    for r in range(B):
        c = torch.from_numpy(cands[r]).double()[None]
        if c.shape[1] == 1:
            assert golden_idx[r] == 0
            continue
        e = LO.candidate_errors(mode, K[r:r + 1], a[r:r + 1], b[r:r + 1], c)[0]
        assert int(torch.argmin(e)) == golden_idx[r], (name, r, int(torch.argmin(e)), golden_idx[r])
