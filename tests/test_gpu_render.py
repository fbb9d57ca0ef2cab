"""The depth rasteriser (lc_amd.render, lc_amd/csrc/render/lc_render.hip) on the GPU against the fp64 oracle of tests/render_oracle.py
on the cases of tests/render_cases.py: mask, hit pattern and info exact, face exact off the tie pixels, z within the tolerance the
oracle's own fp32 evaluation sets, identical bits for every order of the faces; the crop form, the labels' depth source, graph capture and
the offline tool."""
import gzip
import json
import os
import pickle
import struct

import numpy as np
import pytest
import torch

from tests import render_cases as rc
from tests import render_oracle as ro

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = list(rc.MESHES)
HALF_ULP = 0.5 * (1 + 2.0 ** -20)  # one fp32 rounding of a product; the slack covers the fp64 rounding of the test's own product


@pytest.fixture(scope="module")
def meshes():
    """Every mesh of the cases, then every mesh again with its faces in reverse order."""
    from lc_amd.render import MeshSet

    fwd = [rc.MESHES[n] for n in NAMES]
    rev = [(v, f[::-1].copy()) for v, f in fwd]
    return MeshSet(fwd + rev, DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _render(meshes, rows, size_hw, reverse=False, **kw):
    """rows: [(mesh name, Pose, K)]."""
    from lc_amd.render import render_depth

    idx = torch.tensor([NAMES.index(m) + (len(NAMES) if reverse else 0) for m, _, _ in rows], dtype=torch.int32, device=DEV)
    R, t, K = (_dev(np.stack(x)) for x in zip(*[(p.R, p.t, k) for _, p, k in rows]))
    return render_depth(meshes, idx, R, t, K, size_hw, near=rc.NEAR, far=rc.FAR, **kw)


def _check_image(out, b, ref, K, center=(0.5, 0.5)):
    depth, mask, face, homo = (x[b].cpu().numpy() for x in (out.depth, out.mask, out.face, out.homo_z))
    assert np.array_equal(mask, ref.mask), f"mask differs on {(mask != ref.mask).sum()} pixels"
    assert np.array_equal(depth > 0, ref.mask) and np.array_equal(face >= 0, ref.mask)
    assert int(out.info[b]) == ref.info
    tol = ro.z_tolerance(ref)
    ties = ro.tie_pixels(ref, tol)
    assert np.array_equal(face[~ties], ref.face[~ties]), f"face differs on {(face != ref.face)[~ties].sum()} non-tie pixels"
    if ref.mask.any():
        err = (np.abs(depth.astype(np.float64) - ref.z64)[ref.mask] / ref.z64[ref.mask]).max()
        print(f"max rel z error {err:.3e} (bound {tol:.3e}), ties {ties.sum()}/{ref.mask.sum()}")
        assert err <= tol
    H, W = ref.mask.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + center[0], np.arange(H, dtype=np.float64) + center[1])
    z = depth.astype(np.float64)
    for c, p in enumerate((xs, ys)):  # one fp32 rounding of each product
        want = p * z
        assert (np.abs(homo[..., c] - want) <= np.spacing(np.abs(want).astype(np.float32)) * HALF_ULP).all()
    assert np.array_equal(homo[..., 2], depth)


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_case_vs_fp64_oracle(meshes, name):
    c = next(c for c in rc.CASES if c.name == name)
    out = _render(meshes, [(c.mesh, c.pose, c.K)], c.size_hw, want_face=True, want_homo=True)
    _check_image(out, 0, rc.reference(name), c.K)


def _mixed_rows():
    K = rc.camera((64, 64))
    return [(m or "torus", rc.POSES[m] if m else rc.OUT_OF_VIEW, K) for m in rc.MIXED]


def test_mixed_batch_through_mesh_index(meshes):
    rows = _mixed_rows()
    out = _render(meshes, rows, (64, 64), want_face=True, want_homo=True)
    for b, (m, pose, K) in enumerate(rows):
        v, f = rc.MESHES[m]
        ref = ro.render(v, f, pose.R, pose.t, K, (64, 64), rc.NEAR, rc.FAR)
        assert ref.margin >= 2.0 ** -30
        _check_image(out, b, ref, K)
    assert not out.mask[2].any() and int(out.info[2]) == 0  # the out-of-view row
    assert torch.equal(out.depth[0], out.depth[3])  # the repeated mesh


def test_unknown_mesh_index_renders_nothing(meshes):
    from lc_amd.render import render_depth

    rows = _mixed_rows()[:2]
    R, t, K = (_dev(np.stack(x)) for x in zip(*[(p.R, p.t, k) for _, p, k in rows]))
    idx = torch.tensor([-1, 10 ** 6], dtype=torch.int32, device=DEV)
    out = render_depth(meshes, idx, R, t, K, (33, 47), near=rc.NEAR, far=rc.FAR, want_face=True)
    assert not out.mask.any() and (out.depth == 0).all() and (out.face == -1).all() and out.info.tolist() == [-1, -1]


def test_bits_do_not_depend_on_call_or_face_order(meshes):
    """Two calls agree, and the meshes with their faces reversed give the same depth bits and, mapped back, the same faces off the tie
    pixels: an implementation whose winner depends on the order of evaluation fails this."""
    for size in ((64, 64), (33, 47)):
        K = rc.camera(size)
        rows = [(m, rc.POSES[m], K) for m in NAMES]
        a = _render(meshes, rows, size, want_face=True, want_homo=True)
        b = _render(meshes, rows, size, want_face=True, want_homo=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        r = _render(meshes, rows, size, reverse=True, want_face=True, want_homo=True)
        assert torch.equal(a.depth.view(torch.int32), r.depth.view(torch.int32)) and torch.equal(a.mask, r.mask) and torch.equal(a.homo_z, r.homo_z)
        assert torch.equal(a.info, r.info)
        for i, m in enumerate(NAMES):
            nf = len(rc.MESHES[m][1])
            ref = rc.reference(f"{m}-{size[0]}x{size[1]}")
            keep = torch.from_numpy(ref.mask & ~ro.tie_pixels(ref, ro.z_tolerance(ref))).to(DEV)
            assert torch.equal(a.face[i][keep], (nf - 1 - r.face[i])[keep])


def _crop_setup(B=3, size=(64, 64)):
    """Full-frame cameras, poses in metres, and the crop out_K = A K of a rotated, scaled window (dataset.py:409-423)."""
    names = ["ico", "torus", "box"][:B]
    Kf = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    outK, poses = [], []
    for i, m in enumerate(names):
        p = rc.POSES[m]
        poses.append(p)
        c = (Kf.astype(np.float64) @ (p.t.astype(np.float64) / p.t[2]))[:2]  # the object's centre in the frame
        s = size[1] / (300.0 + 40 * i)
        th = np.deg2rad(17.0 * i)
        A = np.eye(3)
        A[:2, :2] = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        A[:2, 2] = np.array([size[1] / 2, size[0] / 2]) - A[:2, :2] @ c
        outK.append((A.astype(np.float32) @ Kf).astype(np.float32))
    return names, poses, np.stack([Kf] * B), np.stack(outK)


def test_render_homo_z_out_vs_oracle_and_back_projection(meshes):
    from lc_amd import labels
    from lc_amd.render import crop_matrices, render_homo_z_out

    size = (64, 64)
    names, poses, Kf, outK = _crop_setup()
    idx = torch.tensor([NAMES.index(m) for m in names], dtype=torch.int32, device=DEV)
    R, t = _dev(np.stack([p.R for p in poses])), _dev(np.stack([p.t for p in poses]))
    hz, msk = render_homo_z_out(meshes, idx, R, t, _dev(Kf), _dev(outK), size, near=rc.NEAR, far=rc.FAR)
    Kr, pix2k = (x.cpu().numpy() for x in crop_matrices(_dev(Kf), _dev(outK)))
    xyz = labels.xyz_from_homo_z(hz, R, t, _dev(Kf)).cpu().numpy()
    hz, msk = hz.cpu().numpy(), msk.cpu().numpy()
    xs, ys = np.meshgrid(np.arange(size[1], dtype=np.float64), np.arange(size[0], dtype=np.float64))
    for b, m in enumerate(names):
        v, f = rc.MESHES[m]
        ref = ro.render(v, f, poses[b].R, poses[b].t, Kr[b], size, rc.NEAR, rc.FAR, center=(0.0, 0.0))
        assert ref.margin >= 2.0 ** -30 and ref.mask.sum() > 200
        assert np.array_equal(msk[b], ref.mask)
        tol = ro.z_tolerance(ref)
        z = hz[b, ..., 2].astype(np.float64)
        assert (np.abs(z - ref.z64)[ref.mask] / ref.z64[ref.mask]).max() <= tol
        M = pix2k[b].astype(np.float64)
        for c in range(2):
            want = (M[c, 0] * xs + M[c, 1] * ys + M[c, 2]) * z
            assert (np.abs(hz[b, ..., c] - want) <= HALF_ULP * np.spacing(np.abs(want).astype(np.float32))).all()
        # back-projection: the oracle's fp64 intersection points on the rays of the render camera, in model coordinates
        cam = ro.points(ref, Kr[b], center=(0.0, 0.0))
        R64, t64 = poses[b].R.astype(np.float64), poses[b].t.astype(np.float64)
        want = (cam - t64) @ R64  # R^T (x - t)
        # 1e-3 mm (the poses are in metres: 1e-6) + 4 ulp of fp32 at the camera-space magnitude the fp32 back-projection cancels at
        bound = 1e-6 + 4 * np.spacing(np.float32(np.abs(cam).max()))
        err = np.abs(xyz[b] - want)[ref.mask].max()
        print(f"{m}: back-projection error {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def _label_dicts(meshes, size=(64, 64)):
    names, poses, Kf, outK = _crop_setup()
    B = len(names)
    R, t = np.stack([p.R for p in poses]), np.stack([p.t for p in poses])
    Rt = torch.from_numpy(np.concatenate((R, t[:, :, None]), -1))
    gt = dict(Rt_candi=[Rt[:, None]], R_no_aug=torch.from_numpy(R), t_no_aug=torch.from_numpy(t), K_no_aug=torch.from_numpy(Kf),
              out_K=torch.from_numpy(outK), noc_scale=torch.full((B, 3), 0.3), obj_id=torch.tensor([NAMES.index(m) for m in names]),
              sym_ck_pts2d=torch.zeros(B, 256, 2, dtype=torch.int64))
    gt = {k: ([c.to(DEV) for c in v] if isinstance(v, list) else v.to(DEV)) for k, v in gt.items()}
    out = {"xyz_noc": torch.zeros(B, 3, *size, device=DEV)}
    return gt, out


def test_annots_on_the_fly_renders_missing_depth_only(meshes):
    from lc_amd import labels
    from lc_amd.render import render_homo_z_out

    size = (64, 64)
    gt, out = _label_dicts(meshes, size)
    hz, msk = render_homo_z_out(meshes, meshes.index_of(gt["obj_id"]), gt["R_no_aug"], gt["t_no_aug"], gt["K_no_aug"], gt["out_K"], size,
                                near=rc.NEAR, far=rc.FAR)
    assert msk.sum() > 600
    explicit = dict(gt, homo_z_out=hz, msk_noc=msk)
    labels.annots_on_the_fly(explicit, out, {}, 0)
    try:
        labels.set_depth_source(meshes, rc.NEAR, rc.FAR)
        sourced = dict(gt)
        labels.annots_on_the_fly(sourced, out, {}, 0)
        present = dict(gt, homo_z_out=hz * 1.5, msk_noc=msk)  # with the key present the source is not consulted
        labels.annots_on_the_fly(present, out, {}, 0)
    finally:
        labels.clear_depth_source()
    plain = dict(gt, homo_z_out=hz * 1.5, msk_noc=msk)
    labels.annots_on_the_fly(plain, out, {}, 0)
    for a, b in ((sourced, explicit), (present, plain)):
        assert set(a) == set(b)
        for k in ("homo_z_out", "msk_noc", "Rt_best", "pose_best", "xyz_gt", "xyz_noc_tgt"):
            assert torch.equal(a[k], b[k]), k
    missing = dict(gt)
    with pytest.raises(KeyError):
        labels.annots_on_the_fly(missing, out, {}, 0)  # no source, no key: today's behaviour


def test_graph_capture_replays_like_eager(meshes):
    from lc_amd.render import render_depth

    size, names = (64, 64), ["ico", "torus", "box", "fan"]
    K = _dev(np.stack([rc.camera(size)] * 4))
    idx = torch.tensor([NAMES.index(m) for m in names], dtype=torch.int32, device=DEV)
    R1, t1 = np.stack([rc.POSES[m].R for m in names]), np.stack([rc.POSES[m].t for m in names])
    R2 = np.stack([rc.rot((0.2, 1, 0.4), 20.0 + 10 * i) @ R1[i] for i in range(4)]).astype(np.float32)
    t2 = (t1 + np.array([0.01, -0.02, 0.07], dtype=np.float32)).astype(np.float32)
    kw = dict(near=rc.NEAR, far=rc.FAR, want_face=True, want_homo=True)
    eager1 = render_depth(meshes, idx, _dev(R1), _dev(t1), K, size, **kw)
    eager2 = render_depth(meshes, idx, _dev(R2), _dev(t2), K, size, **kw)
    assert not torch.equal(eager1.depth, eager2.depth)
    R, t = _dev(R1), _dev(t1)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        render_depth(meshes, idx, R, t, K, size, **kw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = render_depth(meshes, idx, R, t, K, size, **kw)
    for want, (Rn, tn) in ((eager1, (R1, t1)), (eager2, (R2, t2))):
        R.copy_(_dev(Rn))
        t.copy_(_dev(tn))
        for x in cap:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(cap, want))


def _write_ply_ascii(path, v, f):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\ncomment written by the test\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"property uchar red\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for p in v:
            fh.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 200\n")
        for t in f:
            fh.write(f"3 {t[0]} {t[1]} {t[2]}\n")


def _write_ply_binary(path, v, f):
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                  f"property float nx\nproperty uchar red\nelement face {len(f)}\nproperty list uchar uint vertex_index\nproperty uchar flag\n"
                  f"end_header\n").encode())
        for p in v:
            fh.write(struct.pack("<ffffB", float(p[0]), float(p[1]), float(p[2]), 0.5, 7))
        for t in f:
            fh.write(struct.pack("<BIIIB", 3, int(t[0]), int(t[1]), int(t[2]), 1))


def test_gen_z_tool_writes_the_reference_records(tmp_path):
    """One scene, two images, two objects and one instance out of view, from PLYs written here (mm, as BOP models)."""
    from lc_amd import gen_z
    from lc_amd.render import decode_z_info

    models, data = tmp_path / "models", tmp_path / "train"
    (data / "000003").mkdir(parents=True)
    models.mkdir()
    objs = {2: rc.MESHES["ico"], 5: rc.MESHES["torus"]}
    mm = {k: ((v.astype(np.float64) * 1000).astype(np.float32), f) for k, (v, f) in objs.items()}
    _write_ply_ascii(models / "obj_000002.ply", *mm[2])
    _write_ply_binary(models / "obj_000005.ply", *mm[5])
    Kf = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], dtype=np.float32)
    inst = {"0": [(2, rc.POSES["ico"]), (5, rc.POSES["torus"])], "7": [(5, rc.POSES["torus257"]), (2, rc.OUT_OF_VIEW)]}
    gt = {im: [dict(obj_id=o, cam_R_m2c=p.R.astype(np.float64).reshape(-1).tolist(), cam_t_m2c=(p.t.astype(np.float64) * 1000).tolist()) for o, p in a]
          for im, a in inst.items()}
    (data / "000003" / "scene_gt.json").write_text(json.dumps(gt))
    (data / "000003" / "scene_camera.json").write_text(json.dumps({im: dict(cam_K=Kf.astype(np.float64).reshape(-1).tolist(), depth_scale=1.0) for im in inst}))
    assert gen_z.main(["--data_dir", str(data), "--model_dir", str(models)]) == 0
    size = (gen_z.IM_H, gen_z.IM_W)
    for im, annos in inst.items():
        for i, (o, pose) in enumerate(annos):
            with gzip.open(data / "z_crop" / "000003" / f"{int(im):06d}_{i:06d}.pkl.gz", "rb") as fh:
                z_info = pickle.load(fh)
            assert set(z_info) == {"z_crop", "xyxy", "z_max", "z_min"} and z_info["z_crop"].dtype == np.uint16
            if pose is rc.OUT_OF_VIEW:
                assert z_info["z_crop"].shape == size and not z_info["z_crop"].any() and list(z_info["xyxy"]) == [0, 0, size[1] - 1, size[0] - 1]
                assert np.asarray(z_info["z_max"]).reshape(-1)[0] == 0 and np.asarray(z_info["z_min"]).reshape(-1)[0] == 0
                continue
            # the tool's inputs: the PLY's mm scaled by fp32 0.001, t in mm divided by fp32 1000 (gen_z.py:105,142)
            v = mm[o][0] * np.float32(0.001)
            t = (np.asarray(gt[im][i]["cam_t_m2c"], dtype=np.float32) / np.float32(1000.0)).astype(np.float32)
            ref = ro.render(v, mm[o][1], pose.R, t, Kf, size, gen_z.NEAR, gen_z.FAR)
            assert ref.margin >= 2.0 ** -30
            depth, mask = decode_z_info(z_info, size)
            assert np.array_equal(mask, ref.mask)
            ys, xs = np.nonzero(ref.mask)
            assert list(z_info["xyxy"]) == [xs.min(), ys.min(), xs.max(), ys.max()]
            step = (float(z_info["z_max"]) - float(z_info["z_min"])) / 65534
            # half a quantisation step, the fp32 rendering and the fp32 arithmetic of the encode and decode (in mm)
            bound = 0.5 * step + 1000 * ref.z64.max() * (ro.z_tolerance(ref) + 8 * 2.0 ** -24)
            assert np.abs(depth.astype(np.float64) - 1000 * ref.z64)[ref.mask].max() <= bound
