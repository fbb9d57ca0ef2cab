"""GPU tests of the ground-truth annotations (lc_amd.gtinfo, lc_amd/csrc/gtinfo/lc_gtinfo.hip).  Every record, mask and composed map is
compared with the numpy fp64 oracle (tests/gtinfo_oracle.py) for EQUALITY: the outputs are integers and bytes.  The cases and the margin
condition that makes equality a fair demand (tests/gtinfo_cases.py) are shown on the CPU by tests/test_gtinfo_oracle.py."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import gtinfo_cases as C
from tests import gtinfo_oracle as oracle
from tests import render_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = C.names()


def _dev(a, rows=slice(None)):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a[rows])).to(DEV)


def _dirty(*shapes):
    """Blocks of the outputs' sizes filled with ones and given back to the allocator: an output the kernel forgot to write would show."""
    for shape, dtype in shapes:
        torch.full(shape, 1, device=DEV, dtype=dtype)


def _np(out):
    info = out.info.cpu().numpy()
    assert info.dtype == np.int32 and out.mask_visib.dtype == torch.bool
    return info, out.mask_visib.view(torch.uint8).cpu().numpy()  # the bytes themselves: 0 or 1


def _record(name, rows=slice(None), **kw):
    from lc_amd import gtinfo

    c = C.case(name)
    gt = _dev(c.depth_gt, rows)
    _dirty((tuple(gt.shape), torch.bool), ((gt.shape[0], 12), torch.int32))
    return gtinfo.gt_info_from_depth(gt, _dev(c.depth_test), _dev(c.K, rows), delta=c.delta, scene_index=_dev(c.scene_index, rows),
                                     origin_xy=_dev(c.origins, rows), pixel_center=c.center, **kw)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "info", got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1], want[1]), (what, "mask", np.argwhere(got[1] != want[1])[:8].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_record_equals_the_oracle(name):
    info, mask, _ = C.expected(name)
    got = _np(_record(name))
    _same(got, (info, mask), name)
    c = C.case(name)
    for b, s in enumerate(c.scene_index):  # a refused row: -1 throughout and a zero mask
        if oracle.refused(s, len(c.depth_test), None if c.origins is None else c.origins[b]):
            assert (got[0][b] == -1).all() and not got[1][b].any(), b


def test_threshold_pixel_and_values():
    """At the pixel where n = 1 a difference equal to delta is visible and one ulp above it is not; what counts as a hit and as a measurement."""
    info, mask = _np(_record("threshold-7x9"))
    assert mask[0, 3, 4] == 1 and mask[1, 3, 4] == 0 and info[:, 2].tolist() == [2, 0]
    info, mask = _np(_record("values-7x9"))
    assert info[0].tolist() == [0, 0, 0, 0] + [-1] * 8 and info[1].tolist() == [63, 60, 54, 28, 0, 0, 8, 6, 0, 0, 8, 6]
    assert mask[1, 1, 1:5].all() and not mask[2, 2, 2:5].any() and not mask[2, 3, 3]
    info, _ = _np(_record("edge-5x6"))
    assert info[:, 3].tolist() == [0, 1, 1, 1, 1, 4]
    assert _np(_record("corners-3x-7x9"))[0][0].tolist() == [6, 4, 4, 2, -9, -7, 17, 13, 0, 0, 8, 6]


def test_without_the_mask_and_visib_fract():
    from lc_amd import gtinfo

    out = _record("full-16x20", want_mask=False)
    assert out.mask_visib is None
    info = C.expected("full-16x20")[0]
    assert np.array_equal(out.info.cpu().numpy(), info)
    fract = out.visib_fract()
    assert fract.dtype == torch.float64 and fract.is_cuda
    ratio = info[:, 2].astype(np.float64) / info[:, 0].astype(np.float64)
    assert (np.abs(fract.cpu().numpy() - ratio) <= 2.0 ** -52 * ratio).all()  # one fp64 division on either side
    out = _record("full-33x37")  # an empty render and two refused rows: 0
    assert out.visib_fract().cpu().numpy()[[0, 2, 4]].tolist() == [0.0, 0.0, 0.0]
    assert [r["visib_fract"] for r in gtinfo.bop_records(out)] == pytest.approx(out.visib_fract().cpu().tolist(), rel=2.0 ** -52, abs=0.0)


def test_same_bits_under_permutation_split_and_allocation_phase():
    from lc_amd import gtinfo

    for name in ("full-16x20", "win-5x8", "win-5x9", "larger-20x25", "full-33x37", "tiles"):
        c = C.case(name)
        B = len(c.depth_gt)
        want = C.expected(name)[:2]
        perm = list(np.random.default_rng(B).permutation(B))
        got = _np(_record(name, perm))
        _same(got, (want[0][perm], want[1][perm]), (name, "permuted"))
        head, tail = _np(_record(name, slice(0, 1))), _np(_record(name, slice(1, None)))
        _same((np.concatenate((head[0], tail[0])), np.concatenate((head[1], tail[1]))), want, (name, "1 + (B - 1)"))
        # the same maps one, two and three elements further into their allocations: every 16-byte phase of both maps

        def shifted(a, k):
            t = _dev(a)
            buf = torch.empty(t.numel() + k, dtype=t.dtype, device=DEV)
            buf[k:].copy_(t.reshape(-1))
            return buf[k:].view(t.shape)

        for kg, kt in ((1, 0), (2, 3), (3, 2), (0, 1)):
            out = gtinfo.gt_info_from_depth(shifted(c.depth_gt, kg), shifted(c.depth_test, kt), _dev(c.K), delta=c.delta, scene_index=_dev(c.scene_index),
                                            origin_xy=_dev(c.origins), pixel_center=c.center)
            _same(_np(out), want, (name, "shifted", kg, kt))


def test_refused_rows_leave_their_neighbours_untouched():
    from lc_amd import gtinfo

    name = "win-5x9"
    c = C.case(name)
    want = C.expected(name)[:2]
    scene = c.scene_index.copy()
    scene[1], scene[4] = -1, len(c.depth_test)  # below and one past the scenes
    # a refused row's maps are never read: NaN all over would count nothing either, so give it hits that WOULD count
    gt = c.depth_gt.copy()
    gt[1] = gt[4] = 1.0
    _dirty((tuple(gt.shape), torch.bool), ((len(gt), 12), torch.int32))
    out = gtinfo.gt_info_from_depth(_dev(gt), _dev(c.depth_test), _dev(c.K), delta=c.delta, scene_index=_dev(scene), origin_xy=_dev(c.origins), pixel_center=c.center)
    info, mask = _np(out)
    for b in (1, 4):
        assert (info[b] == -1).all() and not mask[b].any(), b
    ok = [0, 2, 3, 5]
    _same((info[ok], mask[ok]), (want[0][ok], want[1][ok]), "the other rows")


def test_cross_check_against_the_vsd_kernel():
    """The shipped VSD kernel with depth_est = depth_gt counts the visible ground-truth pixels twice over: union = inter = px_count_visib."""
    from lc_amd import vsd

    for name in ("full-7x9", "full-16x20", "values-7x9", "threshold-7x9", "corners-7x9"):
        c = C.case(name)
        assert c.origins is None and ((0 <= c.scene_index) & (c.scene_index < len(c.depth_test))).all()
        info, _ = _np(_record(name))
        gt = _dev(c.depth_gt)
        out = vsd.vsd_from_depth(gt, gt, _dev(c.depth_test), _dev(c.K), delta=c.delta, taus=(0.1,), scene_index=_dev(c.scene_index), pixel_center=c.center)
        counts = out.counts.cpu().numpy()
        assert np.array_equal(counts[:, 0], info[:, 2]) and np.array_equal(counts[:, 1], info[:, 2]), name


def _compose(name, rows=slice(None), **kw):
    from lc_amd import gtinfo

    c = C.case(name)
    S, (H, W) = len(c.depth_test), c.frame_hw
    _dirty(((S, H, W), torch.float32), ((S, H, W), torch.int32))
    return gtinfo.compose_scene_depth(_dev(c.depth_gt, rows), _dev(c.scene_index, rows), c.frame_hw, S, origin_xy=_dev(c.origins, rows), **kw)


def _same_scene(out, want, what):
    depth = out.depth.cpu().numpy()
    assert depth.dtype == np.float32 and np.array_equal(depth.view(np.int32), want.depth.view(np.int32)), (what, "depth")
    if out.instance is not None:
        assert out.instance.dtype == torch.int32 and np.array_equal(out.instance.cpu().numpy(), want.instance), (what, "instance")
    assert np.array_equal(out.info.cpu().numpy(), want.info), (what, "info")


@pytest.mark.parametrize("name", NAMES)
def test_composition_equals_the_oracle(name):
    """Ties go to the lowest row (the maps lie on a 1/16 grid), 0, negative, NaN and inf values are no hits, windows overlap and reach
    outside the frame, rows are skipped."""
    _same_scene(_compose(name, want_instance=True), C.expected_compose(name), name)
    assert _compose(name).instance is None


def test_composition_ties_and_order():
    from lc_amd import gtinfo

    inst = np.array([[[1, 0, 2], [0, 0, np.nan]], [[1, 3, 1], [np.inf, -1, 0]], [[0.5, 0, 1], [0, 0, 0]]], dtype=np.float32)
    out = gtinfo.compose_scene_depth(_dev(inst), torch.zeros(3, dtype=torch.int64, device=DEV), (2, 3), 1, want_instance=True)
    assert out.depth.cpu().tolist() == [[[0.5, 3, 1], [0, 0, 0]]] and out.instance.cpu().tolist() == [[[2, 1, 1], [-1, -1, -1]]]
    for name in ("full-16x20", "win-5x8", "larger-20x25"):
        c = C.case(name)
        B = len(c.depth_gt)
        want = C.expected_compose(name)
        perm = list(np.random.default_rng(B + 1).permutation(B))
        out = _compose(name, perm, want_instance=True)
        assert np.array_equal(out.depth.cpu().numpy().view(np.int32), want.depth.view(np.int32)), name  # the depth knows no order
        again = oracle.compose(c.depth_gt[perm], c.scene_index[perm], c.frame_hw, len(c.depth_test), None if c.origins is None else c.origins[perm])
        _same_scene(out, again, (name, "permuted"))  # the instance map names the lowest of the rows as they are numbered now


def _graph(call):
    """call() eagerly, then captured and replayed twice: the three results."""
    eager = call()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a host synchronisation or a read-back in here would fail the capture
        assert torch.cuda.is_current_stream_capturing()
        out = call()
    return eager, g, out


def test_graph_replay():
    from lc_amd import gtinfo

    name = "win-5x9"
    c = C.case(name)
    t = dict(gt=_dev(c.depth_gt), test=_dev(c.depth_test), K=_dev(c.K), scene=_dev(c.scene_index), org=_dev(c.origins))

    def call():
        rec = gtinfo.gt_info_from_depth(t["gt"], t["test"], t["K"], delta=c.delta, scene_index=t["scene"], origin_xy=t["org"], pixel_center=c.center)
        return rec, gtinfo.compose_scene_depth(t["gt"], t["scene"], c.frame_hw, len(c.depth_test), origin_xy=t["org"], want_instance=True)

    (rec, scene), g, (rec_g, scene_g) = _graph(call)
    want = C.expected(name)[:2]
    _same(_np(rec), want, "eager")
    B = len(c.depth_gt)
    perm = [3, 0, 5, 1, 4, 2]  # other rows written into the same tensors
    for k, a in (("gt", c.depth_gt), ("K", c.K), ("scene", c.scene_index), ("org", c.origins)):
        t[k].copy_(_dev(a)[perm])
    assert len(perm) == B
    again = oracle.compose(c.depth_gt[perm], c.scene_index[perm], c.frame_hw, len(c.depth_test), c.origins[perm])
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _same(_np(rec_g), (want[0][perm], want[1][perm]), "replay")
        _same_scene(scene_g, again, "replay")
    _same(_np(call()[0]), (want[0][perm], want[1][perm]), "eager after the copy")


def test_empty_batch():
    from lc_amd import gtinfo

    c = C.case("full-7x9")
    out = gtinfo.gt_info_from_depth(_dev(c.depth_gt)[:0], _dev(c.depth_test), _dev(c.K)[:0], delta=c.delta, scene_index=_dev(c.scene_index)[:0])
    assert out.info.shape == (0, 12) and out.info.dtype == torch.int32 and out.mask_visib.shape == (0, 7, 9)
    out = _compose("full-7x9", slice(0, 0), want_instance=True)
    assert out.info.shape == (0,) and not out.depth.any() and (out.instance == -1).all() and out.depth.shape == (2, 7, 9)


@functools.lru_cache(maxsize=None)
def _meshes():
    from lc_amd import render

    return render.MeshSet([rc.MESHES[m] for m in ("ico", "torus", "box")], DEV)


def _whole_camera(size_hw):
    """fx != fy, skew, and an integer-valued principal point: shifting it by a window origin is exact in fp32."""
    H, W = size_hw
    f = 1.25 * max(H, W)
    return np.array([[f, 0.03 * f, W // 2], [0, 0.97 * f, H // 2], [0, 0, 1]], dtype=np.float32)


def _scene_of_three(idx=(0, 1, 2)):
    """The icosphere (z = 0.41) in front of the torus (0.47) in front of the box (0.9) of tests/render_cases.py, all near the optical axis."""
    poses = [rc.POSES[m] for m in ("ico", "torus", "box")]
    return dict(mesh_index=torch.tensor(idx, dtype=torch.int32, device=DEV), R=_dev(np.stack([p.R for p in poses])), t=_dev(np.stack([p.t for p in poses])))


def test_rendered_instances_of_a_composed_scene():
    from lc_amd import gtinfo

    size = (64, 64)
    K = _dev(_whole_camera(size))
    p = _scene_of_three()
    out = gtinfo.compute_gt_info(_meshes(), p["mesh_index"], p["R"], p["t"], K, None, frame_hw=size, delta=0.0, near=rc.NEAR, far=rc.FAR)
    info, mask = _np(out)
    d = out.depth_gt.cpu().numpy()
    hit = d > 0
    assert out.render_info.cpu().tolist() == [0, 0, 0] and out.origin_xy.cpu().tolist() == [[0, 0]] * 3 and d.shape == (3, 64, 64)
    assert (hit[0] & hit[1]).sum() > 50 and (hit[1] & hit[2]).sum() > 50  # they do overlap
    # delta = 0: an instance is visible exactly where it is the nearest, so where depths differ the visible sets are disjoint, and
    # together they cover the union of the silhouettes
    vis = mask.astype(bool)
    assert np.array_equal(vis.any(0), hit.any(0))
    stacked = np.where(hit, d, np.inf)
    differ = (np.sort(stacked, 0)[1] != np.sort(stacked, 0)[0])
    assert not (vis.sum(0) > 1)[differ].any()
    assert (info[:, 2] <= info[:, 0]).all() and (info[1:, 2] < info[1:, 0]).all()  # the torus and the box are partly hidden
    # the oracle on the same renders
    want_scene = oracle.compose(d, np.zeros(3, np.int32), size, 1)
    _same_scene(out.scene, want_scene, "scene")
    want = oracle.records(d, want_scene.depth, _whole_camera(size), 0.0, np.zeros(3, np.int32))
    _same((info, mask), want[:2], "records")
    assert np.array_equal(out.scene.instance.cpu().numpy()[0] >= 0, hit.any(0))


def test_rendered_instances_against_a_measured_depth_windows_and_an_unknown_mesh():
    from lc_amd import gtinfo

    size = (48, 64)
    H, W = size
    Kn = _whole_camera(size)
    K = _dev(Kn)
    p = _scene_of_three(idx=(0, 7, 2))  # the second row names no mesh of the set
    rng = np.random.default_rng(5)
    test = rng.uniform(0.35, 1.0, size=(1, H, W)).astype(np.float32)
    test[0, 10:20, 10:30] = 0
    kw = dict(delta=0.015, near=rc.NEAR, far=rc.FAR)
    full = gtinfo.compute_gt_info(_meshes(), p["mesh_index"], p["R"], p["t"], K, _dev(test), **kw)
    info, mask = _np(full)
    assert full.scene is None and full.render_info.cpu().tolist() == [0, -1, 0]
    assert (info[1] == -1).all() and not mask[1].any()
    d = full.depth_gt.cpu().numpy()
    want = oracle.records(d[[0, 2]], test, Kn, 0.015, np.zeros(2, np.int32))
    assert want[2] >= C.MARGIN
    _same((info[[0, 2]], mask[[0, 2]]), want[:2], "full frame")
    # BOP's 3H x 3W form: the whole principal point makes the frame's part of the wide render the frame's render, so what is visible
    # and where does not change, and the silhouette can only grow
    wide = gtinfo.compute_gt_info(_meshes(), p["mesh_index"], p["R"], p["t"], K, _dev(test), margin=(W, H), **kw)
    wi, wm = _np(wide)
    assert wide.depth_gt.shape == (3, 3 * H, 3 * W) and wide.origin_xy.cpu().tolist() == [[-W, -H]] * 3
    assert torch.equal(wide.depth_gt[:, H:2 * H, W:2 * W], full.depth_gt)
    assert np.array_equal(wi[:, [1, 2, 8, 9, 10, 11]], info[:, [1, 2, 8, 9, 10, 11]]) and np.array_equal(wm[:, H:2 * H, W:2 * W], mask)
    assert (wi[[0, 2], 0] >= info[[0, 2], 0]).all() and not wi[[0, 2], 3].any()
    want = oracle.records(wide.depth_gt.cpu().numpy()[[0, 2]], test, Kn, 0.015, np.zeros(2, np.int32), np.asarray([[-W, -H]] * 2))
    _same((wi[[0, 2]], wm[[0, 2]]), want[:2], "3H x 3W")
    # a window per row, one of them cutting its object: edge says so
    org = torch.tensor([[20, 10], [0, 0], [W // 2, -3]], dtype=torch.int32, device=DEV)
    win = gtinfo.compute_gt_info(_meshes(), p["mesh_index"], p["R"], p["t"], K, _dev(test), window_hw=(30, 28), window_xy=org, **kw)
    gi, gm = _np(win)
    want = oracle.records(win.depth_gt.cpu().numpy()[[0, 2]], test, Kn, 0.015, np.zeros(2, np.int32), org.cpu().numpy()[[0, 2]])
    _same((gi[[0, 2]], gm[[0, 2]]), want[:2], "windows")
    assert gi[2, 3] > 0 and gi[2, 0] < info[2, 0]


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for v in verts:
            f.write(" ".join(repr(float(x)) for x in v) + "\n")
        for t in faces:
            f.write("3 " + " ".join(str(int(i)) for i in t) + "\n")


def test_command_line_tool(tmp_path):
    """A two-image scene: the JSON written is `bop_records` of the direct call, the masks are the direct call's, with the depth composed
    and with one read from --depth-dir."""
    from lc_amd import gen_gt_info, gen_z, gtinfo

    H, W = 40, 48
    Kn = _whole_camera((H, W))
    models, scene = tmp_path / "models", tmp_path / "000001"
    models.mkdir()
    scene.mkdir()
    for obj_id, m in ((1, "ico"), (4, "torus")):
        v, f = rc.MESHES[m]
        _write_ply(models / f"obj_{obj_id:06d}.ply", v.astype(np.float64) * 1000.0, f)  # mm

    def anno(obj_id, m, dt=(0, 0, 0)):
        p = rc.POSES[m]
        return dict(obj_id=obj_id, cam_R_m2c=[float(x) for x in p.R.reshape(-1)], cam_t_m2c=[float(x) * 1000.0 for x in (p.t + np.asarray(dt, np.float32))])

    gt = {"0": [anno(1, "ico"), anno(4, "torus")], "3": [anno(4, "torus", (0.02, 0, 0)), anno(9, "ico"), anno(1, "ico", (-0.03, 0.01, 0.1))]}
    cam = {k: dict(cam_K=[float(x) for x in Kn.reshape(-1)], depth_scale=1.0) for k in gt}
    (scene / "scene_gt.json").write_text(json.dumps(gt))
    (scene / "scene_camera.json").write_text(json.dumps(cam))
    depth_dir = tmp_path / "depth"
    depth_dir.mkdir()
    rng = np.random.default_rng(9)
    measured = {k: rng.uniform(380, 520, size=(H, W)).astype(np.float32) for k in gt}  # mm
    for k, d in measured.items():
        np.save(depth_dir / f"{int(k):06d}.npy", d)
    meshes = gen_z.load_models(str(models), DEV)
    for args, depth_of, margin, out_dir in (
            (["--frame-hw", str(H), str(W), "--margin", "8", "6"], None, (8, 6), scene),
            (["--depth-dir", str(depth_dir), "--delta", "10", "--bbox-plus-one", "--out-dir", str(tmp_path / "out")], measured, (W, H), tmp_path / "out")):
        assert gen_gt_info.main([str(scene), str(models), *args]) == 0
        written = json.loads((out_dir / "scene_gt_info.json").read_text())
        assert list(written) == list(gt)
        for k, annos in gt.items():
            R = _dev(np.stack([np.asarray(a["cam_R_m2c"], np.float32).reshape(3, 3) for a in annos]))
            t = _dev(np.stack([np.asarray(a["cam_t_m2c"], np.float32) / np.float32(1000.0) for a in annos]))
            test = None if depth_of is None else _dev((depth_of[k] * np.float32(0.001))[None])
            direct = gtinfo.compute_gt_info(meshes, meshes.index_of([a["obj_id"] for a in annos]), R, t, _dev(Kn), test, frame_hw=(H, W), margin=margin,
                                            delta=0.015 if depth_of is None else 0.010, near=gen_z.NEAR, far=gen_z.FAR)
            want = gtinfo.bop_records(direct, bbox_plus_one=depth_of is not None)
            assert written[k] == want, k
            assert len(want) == len(annos) and all(r["px_count_all"] > 0 for r, a in zip(want, annos) if a["obj_id"] != 9)
            z = np.load(out_dir / "mask_npz" / f"{int(k):06d}.npz")
            mx, my = margin
            assert z["mask"].shape == z["mask_visib"].shape == (len(annos), H, W) and z["mask"].dtype == z["mask_visib"].dtype == np.bool_
            assert np.array_equal(z["mask"], (direct.depth_gt[:, my:my + H, mx:mx + W] > 0).cpu().numpy())
            assert np.array_equal(z["mask_visib"], direct.mask_visib[:, my:my + H, mx:mx + W].cpu().numpy())
            assert [int(m.sum()) for m in z["mask_visib"]] == [max(r["px_count_visib"], 0) for r in want]
        assert written["3"][1] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=-1, px_count_valid=-1, px_count_visib=-1, visib_fract=0.0)  # no model 9
