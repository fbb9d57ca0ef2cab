"""`python -m lc_amd.gen_scenes` on the device: 2 scenes of 2 objects into a temporary directory, from two procedural models written as PLY
files.  The two JSON files parse in BOP's layout, their poses are `posedraw.draw_scene_poses_host`'s for the same seed, and
`python -m lc_amd.gen_gt_info` accepts the directory."""
import json
import os

import numpy as np
import pytest
import torch

from tests import render_cases

pytestmark = pytest.mark.gpu
FRAME = (48, 64)
SEED = 2 ** 33 + 5
OBJ_IDS = (2, 9)


def _write_ply(path, verts_mm, faces):
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts_mm)}\nproperty float x\nproperty float y\nproperty float z\n"
                f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for v in verts_mm:
            f.write(" ".join(repr(float(x)) for x in v) + "\n")
        for tri in faces:
            f.write("3 " + " ".join(str(int(i)) for i in tri) + "\n")


def test_the_tool_writes_bop_s_two_files_from_the_host_contract_s_poses(tmp_path, capsys):
    from lc_amd import gen_gt_info, gen_scenes, gen_z, posedraw

    models, out = tmp_path / "models", tmp_path / "scene"
    models.mkdir()
    meshes = [render_cases.box((0.08, 0.06, 0.05)), render_cases.icosphere(0, 0.1)]
    for obj_id, (v, f) in zip(OBJ_IDS, meshes):
        _write_ply(models / f"obj_{obj_id:06d}.ply", v.astype(np.float64) * 1000.0, f)
    K = render_cases.camera(FRAME)
    argv = [str(models), str(out), "--scenes", "2", "--objects", "2", "--seed", str(SEED), "--first-id", "4", "--frame-hw", "48", "64", "--z-range", "0.6", "0.9",
            "--centre-box", "8", "8", "56", "40", "--gap", "0.005", "--cam-K", *[repr(float(v)) for v in K.reshape(-1)]]
    assert gen_scenes.main(argv) == 0
    assert "wrote 4 instances of 2 images" in capsys.readouterr().out

    with open(out / "scene_gt.json") as f:
        gt = json.load(f)
    with open(out / "scene_camera.json") as f:
        cam = json.load(f)
    assert sorted(gt) == sorted(cam) == ["4", "5"]
    # the host contract on what the tool read: the models as gen_z loads them (mm to metres in float32), their radii, the round-robin slots
    loaded = [(gen_z.read_ply(str(models / f"obj_{i:06d}.ply"))[0] * np.float32(0.001), f) for i, (_, f) in zip(OBJ_IDS, meshes)]
    radius = posedraw.mesh_radii(loaded)
    slots = gen_scenes.slot_models(2, 4, 2, 2)
    assert slots.tolist() == [[0, 1], [0, 1]]
    cfg = posedraw.PoseDrawConfig(z_range=(0.6, 0.9), centre_box=(8.0, 8.0, 56.0, 40.0), gap=0.005, near=gen_z.NEAR)
    host = posedraw.draw_scene_poses_host(cfg, SEED, np.array([4, 5], np.int32), slots, radius, K)
    assert not host.info.any()
    for s, im in enumerate(("4", "5")):
        assert set(cam[im]) == {"cam_K", "depth_scale"} and cam[im]["depth_scale"] == 1.0
        assert np.array_equal(np.asarray(cam[im]["cam_K"], dtype=np.float32).reshape(3, 3), K) and len(cam[im]["cam_K"]) == 9
        assert len(gt[im]) == 2
        for m, anno in enumerate(gt[im]):
            assert set(anno) == {"cam_R_m2c", "cam_t_m2c", "obj_id"} and len(anno["cam_R_m2c"]) == 9 and len(anno["cam_t_m2c"]) == 3
            assert anno["obj_id"] == OBJ_IDS[slots[s, m]]
            assert np.array_equal(np.asarray(anno["cam_R_m2c"], dtype=np.float64).astype(np.float32).view(np.int32), host.R[s, m].reshape(-1).view(np.int32))
            t_m = (np.asarray(anno["cam_t_m2c"], dtype=np.float64) / 1000.0).astype(np.float32)  # mm in the file
            assert np.array_equal(t_m.view(np.int32), host.t[s, m].view(np.int32))
        rgb, depth = np.load(out / "rgb" / f"{int(im):06d}.npy"), np.load(out / "depth" / f"{int(im):06d}.npy")
        assert rgb.shape == (*FRAME, 3) and rgb.dtype == np.uint8 and depth.shape == FRAME and depth.dtype == np.float32
        hit = depth > 0
        assert hit.any() and rgb[hit].any() and not rgb[~hit].any() and depth[hit].min() >= 400.0 and depth[hit].max() <= 1100.0  # mm

    # the annotation tool accepts the directory, with the composed depth and with the written one
    for extra in ([], ["--depth-dir", str(out / "depth")]):
        assert gen_gt_info.main([str(out), str(models), "--margin", "0", "0", "--frame-hw", "48", "64", "--out-dir", str(tmp_path / "info")] + extra) == 0
        with open(tmp_path / "info" / "scene_gt_info.json") as f:
            records = json.load(f)
        assert sorted(records) == ["4", "5"] and all(len(records[im]) == 2 for im in records)
        assert all(r["px_count_all"] > 0 and 0.0 < r["visib_fract"] <= 1.0 for im in records for r in records[im])
    torch.cuda.synchronize()
