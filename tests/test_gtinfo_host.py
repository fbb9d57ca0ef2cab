"""The ground-truth annotations without a GPU: the library of its own (liblc_amd_gtinfo.so: header, exports, signatures and source hash
agree; its place among the libraries: tests/test_libraries_host.py), every refusal of the wrappers (lc_amd.gtinfo) on CPU tensors, the
argument checks of the two C entry points before any launch, the kernels' resources read from the code object, and `bop_records`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_group_and_order():
    import __graft_entry__ as entry
    from lc_amd import build

    entry.build()  # (the registry and the build order: tests/test_libraries_host.py) leaves this library in place and current
    assert os.path.exists(build.GTINFO.so_path) and not build.is_stale(build.GTINFO)


def test_library_header_exports_and_signatures_agree():
    from lc_amd import build, gtinfo

    lib = gtinfo.load()
    header = open(os.path.join(ROOT, "include", "lc_amd_gtinfo.h")).read()
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(gtinfo._SIGNATURES) and {"lc_gtinfo_f32", "lc_scene_compose_f32", "lc_scene_compose_workspace_bytes"} <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", build.GTINFO.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_gtinfo_version() == int(re.search(r"#define LC_AMD_GTINFO_VERSION (\d+)", header).group(1)) == 1
    for name, have in (("COLUMNS", gtinfo.COLUMNS), ("MAX_FRAME", gtinfo.MAX_FRAME), ("MAX_WINDOW", gtinfo.MAX_WINDOW), ("MAX_ORIGIN", gtinfo.MAX_ORIGIN),
                       ("TILE_W", gtinfo.TILE_W), ("TILE_H", gtinfo.TILE_H)):
        assert have == int(re.search(rf"#define LC_GTINFO_{name} (\d+)", header).group(1)), name
    # every prototype's argument list against the ctypes signature: pointers, ints, floats and sizes in the same places
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_size_t: "s"}
    for name in ("lc_gtinfo_f32", "lc_scene_compose_f32", "lc_scene_compose_workspace_bytes"):
        m = re.search(rf"(int|size_t) {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else a.split()[0][0] for a in m.group(2).split(",")]
        res, args = gtinfo._SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)], name
        assert kinds == [kinds_of[a] for a in args], (name, kinds)
    assert lib.lc_scene_compose_workspace_bytes(3, 7, 9) == 3 * 7 * 9 * 8 and lib.lc_scene_compose_workspace_bytes(0, 7, 9) == 0


def test_source_hash_is_its_own():
    from lc_amd import build, gtinfo

    lib = gtinfo.load()
    T = build.GTINFO
    assert not build.is_stale(T)
    assert lib.lc_amd_gtinfo_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert build.sources(T) == [os.path.join(build.CSRC, "gtinfo", "lc_gtinfo.hip")]


def _good(B=3, h=4, w=5):
    return dict(depth_gt=torch.zeros(B, h, w), depth_test=torch.zeros(h, w), K=torch.eye(3), delta=15.0)


def test_wrapper_refusals_of_the_record():
    from lc_amd import gtinfo

    f = gtinfo.gt_info_from_depth
    with pytest.raises(TypeError, match="depth_gt must be a torch.Tensor"):
        f(**dict(_good(), depth_gt=np.zeros((3, 4, 5), np.float32)))
    with pytest.raises(TypeError, match="depth_gt must be float32"):
        f(**dict(_good(), depth_gt=torch.zeros(3, 4, 5, dtype=torch.float64)))
    with pytest.raises(TypeError, match="depth_test must be float32"):
        f(**dict(_good(), depth_test=torch.zeros(4, 5, dtype=torch.float16)))
    with pytest.raises(TypeError, match="K must be float32"):
        f(**dict(_good(), K=torch.eye(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"depth_gt has shape \(4, 5\)"):
        f(**dict(_good(), depth_gt=torch.zeros(4, 5)))
    with pytest.raises(ValueError, match=r"depth_test has shape \(1, 2, 4, 5\)"):
        f(**dict(_good(), depth_test=torch.zeros(1, 2, 4, 5)))
    with pytest.raises(ValueError, match=r"K has shape \(2, 3, 3\)"):
        f(**dict(_good(), K=torch.zeros(2, 3, 3)))
    with pytest.raises(ValueError, match="must have the frame's size"):
        f(**dict(_good(), depth_test=torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="scene_index is needed"):
        f(**dict(_good(), depth_test=torch.zeros(2, 4, 5)))
    with pytest.raises(TypeError, match="scene_index must be int32 or int64"):
        f(**dict(_good(), scene_index=torch.zeros(3)))
    with pytest.raises(ValueError, match=r"scene_index has shape \(2,\)"):
        f(**dict(_good(), scene_index=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(TypeError, match="origin_xy must be a torch.Tensor"):
        f(**dict(_good(), origin_xy=[(0, 0)] * 3))
    with pytest.raises(TypeError, match="origin_xy must be int32 or int64"):
        f(**dict(_good(), origin_xy=torch.zeros(3, 2)))
    with pytest.raises(ValueError, match=r"origin_xy has shape \(3,\)"):
        f(**dict(_good(), origin_xy=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="the frame of 1 to 16384"):
        f(**dict(_good(), depth_test=torch.zeros(1, 16385), origin_xy=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="the window of 1 to 49152"):
        f(**dict(_good(), depth_gt=torch.zeros(3, 0, 5), origin_xy=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(TypeError, match="delta must be a number"):
        f(**dict(_good(), delta=torch.tensor(15.0)))
    with pytest.raises(ValueError, match="delta must be finite and not negative"):
        f(**dict(_good(), delta=-1.0))
    with pytest.raises(ValueError, match="delta must be finite and not negative"):
        f(**dict(_good(), delta=float("nan")))
    with pytest.raises(ValueError, match="pixel_center"):
        f(**dict(_good(), pixel_center=0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order: the maps are not on the HIP device
        f(**_good())
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a window larger than the frame, at a negative origin, is in order
        f(**dict(_good(), depth_gt=torch.zeros(3, 12, 15), scene_index=torch.zeros(3, dtype=torch.int32), origin_xy=torch.full((3, 2), -4, dtype=torch.int64)))


def test_wrapper_refusals_of_the_composition():
    from lc_amd import gtinfo

    f = gtinfo.compose_scene_depth
    good = dict(depth_inst=torch.zeros(3, 4, 5), scene_index=torch.zeros(3, dtype=torch.int32), frame_hw=(4, 5), n_scenes=1)
    with pytest.raises(TypeError, match="depth_inst must be float32"):
        f(**dict(good, depth_inst=torch.zeros(3, 4, 5, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"depth_inst has shape \(4, 5\)"):
        f(**dict(good, depth_inst=torch.zeros(4, 5)))
    with pytest.raises(TypeError, match="scene_index must be a torch.Tensor"):
        f(**dict(good, scene_index=None))
    with pytest.raises(ValueError, match=r"scene_index has shape \(1,\)"):
        f(**dict(good, scene_index=torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(ValueError, match="frame_hw is a pair"):
        f(**dict(good, frame_hw=4))
    with pytest.raises(TypeError, match="frame_hw holds two whole numbers"):
        f(**dict(good, frame_hw=(4.0, 5)))
    with pytest.raises(ValueError, match="frame_hw of 1 to 16384"):
        f(**dict(good, frame_hw=(0, 5)))
    with pytest.raises(TypeError, match="n_scenes must be a whole number"):
        f(**dict(good, n_scenes=1.0))
    with pytest.raises(ValueError, match="at least one scene"):
        f(**dict(good, n_scenes=0))
    with pytest.raises(ValueError, match="must have the frame's size"):
        f(**dict(good, frame_hw=(8, 8)))
    with pytest.raises(ValueError, match=r"origin_xy has shape \(2, 2\)"):
        f(**dict(good, origin_xy=torch.zeros(2, 2, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**dict(good, frame_hw=(2, 2), origin_xy=torch.zeros(3, 2, dtype=torch.int32), want_instance=True))


def _stand_in(device="cuda:0"):
    """A MeshSet without a device behind it (its constructor refuses the CPU): what the wrapper looks at before it renders."""
    from lc_amd import render

    m = object.__new__(render.MeshSet)
    m.device, m.n_meshes = torch.device(device), 3
    return m


def _good_poses(B=3):
    return dict(meshes=_stand_in(), mesh_index=torch.zeros(B, dtype=torch.int32), R=torch.zeros(B, 3, 3), t=torch.zeros(B, 3, 1), K=torch.eye(3),
                depth_test=torch.zeros(4, 5), delta=15.0, near=0.01, far=6.5)


def test_wrapper_refusals_of_the_chain():
    from lc_amd import gtinfo

    f = gtinfo.compute_gt_info
    with pytest.raises(TypeError, match="MeshSet"):
        f(**dict(_good_poses(), meshes=[(None, None)]))
    with pytest.raises(TypeError, match="mesh_index must be an int32 tensor"):
        f(**dict(_good_poses(), mesh_index=torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"mesh_index has shape \(3, 1\)"):
        f(**dict(_good_poses(), mesh_index=torch.zeros(3, 1, dtype=torch.int32)))
    with pytest.raises(TypeError, match="R must be float32"):
        f(**dict(_good_poses(), R=torch.zeros(3, 3, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"t has shape \(3, 1, 3\)"):
        f(**dict(_good_poses(), t=torch.zeros(3, 1, 3)))
    with pytest.raises(TypeError, match="t must be a torch.Tensor"):
        f(**dict(_good_poses(), t=np.zeros((3, 3), np.float32)))
    with pytest.raises(ValueError, match="frame_hw = .* is needed"):
        f(**dict(_good_poses(), depth_test=None))
    with pytest.raises(ValueError, match="n_scenes says how many"):
        f(**dict(_good_poses(), depth_test=None, frame_hw=(4, 5), scene_index=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="scene_index is needed"):
        f(**dict(_good_poses(), depth_test=None, frame_hw=(4, 5), n_scenes=2))
    with pytest.raises(ValueError, match="but depth_test is 4 x 5"):
        f(**dict(_good_poses(), frame_hw=(5, 4)))
    with pytest.raises(ValueError, match="but depth_test holds 1 scenes"):
        f(**dict(_good_poses(), n_scenes=2))
    with pytest.raises(ValueError, match="go together"):
        f(**dict(_good_poses(), window_hw=(2, 2)))
    with pytest.raises(ValueError, match="not both"):
        f(**dict(_good_poses(), margin=(1, 1), window_hw=(2, 2), window_xy=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="margin"):
        f(**dict(_good_poses(), margin=(-1, 0)))
    with pytest.raises(ValueError, match="margin"):
        f(**dict(_good_poses(), margin=3))
    with pytest.raises(ValueError, match="the window of 1 to 49152"):
        f(**dict(_good_poses(), margin=(30000, 0)))
    with pytest.raises(ValueError, match="delta must be finite"):
        f(**dict(_good_poses(), delta=float("inf")))
    with pytest.raises(RuntimeError, match="mesh_index is on cpu, the meshes are on cuda:0"):
        f(**_good_poses())
    with pytest.raises(RuntimeError, match="mesh_index is on cpu, the meshes are on cuda:0"):
        f(**dict(_good_poses(), depth_test=None, frame_hw=(4, 5), margin=(5, 4)))


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import gtinfo

    lib = gtinfo.load()
    buf = ctypes.create_string_buffer(2048)
    p = (ctypes.addressof(buf) + 15) & ~15

    def info(gt=p, org=None, test=p, scene=p, K=p, B=4, h=48, w=64, S=2, H=48, W=64, out=p, mask=p):
        return lib.lc_gtinfo_f32(gt, org, test, scene, K, B, h, w, S, H, W, 0.0, 0.0, 15.0, out, mask, None)

    msg = lib.lc_amd_gtinfo_last_error
    assert info(B=-1) != 0 and b"lc_gtinfo_f32: a negative size" in msg()
    assert info(w=-1) != 0 and b"negative" in msg()
    assert info(S=0) != 0 and b"at least one scene" in msg()
    assert info(H=16385, h=16385) != 0 and b"16384" in msg()
    assert info(h=0, org=p) != 0 and b"49152" in msg()
    assert info(h=49153, org=p) != 0 and b"49152" in msg()
    assert info(h=49152, w=49152, org=p) != 0 and b"2^31 pixels" in msg()
    assert info(h=40) != 0 and b"without origin_xy" in msg()
    assert info(gt=None) != 0 and b"null" in msg()
    assert info(scene=None) != 0 and b"null" in msg()
    assert info(out=None) != 0 and b"null" in msg()
    assert info(gt=p + 2) != 0 and b"4-byte" in msg()
    assert info(org=p + 1, h=40) != 0 and b"4-byte" in msg()
    assert info(B=1 << 30, h=16384, H=16384) != 0 and b"2^31 tiles" in msg()
    assert lib.lc_gtinfo_f32(None, None, None, None, None, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, None, None, None) == 0  # an empty batch is a no-op

    def compose(inst=p, org=None, scene=p, B=4, h=48, w=64, S=2, H=48, W=64, depth=p, instance=p, out=p, ws=p, nbytes=2 * 48 * 64 * 8):
        return lib.lc_scene_compose_f32(inst, org, scene, B, h, w, S, H, W, depth, instance, out, ws, nbytes, None)

    assert compose(S=-1) != 0 and b"lc_scene_compose_f32: a negative size" in msg()
    assert compose(S=0) != 0 and b"at least one scene" in msg()
    assert compose(W=16385, w=16385) != 0 and b"16384" in msg()
    assert compose(w=60) != 0 and b"without origin_xy" in msg()
    assert compose(depth=None) != 0 and b"null" in msg()
    assert compose(ws=None) != 0 and b"null" in msg()
    assert compose(inst=None) != 0 and b"null" in msg()
    assert compose(instance=p + 2) != 0 and b"4-byte" in msg()
    assert compose(ws=p + 4) != 0 and b"8-byte" in msg()
    assert compose(nbytes=2 * 48 * 64 * 8 - 1) != 0 and b"workspace is smaller" in msg()
    assert compose(B=0, S=0) != 0 and b"at least one scene" in msg()  # an empty batch still writes the maps: the frame rules hold


def test_kernels_use_no_scratch_and_little_lds():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, gtinfo

    gtinfo.load()
    res = kernel_resources(build.GTINFO.so_path)
    assert len(res) == 6 and all("lc_gtinfo_" in n or "lc_compose_" in n for n in res), sorted(res)
    for d in res.values():
        assert d.get("private_segment_fixed_size", 0) == 0, (d["name"], "scratch")
        assert d["vgpr_count"] <= 128, d["name"]
        # no LDS beyond the workgroup hand-off: four wavefronts times twelve values
        assert d.get("group_segment_fixed_size", 0) == (4 * 12 * 4 if "reduce" in d["name"] else 0), d["name"]


def test_bop_records():
    from lc_amd import gtinfo

    info = torch.tensor([
        [10, 8, 5, 0, 3, 4, 7, 9, 4, 4, 6, 8],         # a plain row
        [6, 0, 0, 2, -2, -1, 3, 1, -1, -1, -1, -1],    # nothing visible: both boxes -1, although the silhouette has a box
        [4, 4, 4, 0, -1, -1, 2, 0, -1, -1, 0, 0],      # real -1 coordinates
        [0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1],  # an empty render
        [-1] * 12,                                     # a refused row
    ], dtype=torch.int32)
    got = gtinfo.bop_records(info)
    assert [sorted(r) for r in got] == [sorted(("bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"))] * 5
    assert got[0] == dict(bbox_obj=[3, 4, 4, 5], bbox_visib=[4, 4, 2, 4], px_count_all=10, px_count_valid=8, px_count_visib=5, visib_fract=0.5)
    assert got[1] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=6, px_count_valid=0, px_count_visib=0, visib_fract=0.0)
    assert got[2]["bbox_obj"] == [-1, -1, 3, 1] and got[2]["bbox_visib"] == [-1, -1, 1, 1] and got[2]["visib_fract"] == 1.0
    assert got[3] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=0, px_count_valid=0, px_count_visib=0, visib_fract=0.0)
    assert got[4] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=-1, px_count_valid=-1, px_count_visib=-1, visib_fract=0.0)
    assert all(type(r["visib_fract"]) is float and type(r["px_count_all"]) is int and all(type(v) is int for v in r["bbox_obj"]) for r in got)
    plus = gtinfo.bop_records(gtinfo.GtInfo(info, None), bbox_plus_one=True)
    assert plus[0]["bbox_obj"] == [3, 4, 5, 6] and plus[0]["bbox_visib"] == [4, 4, 3, 5] and plus[2]["bbox_obj"] == [-1, -1, 4, 2]
    assert plus[1]["bbox_obj"] == [-1] * 4 and plus[3]["bbox_visib"] == [-1] * 4
    third = torch.tensor([[3, 3, 1, 0, 0, 0, 2, 0, 1, 0, 1, 0]], dtype=torch.int32)
    assert gtinfo.bop_records(third)[0]["visib_fract"] == 1 / 3.0
    assert torch.equal(gtinfo.GtInfo(info, None).visib_fract(), torch.tensor([0.5, 0.0, 1.0, 0.0, 0.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="bop_records takes"):
        gtinfo.bop_records(torch.zeros(3, 11, dtype=torch.int32))
    with pytest.raises(ValueError, match="bop_records takes"):
        gtinfo.bop_records(torch.zeros(3, 12))
