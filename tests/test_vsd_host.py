"""VSD without a GPU: the wrapper's refusals (lc_amd.vsd), the library of its own (liblc_amd_vsd.so: header, exports, signatures and source
hash agree; its place among the libraries: tests/test_libraries_host.py), the argument checks of the C entry point before any launch, and the
kernels' resources read from the code object (no scratch)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good(B=3, h=4, w=5):
    return dict(depth_est=torch.zeros(B, h, w), depth_gt=torch.zeros(B, h, w), depth_test=torch.zeros(h, w), K=torch.eye(3), delta=15.0,
                taus=(0.1, 0.2))


def test_build_groups():
    import __graft_entry__ as entry
    from lc_amd import build

    entry.build()  # (the registry and the build order: tests/test_libraries_host.py) leaves this library in place and current
    assert os.path.exists(build.VSD.so_path) and not build.is_stale(build.VSD)


def test_library_header_exports_and_signatures_agree():
    from lc_amd import build, vsd

    lib = vsd.load()
    header = open(os.path.join(ROOT, "include", "lc_amd_vsd.h")).read()
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(vsd._SIGNATURES) and "lc_vsd_score_f32" in declared
    out = subprocess.run(["nm", "-D", "--defined-only", build.VSD.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_vsd_version() == int(re.search(r"#define LC_AMD_VSD_VERSION (\d+)", header).group(1)) == 1
    assert vsd.MAX_TAUS == int(re.search(r"#define LC_VSD_MAX_TAUS (\d+)", header).group(1))
    assert vsd.MAX_SIZE == int(re.search(r"#define LC_VSD_MAX_SIZE (\d+)", header).group(1))
    # the prototype's argument list against the ctypes signature: pointers, ints and floats in the same places
    proto = re.search(r"int lc_vsd_score_f32\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    kinds = ["p" if "*" in a else a.split()[0][0] for a in proto.split(",")]
    res, args = vsd._SIGNATURES["lc_vsd_score_f32"]
    have = ["p" if a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)) else {ctypes.c_int: "i", ctypes.c_float: "f"}[a] for a in args]
    assert res is ctypes.c_int and kinds == have, (kinds, have)


def test_source_hash_is_its_own():
    from lc_amd import build, vsd

    lib = vsd.load()
    assert not build.is_stale(build.VSD)
    assert lib.lc_amd_vsd_source_hash().decode() == build.source_hash(build.VSD) == build.embedded_hash(build.VSD.so_path, build.VSD.hash_marker)
    assert build.sources(build.VSD) == [os.path.join(build.CSRC, "vsd", "lc_vsd.hip")]
    assert not os.path.exists(os.path.join(build.CSRC, "render", "lc_vsd.hip"))


def test_wrapper_refusals_of_the_score():
    from lc_amd import vsd

    f = vsd.vsd_from_depth
    with pytest.raises(TypeError, match="depth_est must be a torch.Tensor"):
        f(**dict(_good(), depth_est=np.zeros((3, 4, 5), np.float32)))
    with pytest.raises(TypeError, match="depth_gt must be float32"):
        f(**dict(_good(), depth_gt=torch.zeros(3, 4, 5, dtype=torch.float64)))
    with pytest.raises(TypeError, match="depth_test must be float32"):
        f(**dict(_good(), depth_test=torch.zeros(4, 5, dtype=torch.float16)))
    with pytest.raises(TypeError, match="K must be float32"):
        f(**dict(_good(), K=torch.eye(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"depth_est has shape \(4, 5\)"):
        f(**dict(_good(), depth_est=torch.zeros(4, 5)))
    with pytest.raises(ValueError, match=r"depth_gt has shape \(2, 4, 5\)"):
        f(**dict(_good(), depth_gt=torch.zeros(2, 4, 5)))
    with pytest.raises(ValueError, match=r"K has shape \(2, 3, 3\)"):
        f(**dict(_good(), K=torch.zeros(2, 3, 3)))
    with pytest.raises(ValueError, match="must have the frame's size"):
        f(**dict(_good(), depth_test=torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="does not fit"):
        f(**dict(_good(), depth_test=torch.zeros(3, 8), window_xy=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="scene_index is needed"):
        f(**dict(_good(), depth_test=torch.zeros(2, 4, 5)))
    with pytest.raises(TypeError, match="scene_index must be int32 or int64"):
        f(**dict(_good(), scene_index=torch.zeros(3)))
    with pytest.raises(ValueError, match=r"scene_index has shape \(2,\)"):
        f(**dict(_good(), scene_index=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(TypeError, match="window_xy must be a torch.Tensor"):
        f(**dict(_good(), window_xy=[(0, 0)] * 3))
    with pytest.raises(ValueError, match=r"window_xy has shape \(3,\)"):
        f(**dict(_good(), window_xy=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(TypeError, match="diameter must be float32"):
        f(**dict(_good(), diameter=torch.ones(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"diameter has shape \(1,\)"):
        f(**dict(_good(), diameter=torch.ones(1)))
    with pytest.raises(ValueError, match="1 to 16 taus"):
        f(**dict(_good(), taus=()))
    with pytest.raises(ValueError, match="1 to 16 taus"):
        f(**dict(_good(), taus=[0.1] * 17))
    with pytest.raises(TypeError, match="taus must be a sequence"):
        f(**dict(_good(), taus=torch.ones(3)))
    with pytest.raises(TypeError, match="taus must be a sequence"):
        f(**dict(_good(), taus=0.1))
    with pytest.raises(ValueError, match="taus must be finite"):
        f(**dict(_good(), taus=(0.1, float("nan"))))
    with pytest.raises(TypeError, match="delta must be a number"):
        f(**dict(_good(), delta=torch.tensor(15.0)))
    with pytest.raises(ValueError, match="delta must be finite and not negative"):
        f(**dict(_good(), delta=-1.0))
    with pytest.raises(ValueError, match="pixel_center"):
        f(**dict(_good(), pixel_center=0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order: the maps are not on the HIP device
        f(**_good())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**dict(_good(), diameter=torch.ones(3), scene_index=torch.zeros(3, dtype=torch.int32), window_xy=torch.zeros(3, 2, dtype=torch.int64)))


def _stand_in(device="cuda:0"):
    """A MeshSet without a device behind it (its constructor refuses the CPU): what the wrapper looks at before it renders."""
    from lc_amd import render

    m = object.__new__(render.MeshSet)
    m.device, m.n_meshes = torch.device(device), 3
    return m


def _good_poses(B=3):
    return dict(meshes=_stand_in(), mesh_index=torch.zeros(B, dtype=torch.int32), R_est=torch.zeros(B, 3, 3), t_est=torch.zeros(B, 3),
                R_gt=torch.zeros(B, 3, 3), t_gt=torch.zeros(B, 3, 1), K=torch.eye(3), depth_test=torch.zeros(4, 5), delta=15.0, taus=(0.1,), near=0.01,
                far=6.5)


def test_wrapper_refusals_of_the_chain():
    from lc_amd import vsd

    f = vsd.compute_vsd
    with pytest.raises(TypeError, match="MeshSet"):
        f(**dict(_good_poses(), meshes=[(None, None)]))
    with pytest.raises(TypeError, match="mesh_index must be an int32 tensor"):
        f(**dict(_good_poses(), mesh_index=torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"mesh_index has shape \(3, 1\)"):
        f(**dict(_good_poses(), mesh_index=torch.zeros(3, 1, dtype=torch.int32)))
    with pytest.raises(TypeError, match="R_est must be float32"):
        f(**dict(_good_poses(), R_est=torch.zeros(3, 3, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"R_gt has shape \(2, 3, 3\)"):
        f(**dict(_good_poses(), R_gt=torch.zeros(2, 3, 3)))
    with pytest.raises(ValueError, match=r"t_est has shape \(3, 1, 3\)"):
        f(**dict(_good_poses(), t_est=torch.zeros(3, 1, 3)))
    with pytest.raises(TypeError, match="t_gt must be a torch.Tensor"):
        f(**dict(_good_poses(), t_gt=np.zeros((3, 3), np.float32)))
    with pytest.raises(ValueError, match="go together"):
        f(**dict(_good_poses(), window_hw=(2, 2)))
    with pytest.raises(ValueError, match="does not fit"):
        f(**dict(_good_poses(), window_hw=(5, 5), window_xy=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="1 to 16 taus"):
        f(**dict(_good_poses(), taus=()))
    with pytest.raises(RuntimeError, match="mesh_index is on cpu, the meshes are on cuda:0"):
        f(**_good_poses())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.vsd_from_states(_stand_in(), torch.zeros(3, dtype=torch.int32), torch.ones(3, 7), torch.ones(3, 7), torch.eye(3), torch.zeros(4, 5),
                            delta=15.0, taus=(0.1,), near=0.01, far=6.5)


def test_window_origins_on_the_host():
    """Plain elementwise torch: it runs wherever its tensors live.  Centred on the midpoint of the two projected centres, clamped."""
    from lc_amd import vsd

    K = torch.tensor([[100.0, 0.0, 320.0], [0.0, 100.0, 240.0], [0.0, 0.0, 1.0]])
    t_gt = torch.tensor([[0.0, 0.0, 1.0], [-5.0, -5.0, 1.0], [5.0, 5.0, 1.0], [0.1, 0.2, 1.0]])
    t_est = torch.tensor([[0.2, 0.0, 1.0], [-5.0, -5.0, 1.0], [5.0, 5.0, 1.0], [0.1, 0.2, 2.0]])
    out = vsd.window_origins(t_est, t_gt, K, None, (64, 96), (480, 640))
    assert out.dtype == torch.int32 and out.shape == (4, 2)
    # row 0: centres at x = 320 and 340 -> 330 - 48; rows 1, 2: far outside, clamped; row 3: (330, 260) and (325, 250) -> (327.5, 255)
    assert out.tolist() == [[282, 208], [0, 0], [640 - 96, 480 - 64], [280, 223]]
    with pytest.raises(ValueError, match="does not fit"):
        vsd.window_origins(t_est, t_gt, K, None, (481, 96), (480, 640))
    with pytest.raises(ValueError, match=r"diameter has shape \(2,\)"):
        vsd.window_origins(t_est, t_gt, K, torch.ones(2), (64, 96), (480, 640))


def test_entry_point_checks_its_arguments_before_launching():
    from lc_amd import vsd

    lib = vsd.load()
    buf = ctypes.create_string_buffer(2048)
    p = (ctypes.addressof(buf) + 15) & ~15
    taus = (ctypes.c_float * 16)(*([0.1] * 16))

    def call(est=p, gt=p, test=p, scene=p, K=p, diam=p, taus=taus, T=10, delta=15.0, win=None, B=4, h=48, w=64, S=2, H=48, W=64, counts=p, errors=p):
        return lib.lc_vsd_score_f32(est, gt, test, scene, K, diam, taus, T, delta, win, B, h, w, S, H, W, 0.0, 0.0, counts, errors, None)

    msg = lib.lc_amd_vsd_last_error
    assert call(B=-1) != 0 and b"negative" in msg()
    assert call(w=-1) != 0 and b"negative" in msg()
    assert call(T=0) != 0 and b"thresholds" in msg()
    assert call(T=17) != 0 and b"thresholds" in msg()
    assert call(S=0) != 0 and b"at least one scene" in msg()
    assert call(H=16385, h=16385) != 0 and b"16384" in msg()
    assert call(h=49, win=p) != 0 and b"fit the frame" in msg()
    assert call(h=0) != 0 and b"fit the frame" in msg()
    assert call(h=40) != 0 and b"without window_xy" in msg()
    assert call(est=None) != 0 and b"null" in msg()
    assert call(scene=None) != 0 and b"null" in msg()
    assert call(taus=None) != 0 and b"null" in msg()
    assert call(errors=None) != 0 and b"null" in msg()
    assert call(gt=p + 2) != 0 and b"4-byte" in msg()
    assert call(diam=p + 1) != 0 and b"4-byte" in msg()
    assert call(win=p + 3, h=40) != 0 and b"4-byte" in msg()
    assert call(B=1 << 30, h=16384, H=16384) != 0 and b"2^31" in msg()
    assert lib.lc_vsd_score_f32(*([None] * 7), 0, 0.0, None, 0, 0, 0, 0, 0, 0, 0.0, 0.0, None, None, None) == 0  # an empty batch is a no-op


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, vsd

    vsd.load()
    res = kernel_resources(build.VSD.so_path)  # reads the code object with the llvm-readelf of the ROCm the library was built with
    assert len(res) == 3 and all("lc_vsd_" in n for n in res), sorted(res)
    for d in res.values():
        assert d.get("private_segment_fixed_size", 0) == 0, (d["name"], "scratch")
        assert d["vgpr_count"] <= 128, d["name"]
