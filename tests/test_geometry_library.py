"""The geometry library without a GPU (lc_amd/csrc/geometry/, include/lc_amd_geometry.h, lc_amd/geometry.py, lc_amd/train_inputs.py):
header = exports = ctypes table, its source hash, every refusal of the two entry points
reached with host pointers (nothing launches), the wrappers' refusals, and what the compiler made of the two kernels."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_group_header_exports_and_source_hash():
    import __graft_entry__ as entry
    from lc_amd import build, geometry

    T = build.GEOMETRY  # (its place among the libraries, its files and includes: tests/test_libraries_host.py)
    entry.build()
    lib = geometry.load()
    assert not build.is_stale(T)
    assert lib.lc_amd_geometry_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert build.sources(T) == [os.path.join(build.CSRC, "geometry", "lc_geometry.hip")]
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_GEOMETRY_SRC_HASH"}  # no build switch
    assert "asm" not in re.sub(r"//.*", "", source)

    header = open(os.path.join(ROOT, "include", "lc_amd_geometry.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(geometry._SIGNATURES) and {"lc_geometry_zoom_f32", "lc_geometry_background_f32"} <= declared and len(declared) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_geometry_version() == int(re.search(r"#define LC_AMD_GEOMETRY_VERSION (\d+)", header).group(1)) == 1
    from lc_amd import augment, crops

    assert geometry.MAX_SIZE == crops.MAX_SIZE == int(re.search(r"#define LC_GEOMETRY_MAX_SIZE (\d+)", header).group(1))
    assert augment.OP_ZOOM == int(re.search(r"#define LC_GEOMETRY_OP_ZOOM (\d+)", header).group(1))
    assert augment.OP_BG_REGION == int(re.search(r"#define LC_GEOMETRY_OP_BG_REGION (\d+)", header).group(1))
    assert geometry.OP_STEP_INDEX == int(re.search(r"#define LC_GEOMETRY_STEP_INDEX (\d+)", header).group(1))
    # every prototype's argument list against the ctypes signature: pointers, whole numbers and doubles in the same places
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_double: "d"}
    for name in ("lc_geometry_zoom_f32", "lc_geometry_background_f32"):
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "double": "d"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = geometry._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)
    # the coefficients the kernel holds are the definition's, digit for digit
    for v in (geometry.PI_4,) + geometry.SIN_C + geometry.COS_C:
        assert ("-" if v < 0 else " ") + abs(v).hex() in source.replace("{", " "), v.hex()


def test_two_kernels_without_scratch_or_lds(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, geometry

    geometry.load()
    res = kernel_resources(build.GEOMETRY.so_path)
    assert len(res) == 2, sorted(res)
    for short in ("lc_geometry_zoom_kernel", "lc_geometry_background_kernel"):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d.get("group_segment_fixed_size", 0) == 0, short
        assert d["max_flat_workgroup_size"] == 64, short


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import geometry

    lib = geometry.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_geometry_last_error
    nan, inf = math.nan, math.inf

    def zoom(ratios=(0.25, 0.25, 1.5), prob=1.0, train=1, sizes=(480, 640, 256, 256, 64, 64), seed=p, sid=p, box=p, K=p, stride=9, B=2, in_affine=p,
             out_affine=p, out_K=p, pix=p, step=p, info=p, centre=None, scale=None, cs=None):
        return lib.lc_geometry_zoom_f32(*ratios, prob, train, *sizes, seed, sid, box, K, stride, B, in_affine, out_affine, out_K, pix, step, info, centre, scale, cs, None)

    assert zoom(B=-1) != 0 and b"lc_geometry_zoom_f32: B < 0" in msg()
    assert zoom(B=0) == 0 and zoom(B=0, seed=None, sid=None, box=None, K=None, in_affine=None, out_affine=None, out_K=None, pix=None, step=None, info=None) == 0
    for name in ("seed", "sid", "box", "K", "in_affine", "out_affine", "out_K", "pix", "step", "info"):
        assert zoom(**{name: None}) != 0 and b"NULL" in msg(), name
    for i in range(6):
        for bad in (0, -3, 16385):
            sizes = [480, 640, 256, 256, 64, 64]
            sizes[i] = bad
            assert zoom(sizes=tuple(sizes)) != 0 and b"[1, 16384], got" in msg() and str(bad).encode() in msg(), (i, bad)
    sizes = (16384,) * 6
    assert zoom(sizes=sizes, B=0) == 0
    for i in range(3):
        for bad in (nan, inf, -inf):
            ratios = [0.25, 0.25, 1.5]
            ratios[i] = bad
            assert zoom(ratios=tuple(ratios)) != 0 and b"must be finite" in msg(), (i, bad)
    for bad in (-1e-9, 1.0000001, nan, inf):
        assert zoom(prob=bad) != 0 and b"rotate_prob must lie in [0, 1]" in msg(), bad
    for bad in (1, 3, 8, 10, -9):
        assert zoom(stride=bad) != 0 and b"K_stride must be 0" in msg() and str(bad).encode() in msg(), bad
    assert zoom(seed=p + 4) != 0 and b"aligned to 8 bytes" in msg()
    for name in ("centre", "scale", "cs"):
        assert zoom(**{name: p + 4}) != 0 and b"aligned to 8 bytes" in msg(), name
    for name in ("sid", "box", "K", "in_affine", "out_affine", "out_K", "pix", "step", "info"):
        assert zoom(**{name: p + 2}) != 0 and b"aligned to 4 bytes" in msg(), name

    def background(seed=p, sid=p, bg=(100, 120), pairs=None, out=(64, 48), B=2, M=p):
        return lib.lc_geometry_background_f32(seed, sid, bg[0], bg[1], pairs, out[0], out[1], B, M, None)

    assert background(B=-1) != 0 and b"lc_geometry_background_f32: B < 0" in msg()
    assert background(B=0) == 0 and background(B=0, seed=None, sid=None, M=None) == 0
    for name in ("seed", "sid", "M"):
        assert background(**{name: None}) != 0 and b"NULL" in msg(), name
    for bad in ((0, 48), (64, 0), (16385, 48), (64, 16385)):
        assert background(out=bad) != 0 and b"out_h and out_w must be in [1, 16384]" in msg(), bad
        assert background(bg=bad) != 0 and b"bg_h and bg_w must be in [1, 16384] where bg_hw is NULL" in msg(), bad
    assert background(seed=p + 4) != 0 and b"aligned to 8 bytes" in msg()
    for name in ("sid", "pairs", "M"):
        assert background(**{name: p + 2}) != 0 and b"aligned to 4 bytes" in msg(), name


def test_wrapper_refusals():
    from lc_amd import geometry
    from lc_amd.augment import AugmentConfig

    cfg = AugmentConfig()
    sid, box, K = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4), torch.eye(3)

    def zoom(cfg=cfg, seed=1, sample_id=sid, bbox_xyxy=box, im_hw=(480, 640), cam_K=K, in_wh=(256, 256), out_wh=(64, 64), **kw):
        return geometry.zoom_geometry(cfg, seed=seed, sample_id=sample_id, bbox_xyxy=bbox_xyxy, im_hw=im_hw, cam_K=cam_K, in_wh=in_wh, out_wh=out_wh, **kw)

    with pytest.raises(TypeError, match="lc_amd.geometry: cfg must be an AugmentConfig"):
        zoom(cfg={"rotate_prob": 1})
    with pytest.raises(ValueError, match="dzi_pad_scale must be finite"):
        zoom(cfg=AugmentConfig(dzi_pad_scale=math.inf))
    with pytest.raises(ValueError, match=r"rotate_prob must lie in \[0, 1\], got 1.5"):
        zoom(cfg=AugmentConfig(rotate_prob=1.5))
    with pytest.raises(TypeError, match="train and want_info are bools"):
        zoom(train=1)
    with pytest.raises(TypeError, match="sample_id must be a torch.Tensor"):
        zoom(sample_id=np.zeros(3, np.int32))
    with pytest.raises(TypeError, match="sample_id must be int32, got torch.int64"):
        zoom(sample_id=sid.long())
    with pytest.raises(ValueError, match=r"sample_id has shape \(3, 1\)"):
        zoom(sample_id=sid[:, None])
    with pytest.raises(TypeError, match="bbox_xyxy must be float32, got torch.float64"):
        zoom(bbox_xyxy=box.double())
    with pytest.raises(ValueError, match=r"bbox_xyxy has shape \(2, 4\), expected \(3, 4\)"):
        zoom(bbox_xyxy=box[:2])
    with pytest.raises(ValueError, match=r"cam_K has shape \(2, 3, 3\), expected \(3, 3, 3\)"):
        zoom(cam_K=K.expand(2, 3, 3))
    with pytest.raises(TypeError, match="cam_K must be float32"):
        zoom(cam_K=K.half())
    with pytest.raises(ValueError, match="im_hw of 1 to 16384, got 0"):
        zoom(im_hw=(0, 640))
    with pytest.raises(ValueError, match="in_wh is a pair"):
        zoom(in_wh=256)
    with pytest.raises(TypeError, match="out_wh must be a whole number"):
        zoom(out_wh=(64.0, 64))
    with pytest.raises(ValueError, match="seed of 0 to 18446744073709551615, got -1"):
        zoom(seed=-1)
    with pytest.raises(TypeError, match="a seed tensor holds one uint64 or int64 element"):
        zoom(seed=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="lc_amd.geometry: sample_id is on cpu.*no CPU fallback"):  # everything in order, but for the device
        zoom()

    def background(seed=1, sample_id=sid, bg_hw=(100, 120), out_hw=(64, 48)):
        return geometry.background_geometry(seed=seed, sample_id=sample_id, bg_hw=bg_hw, out_hw=out_hw)

    with pytest.raises(TypeError, match="sample_id must be int32"):
        background(sample_id=sid.float())
    with pytest.raises(TypeError, match="bg_hw must be int32, got torch.int64"):
        background(bg_hw=torch.ones(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"bg_hw has shape \(2, 2\), expected \(3, 2\)"):
        background(bg_hw=torch.ones(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="bg_hw of 1 to 16384, got 0"):
        background(bg_hw=(100, 0))
    with pytest.raises(ValueError, match="out_hw of 1 to 16384, got 16385"):
        background(out_hw=(16385, 48))
    with pytest.raises(ValueError, match="seed of 0 to"):
        background(seed=2 ** 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        background()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        background(bg_hw=torch.ones(3, 2, dtype=torch.int32))


def test_train_inputs_refusals():
    from lc_amd import train_inputs as ti
    from lc_amd.augment import AugmentConfig

    assert callable(ti.train_inputs)
    frames, masks = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint8)
    B = 5
    base = dict(frame_index=torch.zeros(B, dtype=torch.int32), masks=masks, mask_index=torch.zeros(B, dtype=torch.int32), bbox_xyxy=torch.zeros(B, 4),
                cam_K=torch.eye(3), sample_id=torch.zeros(B, dtype=torch.int32), cfg=AugmentConfig(), seed=3, in_hw=(32, 32), out_hw=(16, 16))

    def call(**kw):
        a = {**base, **kw}
        return ti.train_inputs(frames, a.pop("frame_index"), **a)

    for name in ("frame_index", "mask_index", "bbox_xyxy", "sample_id"):
        with pytest.raises(ValueError, match="the per-row tensors disagree on B"):
            call(**{name: base[name][:4]})
    with pytest.raises(ValueError, match="the per-row tensors disagree on B"):
        call(cam_K=torch.eye(3).expand(4, 3, 3))
    with pytest.raises(TypeError, match="sample_id must be a"):
        call(sample_id=[0] * B)
    with pytest.raises(ValueError, match="one of the two"):
        call(rle_store=object())  # masks given together with a store
    with pytest.raises(ValueError, match="one of the two"):
        call(masks=None)
    with pytest.raises(TypeError, match="rle_store must be an RleStore"):
        call(masks=None, rle_store=object())
    with pytest.raises(ValueError, match="meshes need mesh_index, R, t, near and far; R, t missing"):
        call(meshes=object(), mesh_index=torch.zeros(B, dtype=torch.int32), near=0.1, far=10.0)
    with pytest.raises(ValueError, match="R given without meshes"):
        call(R=torch.eye(3).expand(B, 3, 3))
    with pytest.raises(ValueError, match=r"masks has shape \(2, 48, 60\)"):
        call(masks=masks[:, :, :60])
    with pytest.raises(TypeError, match="frames must be uint8"):
        ti.train_inputs(frames.float(), **base)
    with pytest.raises(ValueError, match="in_hw of 1 to 16384, got 0"):
        call(in_hw=(0, 32))
    with pytest.raises(RuntimeError, match="lc_amd.train_inputs: frames is on cpu.*no CPU fallback"):
        call()
