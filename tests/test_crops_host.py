"""Host-side contract of the zoom-in crops: `test_item` against the stored blobs of the unmodified reference loader, header = exports =
ctypes table, the embedded source hash, the other libraries untouched, the entry point's argument checks, kernel resources, the
drop-in's rebinding against stub modules, and the argument errors of the Python surface.  No GPU needed."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import crops_cases as cc
from tests import crops_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "crops_item.npz")


def _dataset():
    return types.SimpleNamespace(**cc.loader_fixture())


def test_test_item_reproduces_the_reference_loaders_blob(monkeypatch):
    from lc_amd import crops

    z = np.load(GOLDEN)
    frame = z["frame"]
    assert np.array_equal(frame, cc.FRAMES[3][0])
    seen = []
    monkeypatch.setattr(crops, "_read_rgb", lambda path: seen.append(path) or frame)
    ds = _dataset()
    state = np.random.get_state()[1].copy()
    for i in range(int(z["n_items"])):
        blob = crops.test_item(ds, i)
        keys = list(z[f"item{i}_keys"])
        assert [k for k in blob if k not in ("rgb_full", "in_affine")] == [k for k in keys if k != "rgb_in"]  # the same keys in the same order
        assert list(blob)[:2] == ["rgb_full", "in_affine"] and keys[0] == "rgb_in"  # the stand-ins where rgb_in stood
        w, h = z["net_input_wh"]
        box = ds.np_annots[i][1].get("bbox_det", ds.np_annots[i][1]["bbox_visib"])
        center, scale = (box[:2] + box[:2] + box[2:]) * 0.5, float(max(box[2], box[3], 1)) * cc.DZI_PAD_SCALE
        for k in keys:
            if k == "rgb_in":
                continue
            got, want = np.asarray(blob[k]), z[f"item{i}_{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape, (i, k)
            if k == "out_K" and i not in cc.EXACT_ITEMS:  # the closed form against the reference's fp32-staged points: bounded, not equal
                tol = np.zeros((3, 3))
                tol[:2] = cc.affine_tolerance(center, scale, cc.NET_OUTPUT_WH) @ np.abs(ds.np_annots[i][0]["cam_K"])
                print(f"item {i} out_K: max |diff| = {np.abs(got - want).max():.3e}, max |diff| / bound = {(np.abs(got - want)[:2] / tol[:2]).max():.3e}")
                assert (np.abs(got - want) <= tol).all(), (i, k, got - want, tol)
            else:
                assert np.array_equal(got, want), (i, k, got, want)
        assert blob["rgb_full"].dtype == np.uint8 and np.array_equal(blob["rgb_full"], frame) and blob["rgb_full"].flags.writeable
        M = blob["in_affine"]
        assert M.dtype == np.float32 and M.shape == (2, 3) and np.array_equal(z[f"call{i}_in_M"], z[f"affine{i}_in"])
        if i in cc.EXACT_ITEMS:
            assert np.array_equal(M, z[f"call{i}_in_M"])  # the M the reference handed to cv2.warpAffine
        else:
            tol = cc.affine_tolerance(center, scale, cc.NET_INPUT_WH)
            diff = np.abs(M.astype(np.float64) - z[f"call{i}_in_M"].astype(np.float64))
            print(f"item {i} in_affine: max |diff| = {diff.max():.3e}, max |diff| / bound = {(diff / tol).max():.3e}")
            assert (diff <= tol).all(), (i, diff, tol)
        M = z[f"call{i}_in_M"]
        # and the stored rgb_in is that warp: the oracle's bytes through the reference's .to(float32).div(255)
        want = torch.from_numpy(co.warp_one(frame, M, (int(h), int(w)))).permute(2, 0, 1).to(torch.float32).div(255).numpy()
        assert z[f"item{i}_rgb_in"].dtype == np.float32 and np.array_equal(want, z[f"item{i}_rgb_in"])
    assert seen == ["frame_000.png"] * 3
    assert np.array_equal(np.random.get_state()[1], state)  # no random number drawn, as in the reference's test branch


def test_affine_from_box_reproduces_the_reference_helper_on_exact_boxes():
    """Both matrices, both sizes: the boxes of the fixture are exact in fp32, so the reference's fp32 staging of the points loses nothing
    and the closed form lands on the same fp32 values as its three-point solve."""
    from lc_amd.crops import affine_from_box

    z = np.load(GOLDEN)
    fx = cc.loader_fixture()
    for i in cc.EXACT_ITEMS:
        inst = fx["np_annots"][i][1]
        box = inst.get("bbox_det", inst["bbox_visib"])
        center, scale = (box[:2] + box[:2] + box[2:]) * 0.5, float(max(box[2], box[3], 1)) * cc.DZI_PAD_SCALE
        for tag, wh in (("in", cc.NET_INPUT_WH), ("out", cc.NET_OUTPUT_WH)):
            M, Mi = affine_from_box(center, scale, 0, wh)
            assert np.array_equal(M, z[f"affine{i}_{tag}"]) and np.array_equal(Mi, z[f"affine{i}_{tag}_inv"]), (i, tag)


def test_header_exports_and_ctypes_table_agree():
    from lc_amd import build, crops

    lib = crops.load()
    header = open(os.path.join(ROOT, "include", "lc_amd_crop.h")).read()
    declared = set(re.findall(r"^(?:const\s+)?\w+\s+\*?(lc_\w+)\(", header, flags=re.M))
    assert declared == set(crops._SIGNATURES) == {"lc_amd_crop_version", "lc_amd_crop_last_error", "lc_amd_crop_source_hash", "lc_crop_warp_u8"}
    out = subprocess.run(["nm", "-D", "--defined-only", build.CROP.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("lc_")} == declared, exported
    assert lib.lc_amd_crop_version() == int(re.search(r"#define LC_AMD_CROP_VERSION (\d+)", header).group(1)) == 1
    consts = {k: int(v) for k, v in re.findall(r"#define (LC_CROP_\w+) (\d+)", header)}
    assert consts["LC_CROP_MAX_SIZE"] == crops.MAX_SIZE
    assert {"nearest": consts["LC_CROP_NEAREST"], "linear": consts["LC_CROP_LINEAR"]} == crops.INTERP
    assert {torch.uint8: consts["LC_CROP_U8"], torch.float32: consts["LC_CROP_F32"], torch.float16: consts["LC_CROP_F16"],
            torch.bfloat16: consts["LC_CROP_BF16"]} == crops.OUT_DTYPES
    proto = re.search(r"int lc_crop_warp_u8\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(crops._SIGNATURES["lc_crop_warp_u8"][1])


def test_embedded_source_hash_and_separate_sources():
    from lc_amd import build, crops

    lib = crops.load()
    assert not build.is_stale(build.CROP)
    assert lib.lc_amd_crop_source_hash().decode() == build.source_hash(build.CROP) == build.embedded_hash(build.CROP.so_path, build.CROP.hash_marker)
    assert build.sources(build.CROP) == [os.path.join(build.CSRC, "crop", "lc_crop.hip")]
    for t in (build.MAIN, build.OPTIM, build.POSECOV, build.RENDER):  # the libraries before this one: not even the word in a file's name
        assert not any("crop" in os.path.basename(s) for s in build._deps(t)), t.name  # (its directory and header: tests/test_libraries_host.py)


def _call(lib, **over):
    """The entry point with host pointers (which never launch: every call here fails a check, or has nothing to do)."""
    import ctypes

    buf = torch.zeros(4096)
    p = buf.data_ptr()
    a = dict(frames=p, F=1, H=8, W=8, C=3, index=None, M=p, B=1, h=4, w=4, interp=1, dtype=1, mean=None, std=None, out=p, info=p, stream=None)
    a.update(over)
    for k in ("mean", "std"):
        if a[k] is not None:
            a[k] = (ctypes.c_float * 3)(*a[k])
    return lib.lc_crop_warp_u8(*a.values()), lib.lc_amd_crop_last_error()


def test_entry_point_checks_its_arguments():
    from lc_amd import crops

    lib = crops.load()
    assert _call(lib, B=0)[0] == 0  # nothing to do: no launch
    assert _call(lib, B=0, frames=None, M=None, out=None)[0] == 0
    rc, msg = _call(lib, B=-1)
    assert rc != 0 and b"B < 0" in msg
    for C in (0, 2, 4):
        rc, msg = _call(lib, C=C)
        assert rc != 0 and b"C must be 1 or 3" in msg
    for kw in (dict(H=0), dict(W=0), dict(h=0), dict(w=crops.MAX_SIZE + 1), dict(H=crops.MAX_SIZE + 1)):
        rc, msg = _call(lib, **kw)
        assert rc != 0 and b"sizes" in msg, kw
    rc, msg = _call(lib, interp=2)
    assert rc != 0 and b"interp" in msg
    for d in (-1, 4):
        rc, msg = _call(lib, dtype=d)
        assert rc != 0 and b"out_dtype" in msg
    for kw in (dict(mean=(0, 0, 0)), dict(std=(1, 1, 1)), dict(mean=(0, 0, 0), std=(1, 1, 1), dtype=0)):
        rc, msg = _call(lib, **kw)
        assert rc != 0 and b"mean and std" in msg, kw
    for name in ("frames", "M", "out"):
        rc, msg = _call(lib, **{name: None})
        assert rc != 0 and b"NULL" in msg, name
    rc, msg = _call(lib, F=-1)
    assert rc != 0 and b"F < 0" in msg


def test_kernels_use_no_scratch_and_a_table_of_finished_values():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, crops

    crops.load()
    res = kernel_resources(build.CROP.so_path)
    assert len(res) == 16 and all("lc_crop_warp_kernel" in n for n in res)  # 4 output types x 2 channel counts x 2 interpolations
    for name, d in res.items():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (name, d)
        assert d.get("group_segment_fixed_size", 0) <= 256 * 3 * 4 + 64, name  # the table of 256 C finished values and the row's inverse matrix


def _stub_reference(monkeypatch):
    """Stub `dataset` and `utils` modules doing what the reference's do at the rebinding points."""
    ds, ut = types.ModuleType("dataset"), types.ModuleType("utils")

    class BOP_Dataset:
        def __init__(self, training):
            self.__dict__.update(cc.loader_fixture())
            self.training = training

        def _get_single_item(self, index):
            return {"rgb_in": "reference", "index": index}

        def collate_fn(self):
            return "collate"

    def xfer_to(pack, device, non_blocking=True):
        if isinstance(pack, dict):
            return {k: ut.xfer_to(v, device, non_blocking=non_blocking) for k, v in pack.items()}  # recursive through the module's name
        return ("moved", pack)

    ds.BOP_Dataset, ut.xfer_to = BOP_Dataset, xfer_to
    monkeypatch.setitem(sys.modules, "dataset", ds)
    monkeypatch.setitem(sys.modules, "utils", ut)
    return ds, ut


def test_dropin_native_crops_rebinds_the_test_loader_and_the_transfer(monkeypatch):
    from lc_amd import crops, dropin

    ds, ut = _stub_reference(monkeypatch)
    test_mod = types.ModuleType("test")
    test_mod.xfer_to = ut.xfer_to  # `from utils import xfer_to` ran before the rebinding
    monkeypatch.setitem(sys.modules, "test", test_mod)
    orig_item, orig_xfer = ds.BOP_Dataset._get_single_item, ut.xfer_to
    monkeypatch.setattr(crops, "_read_rgb", lambda path: cc.FRAMES[3][0])
    monkeypatch.setattr(crops, "_NET_INPUT_HW", None)
    finished = []
    monkeypatch.setattr(crops, "finish_blob", lambda blob: finished.append(blob) or blob)

    done = dropin.install(patch_ptnet=False, gpu_initialiser=False)  # without the flag: nothing of it happens
    assert "crops" not in done and ds.BOP_Dataset._get_single_item is orig_item and ut.xfer_to is orig_xfer and test_mod.xfer_to is orig_xfer

    assert dropin._install_crops() is True
    test_ds, train_ds = ds.BOP_Dataset(False), ds.BOP_Dataset(True)
    assert train_ds._get_single_item(1) == {"rgb_in": "reference", "index": 1}  # training datasets keep the reference's method
    assert train_ds.collate_fn() == "collate" and crops._NET_INPUT_HW is None
    blob = test_ds._get_single_item(1)
    assert "rgb_in" not in blob and np.array_equal(blob["rgb_full"], cc.FRAMES[3][0]) and blob["obj_id"] == 9
    assert crops._NET_INPUT_HW == (cc.NET_INPUT_WH[1], cc.NET_INPUT_WH[0])
    crops.set_net_input_hw(None)
    assert test_ds.collate_fn() == "collate" and crops._NET_INPUT_HW == (cc.NET_INPUT_WH[1], cc.NET_INPUT_WH[0])
    assert ut.xfer_to is not orig_xfer and test_mod.xfer_to is ut.xfer_to
    assert ut.xfer_to({"a": 1}, "dev") == {"a": ("moved", 1)} and finished[-1] == {"a": ("moved", 1)}  # the transfer, then finish_blob

    item, xfer = ds.BOP_Dataset._get_single_item, ut.xfer_to
    assert dropin._install_crops() is True  # idempotent: nothing is wrapped twice
    assert ds.BOP_Dataset._get_single_item is item and ut.xfer_to is xfer and test_mod.xfer_to is xfer

    monkeypatch.setitem(sys.modules, "dataset", None)  # no reference loader: the opt-in says so
    assert dropin._install_crops() is False
    assert dropin.install(patch_ptnet=False, gpu_initialiser=False, native_crops=True)["crops"] is False


def test_dropin_takes_the_native_crops_flag(monkeypatch, tmp_path):
    from lc_amd import dropin

    seen = {}
    monkeypatch.setattr(dropin, "install", lambda **kw: seen.update(kw) or {})
    script = tmp_path / "test.py"
    script.write_text("import sys\nARGS = list(sys.argv)\n")
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    dropin.main(["--native-crops", str(script), "--cfg", "x.yaml"])
    assert seen == dict(native_labels=False, native_crops=True) and sys.argv == [str(script), "--cfg", "x.yaml"]
    seen.clear()
    dropin.main([str(script)])
    assert seen == dict(native_labels=False)  # install() is passed the flag only when asked for


def test_argument_errors_raise():
    from lc_amd.crops import finish_blob, warp_affine

    frames, M = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp_affine(frames, M, (4, 4))
    with pytest.raises(TypeError, match="torch.Tensor"):
        warp_affine(frames.numpy(), M, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        finish_blob({"rgb_full": frames, "in_affine": M}, net_input_hw=(4, 4))
    with pytest.raises(RuntimeError, match="net_input_hw"):
        finish_blob({"rgb_full": frames, "in_affine": M})

    # shape, dtype and layout checks come after the device check: judged on meta-free stand-ins that claim to be on the device
    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)

    def dev(t):
        return t.as_subclass(OnDevice)

    with pytest.raises(ValueError, match=r"C in \(1, 3\)"):
        warp_affine(dev(torch.zeros(1, 8, 8, 2, dtype=torch.uint8)), dev(M), (4, 4))
    with pytest.raises(ValueError, match="contiguous"):
        warp_affine(dev(torch.zeros(1, 8, 3, 8, dtype=torch.uint8).permute(0, 1, 3, 2)), dev(M), (4, 4))
    with pytest.raises(TypeError, match="uint8"):
        warp_affine(dev(frames.float()), dev(M), (4, 4))
    with pytest.raises(ValueError, match=r"\(B,2,3\)"):
        warp_affine(dev(frames), dev(torch.zeros(1, 3, 3)), (4, 4))
    with pytest.raises(ValueError, match="interp"):
        warp_affine(dev(frames), dev(M), (4, 4), interp="cubic")
    with pytest.raises(TypeError, match="dtype"):
        warp_affine(dev(frames), dev(M), (4, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="float dtype"):
        warp_affine(dev(frames), dev(M), (4, 4), dtype=torch.uint8, normalize=cc.NORMALIZE)
    with pytest.raises(ValueError, match="one value per channel"):
        warp_affine(dev(frames), dev(M), (4, 4), normalize=((0.5,), (0.5,)))
    with pytest.raises(ValueError, match="sizes"):
        warp_affine(dev(frames), dev(M), (0, 4))
