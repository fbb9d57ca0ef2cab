"""The symmetry-aware pose errors without a GPU: the wrapper's refusals (lc_amd.metrics.compute_sym_pose_errors), the library of its own
(liblc_amd_symerr.so: header, exports, signatures and source hash agree; no other library sees its sources), the argument checks of the C
entry point before any launch, the argument-rule header under AddressSanitizer + UBSan as a stand-alone program, and the kernels'
resources read from the code object (no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stand_in(device="cuda:0"):
    """A SymmetrySet without a device behind it (its constructor refuses the CPU): what the wrapper looks at before it launches."""
    from lc_amd import symmetry

    s = object.__new__(symmetry.SymmetrySet)
    s.device, s.n_obj, s.total, s.max_k = torch.device(device), 2, 5, 4
    return s


def _good(B=3, M=10):
    return dict(R_est=torch.zeros(B, 3, 3), t_est=torch.zeros(B, 3), R_gt=torch.zeros(B, 3, 3), t_gt=torch.zeros(B, 3, 1), cam_K=torch.eye(3),
                pts=torch.zeros(M, 3), syms=_stand_in("cpu"), obj_index=torch.zeros(B, dtype=torch.int32))


def test_wrapper_refusals():
    from lc_amd import metrics

    f = metrics.compute_sym_pose_errors
    with pytest.raises(TypeError, match="SymmetrySet"):
        f(**dict(_good(), syms={"1": {}}))
    with pytest.raises(RuntimeError, match="the SymmetrySet is on cuda:0, the poses are on cpu"):
        f(**dict(_good(), syms=_stand_in("cuda:0")))
    with pytest.raises(TypeError, match="R_est must be a torch.Tensor"):
        f(**dict(_good(), R_est=np.zeros((3, 3, 3), np.float32)))
    with pytest.raises(TypeError, match="R_gt must be float32"):
        f(**dict(_good(), R_gt=torch.zeros(3, 3, 3, dtype=torch.float64)))
    with pytest.raises(TypeError, match="cam_K must be float32"):
        f(**dict(_good(), cam_K=torch.eye(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"R_est has shape \(3, 9\)"):
        f(**dict(_good(), R_est=torch.zeros(3, 9)))
    with pytest.raises(ValueError, match=r"R_gt has shape \(2, 3, 3\)"):
        f(**dict(_good(), R_gt=torch.zeros(2, 3, 3)))
    with pytest.raises(ValueError, match=r"t_est has shape \(3, 1, 3\)"):
        f(**dict(_good(), t_est=torch.zeros(3, 1, 3)))
    with pytest.raises(ValueError, match=r"cam_K has shape \(2, 3, 3\)"):
        f(**dict(_good(), cam_K=torch.zeros(2, 3, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything else in order: the poses are not on the HIP device
        f(**_good())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.sym_pose_errors_from_states(torch.ones(3, 7), torch.ones(3, 7), torch.eye(3), torch.zeros(10, 3), _stand_in("cpu"), torch.zeros(3, dtype=torch.int32))


def test_wrapper_refusals_past_the_poses(monkeypatch):
    """The checks behind the pose tensors, reached by letting CPU tensors pass for device tensors (nothing is launched: every call raises)."""
    from lc_amd import _lib, metrics

    monkeypatch.setattr(_lib, "require_hip_f32", lambda name, t: t.float().contiguous())
    monkeypatch.setattr(metrics, "load_symerr", lambda: None)
    f = metrics.compute_sym_pose_errors
    with pytest.raises(TypeError, match="obj_index must be a torch.Tensor"):
        f(**dict(_good(), obj_index=[0, 0, 0]))
    with pytest.raises(TypeError, match="obj_index must be int32 or int64"):
        f(**dict(_good(), obj_index=torch.zeros(3)))
    with pytest.raises(ValueError, match=r"obj_index has shape \(2,\)"):
        f(**dict(_good(), obj_index=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match="vertices are missing"):
        f(**dict(_good(), pts=None))
    with pytest.raises(ValueError, match="go together"):
        f(**dict(_good(), pts_off=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(TypeError, match="pts_cnt must be int32 or int64"):
        f(**dict(_good(), pts_off=torch.zeros(3, dtype=torch.int32), pts_cnt=torch.zeros(3)))
    with pytest.raises(ValueError, match=r"pts has shape \(10, 2\)"):
        f(**dict(_good(), pts=torch.zeros(10, 2)))
    with pytest.raises(TypeError, match="pts must be float32"):
        f(**dict(_good(), pts=torch.zeros(10, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="holds no vertex"):
        f(**dict(_good(), pts=torch.zeros(0, 3)))
    with pytest.raises(ValueError, match="mesh_index goes with meshes"):
        f(**dict(_good(), mesh_index=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(TypeError, match="MeshSet"):
        f(**dict(_good(), pts=None, meshes=torch.zeros(10, 3)))

    class Meshes:
        verts, table, n_meshes, device = torch.zeros(10, 3), torch.tensor([[0, 10, 0, 1]], dtype=torch.int32), 1, torch.device("cuda:0")

    with pytest.raises(ValueError, match="not both"):
        f(**dict(_good(), meshes=Meshes))
    with pytest.raises(RuntimeError, match="the MeshSet is on cuda:0, the poses are on cpu"):
        f(**dict(_good(), pts=None, meshes=Meshes))


def test_library_header_exports_and_signatures_agree():
    from lc_amd import build, metrics

    lib = metrics.load_symerr()
    header = open(os.path.join(ROOT, "include", "lc_amd_symerr.h")).read()
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(metrics._SYMERR_SIGNATURES) and {"lc_sym_pose_errors_f32", "lc_sym_pose_errors_workspace_bytes"} <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", build.SYMERR.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_symerr_version() == int(re.search(r"#define LC_AMD_SYMERR_VERSION (\d+)", header).group(1)) == 1
    assert not build.is_stale(build.SYMERR)
    assert lib.lc_amd_symerr_source_hash().decode() == build.source_hash(build.SYMERR) == build.embedded_hash(build.SYMERR.so_path, build.SYMERR.hash_marker)
    assert build.sources(build.SYMERR) == [os.path.join(build.CSRC, "symerr", "lc_sym_metrics.hip")]
    deps = build._deps(build.SYMERR)  # what the source includes from outside its directory is hashed with it (tests/test_libraries_host.py)
    assert os.path.join(build.CSRC, "lc_sym_args.h") in deps and build.SHARED_H in deps


def test_entry_point_checks_its_arguments_before_launching():
    from lc_amd import metrics

    lib = metrics.load_symerr()
    ws_bytes = lib.lc_sym_pose_errors_workspace_bytes
    assert ws_bytes(0, 8) == 0 and ws_bytes(4, 0) == 0 and ws_bytes(1, 1) == 24 and ws_bytes(1, 8) == 24 and ws_bytes(1, 9) == 40
    assert ws_bytes(64, 768) == 64 * (2 * 96 + 1) * 8
    buf = ctypes.create_string_buffer(2048)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(Re=p, te=p, Rg=p, tg=p, K=p, pts=p, off=p, cnt=p, P=700, idx=p, tab=p, ooff=p, ok=p, n_obj=4, rows=43, max_k=36, B=12, err=p, arg=p, ws=p,
             bytes_=12 * 11 * 8):
        return lib.lc_sym_pose_errors_f32(Re, te, Rg, tg, K, pts, off, cnt, P, idx, tab, ooff, ok, n_obj, rows, max_k, B, err, arg, ws, bytes_, None)

    msg = lib.lc_amd_symerr_last_error
    assert call(B=-1) != 0 and b"size" in msg()
    assert call(P=-1) != 0 and b"size" in msg()
    assert call(P=1 << 30) != 0 and b"2^31" in msg()
    assert call(B=1 << 30, max_k=9) != 0 and b"chunks" in msg()
    assert call(P=0) != 0 and b"at least one vertex" in msg()
    assert call(max_k=0) != 0 and b"max_k" in msg()
    assert call(Re=None) != 0 and b"null" in msg()
    assert call(K=None) != 0 and b"null" in msg()
    assert call(err=None) != 0 and b"null" in msg()
    assert call(off=None) != 0 and b"go together" in msg()
    assert call(off=None, cnt=None, ws=None) != 0 and b"null workspace" in msg()
    assert call(pts=p + 2) != 0 and b"4-byte" in msg()
    assert call(arg=p + 1) != 0 and b"4-byte" in msg()
    assert call(ws=p + 4) != 0 and b"8-byte" in msg()
    assert call(bytes_=12 * 11 * 8 - 1) != 0 and b"smaller" in msg()
    assert call(n_obj=0) != 0 and b"at least one object" in msg()
    assert call(rows=1 << 28) != 0 and b"2^31" in msg()
    assert call(tab=None) != 0 and b"null" in msg()
    assert call(tab=p + 4) != 0 and b"8-byte" in msg()
    assert call(idx=p + 2) != 0 and b"4-byte" in msg()
    assert lib.lc_sym_pose_errors_f32(*([None] * 8), 0, *([None] * 4), 0, 0, 0, 0, None, None, None, 0, None) == 0  # an empty batch is a no-op


def test_argument_rules_under_sanitizers(tmp_path):
    """lc_sym_metrics_args.h in a stand-alone program with its own main, AddressSanitizer + UBSan, run directly (nothing is preloaded)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "sym_metrics_args_sanitize"
    src = os.path.join(ROOT, "tests", "native", "sym_metrics_args_sanitize.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, metrics

    metrics.load_symerr()
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = kernel_resources(build.SYMERR.so_path)
    hits = [d for n, d in res.items() if "lc_sym_pose_errors" in n]
    assert len(hits) == 2 == len(res), sorted(res)
    for d in hits:
        assert d.get("private_segment_fixed_size", 0) == 0, (d["name"], "scratch")
        assert d["vgpr_count"] <= 256, d["name"]
