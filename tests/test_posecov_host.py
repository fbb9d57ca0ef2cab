"""Host-side contract of the pose-covariance library (liblc_amd_posecov.so): header = exports = ctypes table, the embedded source hash,
the main library's sources untouched, kernel resources, and the errors of the Python surface.  No GPU needed."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_ctypes_table_agree():
    from lc_amd import build, posecov

    lib = posecov.load()
    header = open(os.path.join(ROOT, "include", "lc_amd_posecov.h")).read()
    declared = set(re.findall(r"^(?:const\s+)?\w+\s+\*?(lc_\w+)\(", header, flags=re.M))
    assert declared == set(posecov._SIGNATURES) == {"lc_amd_posecov_version", "lc_amd_posecov_last_error", "lc_amd_posecov_source_hash", "lc_pose_cov_f32"}
    out = subprocess.run(["nm", "-D", "--defined-only", build.POSECOV.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("lc_")} == declared, exported
    assert lib.lc_amd_posecov_version() == int(re.search(r"#define LC_AMD_POSECOV_VERSION (\d+)", header).group(1)) == 1
    consts = dict(re.findall(r"#define (LC_POSE_COV_\w+) (\d+)", header))
    assert (int(consts["LC_POSE_COV_NAN_TO_NUM"]), int(consts["LC_POSE_COV_WEIGHTS_ARE_STD"]), int(consts["LC_POSE_COV_SCALAR_WEIGHTS"]),
            int(consts["LC_POSE_COV_2D"]), int(consts["LC_POSE_COV_MAX_POINTS"])) == (posecov.NAN_TO_NUM, posecov.WEIGHTS_ARE_STD, posecov.SCALAR_WEIGHTS,
                                                                                        posecov.COV_2D, posecov.MAX_POINTS)
    # the argument count of the ctypes signature is the header's
    proto = re.search(r"int lc_pose_cov_f32\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(posecov._SIGNATURES["lc_pose_cov_f32"][1])


def test_embedded_source_hash_and_separate_sources():
    from lc_amd import build, posecov

    lib = posecov.load()
    assert lib.lc_amd_posecov_source_hash().decode() == build.source_hash(build.POSECOV) == build.embedded_hash(build.POSECOV.so_path, build.POSECOV.hash_marker)
    assert build.sources(build.POSECOV) == [os.path.join(build.CSRC, "posecov", "lc_pose_cov.hip")]
    for t in build.TARGETS:  # no other library hashes a path with this one's name in it (its directory and header: tests/test_libraries_host.py)
        assert t is build.POSECOV or not any("posecov" in os.path.relpath(s, ROOT) for s in build._deps(t))


def _quoted_includes(path):
    return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in re.findall(r'#include "([^"]+)"', open(path).read())]


def test_every_library_hashes_every_file_it_includes():
    """A library's hash sees every edit that can change it: whatever its .hip and .h files include with quotes, followed through the
    included files, is one of the files the hash is taken over, for EVERY library.  (That a shared header belongs to exactly the
    libraries that include it: tests/test_libraries_host.py.)"""
    from lc_amd import build

    for t in build.TARGETS:
        deps = {os.path.normpath(d) for d in build._deps(t)}
        assert all(os.path.exists(d) for d in deps), t.name
        seen, todo = set(), sorted(deps)
        while todo:
            f = todo.pop()
            if f in seen:
                continue
            seen.add(f)
            assert f in deps, f"{t.name}: {f} is included but not hashed"
            todo += _quoted_includes(f)


def test_entry_point_checks_its_arguments():
    from lc_amd import posecov

    lib = posecov.load()
    assert lib.lc_pose_cov_f32(*([None] * 8), 0, 16, 0, 1, 1, *([None] * 5)) == 0  # nothing to do: no launch
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert lib.lc_pose_cov_f32(*([p] * 5), None, p, None, 2, 0, 0, 2, 2, p, p, p, p, None) != 0 and b"N must be" in lib.lc_amd_posecov_last_error()
    assert lib.lc_pose_cov_f32(*([p] * 5), None, p, None, 2, posecov.MAX_POINTS + 1, 0, 2, 2, p, p, p, p, None) != 0
    assert lib.lc_pose_cov_f32(None, *([p] * 4), None, p, None, 2, 8, 0, 2, 2, p, p, p, p, None) != 0 and b"NULL" in lib.lc_amd_posecov_last_error()
    assert lib.lc_pose_cov_f32(*([p] * 5), None, p, None, 3, 8, 0, 2, 3, p, p, p, p, None) != 0 and b"divisors" in lib.lc_amd_posecov_last_error()
    assert lib.lc_pose_cov_f32(*([p] * 5), None, p, None, 2, 8, 64, 2, 2, p, p, p, p, None) != 0 and b"option" in lib.lc_amd_posecov_last_error()


def test_kernels_use_no_scratch_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, posecov

    posecov.load()
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = kernel_resources(build.POSECOV.so_path)
    assert sorted(n for n in res) == sorted(n for n in res if "lc_pose_cov_kernel" in n) and len(res) == 2  # the two forms tests/test_gpu_posecov.py names
    for name, d in res.items():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (name, d)
        assert d.get("group_segment_fixed_size", 0) == 0, name  # all LDS is dynamic: sized by the launcher ...
    # ... to ceil(N/64) tile rows of 22 doubles + 86: at the largest row within the 64 KiB a launch gets without opting in (160 KiB per CU)
    assert (-(-posecov.MAX_POINTS // 64) * 22 + 86) * 8 <= 64 * 1024


def test_python_surface_errors():
    from lc_amd import inference, posecov
    from lc_amd.config import AttrDict

    with pytest.raises(KeyError, match="bbox_3d.*test blob"):
        inference.solve_pnp_with_cov(AttrDict(solvers=["weighted"]), {}, {})
    with pytest.raises(KeyError, match="bbox_3d"):
        inference.GraphedSolvePnP(AttrDict(solvers=["weighted"]), {}, {}, with_cov=True)
    B, N = 2, 8
    K, X, U, W, pose, bbox = torch.zeros(B, 3, 3), torch.zeros(B, N, 3), torch.zeros(B, N, 2), torch.ones(B, N, 2), torch.zeros(B, 7), torch.zeros(B, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        posecov.pose_covariance(K, X, U, W, pose, bbox_3d=bbox)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        posecov.pose_covariance(K.numpy(), X, U, W, pose, bbox_3d=bbox)
    with pytest.raises(TypeError):
        posecov.pose_covariance(K, X, U, W, pose)  # bbox_3d is required
