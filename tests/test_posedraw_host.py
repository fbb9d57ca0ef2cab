"""The posedraw library and the scene poses' contract without a GPU (lc_amd/csrc/posedraw/, include/lc_amd_posedraw.h, lc_amd/posedraw.py,
lc_amd/synthscene.py): the library's place in the registry, header = exports = ctypes table, what the compiler made of the kernel, the
refusals of the entry point reached with host pointers (nothing launches), every refusal of the wrappers, and on tests/posedraw_cases.py
the properties of the host statement -- each derivable, none measured -- with the assertions that the list reaches every branch."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import posedraw_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_is_the_sixth_of_the_third_tuple_and_of_no_other():
    import __graft_entry__ as entry
    from lc_amd import build, posedraw

    T = build.POSEDRAW
    assert build.EXTRA_TARGETS[:6] == (build.SHADE, build.OBOX, build.SYMFIND, build.TEXTURE, build.SAMPLER, T) and T not in build.TARGETS + build.LATER_TARGETS
    assert T == build._side("posedraw", (build.KEYED_HASH_H,))
    assert T.src_dir == os.path.join(build.CSRC, "posedraw") and T.header == "lc_amd_posedraw.h" and T.hash_marker == b"LC_AMD_POSEDRAW_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_posedraw.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_posedraw.so " in doc and "lc_amd/csrc/posedraw/ " in doc and "include/lc_amd_posedraw.h " in doc
    entry.build()
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = posedraw.load()
    assert lib.lc_amd_posedraw_version() == 1
    assert lib.lc_amd_posedraw_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    every = build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS
    assert every.count(T) == 1 and len({t.so_path for t in every}) == len({t.hash_marker for t in every}) == len({build.source_hash(t) for t in every}) == len(every)
    for other in every:  # no other library sees this one's files or carries its marker, and the reverse
        if other is T:
            continue
        assert not any("posedraw" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    own = {os.path.join(T.src_dir, "lc_posedraw.hip"), os.path.join(ROOT, "include", T.header)}
    assert {os.path.normpath(d) for d in build._deps(T)} == own | {build.KEYED_HASH_H}
    assert not any("shade" in os.path.basename(d) for d in own)
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_posedraw.h", "../shared/lc_keyed_hash.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_POSEDRAW_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomic" not in code and "hipMalloc" not in code and "hipMemset" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert "__shared__" not in code and code.count("hipLaunchKernelGGL") == 1 and "fmix32(unsigned" not in code  # the shared hash is used, not restated
    # every fp64 operation the contract rounds is a call: no bare product, sum or quotient of doubles in the kernel, and no library sine, cosine or sqrt
    kernel = code[code.index("cos_sin_turns(double x"):code.index("bool misaligned")]
    assert not re.search(r"\b(sin|cos|sincos|sqrt|fma)\s*\(", kernel) and "__dsqrt_rn" in kernel


def test_header_exports_and_the_ctypes_table_agree():
    from lc_amd import augment, build, posedraw, sampler

    T = build.POSEDRAW
    posedraw.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(posedraw._SIGNATURES) and "lc_posedraw_scenes_f32" in declared and len(declared) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared

    def define(name):
        return int(re.search(rf"#define {name} (\w+)", header).group(1), 0)

    assert define("LC_AMD_POSEDRAW_VERSION") == 1
    assert (posedraw.MAX_INSTANCES, posedraw.TRIES, posedraw.MAX_SCENES) == tuple(define("LC_POSEDRAW_" + n) for n in ("MAX_INSTANCES", "TRIES", "MAX_SCENES")) == (64, 64, 2 ** 20)
    # the next free op code after the sampler's two
    assert posedraw.OP_POSE == define("LC_POSEDRAW_OP_POSE") == max(sampler.OP_SPARE, sampler.OP_PERM) + 1 == augment.OP_HOST + 16
    assert ((posedraw.MAX_INSTANCES - 1) * posedraw.TRIES + posedraw.TRIES - 1) * 8 + 7 < 2 ** 31
    m = re.search(r"int lc_posedraw_scenes_f32\((.*?)\);", text, flags=re.S)
    kinds = ["p" if "*" in a else {"int": "i", "double": "d"}[a.split()[0]] for a in m.group(1).split(",")]
    res, args = posedraw._SIGNATURES["lc_posedraw_scenes_f32"]
    assert res is ctypes.c_int and kinds == [{ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_double: "d"}[a] for a in args], kinds


def test_one_kernel_of_one_wavefront_without_lds_scratch_or_spills(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, posedraw

    posedraw.load()
    res = kernel_resources(build.POSEDRAW.so_path)
    assert len(res) == 1, sorted(res)
    (name, d), = res.items()
    with capsys.disabled():
        print(f"\n{name}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs, {d.get('group_segment_fixed_size', 0)} B of LDS", end="")
    assert "lc_posedraw_scenes_kernel" in name and d["max_flat_workgroup_size"] == 64 and d.get("group_segment_fixed_size", 0) == 0
    assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0


def test_the_entry_point_checks_its_arguments_before_launching():
    from lc_amd import posedraw

    lib = posedraw.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_posedraw_last_error
    names = ("seed", "scene_id", "mesh_index", "radius", "cam_K", "R", "t", "tries", "info", "mesh_index_out")

    def call(z=(0.5, 1.0), box=(0.0, 0.0, 64.0, 48.0), gap=0.0, near=0.01, n_meshes=2, K_stride=9, S=2, M=3, **ptrs):
        a = {n: ptrs.get(n, p) for n in names}
        return lib.lc_posedraw_scenes_f32(*z, *box, gap, near, a["seed"], a["scene_id"], a["mesh_index"], a["radius"], n_meshes, a["cam_K"], K_stride, S, M,
                                          a["R"], a["t"], a["tries"], a["info"], a["mesh_index_out"], None)

    assert call(S=0) == 0  # nothing is launched
    assert call(S=-1) == 1 and call(S=2 ** 20 + 1) == 1 and b"0 <= S <= 1048576" in msg()
    assert call(M=0) == 1 and call(M=65) == 1 and b"1 <= M <= 64, got 65" in msg()
    assert call(S=0, M=65) == 1
    assert call(n_meshes=0) == 1 and b"n_meshes >= 1" in msg()
    for n in names:
        assert call(**{n: None}) == 2, n
        assert call(**{n: p + (4 if n == "seed" else 2)}) == 7, n
    assert call(z=(np.nan, 1.0)) == 3 and call(near=np.inf) == 3 and call(box=(0.0, 0.0, np.inf, 1.0)) == 3 and b"must be finite" in msg()
    assert call(z=(1.0, 0.5)) == 4 and b"z_min <= z_max" in msg()
    assert call(box=(1.0, 0.0, 0.5, 1.0)) == 4 and call(box=(0.0, 2.0, 1.0, 1.0)) == 4 and b"x0 <= x1 and y0 <= y1" in msg()
    assert call(gap=-1e-9) == 5 and b"gap >= 0" in msg()
    assert call(K_stride=3) == 6 and b"K_stride must be 0" in msg()


def test_the_host_function_s_refusals():
    from lc_amd.posedraw import PoseDrawConfig, draw_scene_poses_host

    c = cases.build("s3-m2")
    good = dict(cfg=c.cfg, seed=c.seed, scene_ids=c.scene_ids, mesh_index=c.mesh_index, radius=c.radius, cam_K=c.cam_K)

    def bad(error, match, **change):
        with pytest.raises(error, match=match):
            draw_scene_poses_host(**{**good, **change})

    def cfg(**change):
        return PoseDrawConfig(**{**dict(z_range=(0.5, 1.0), centre_box=(0.0, 0.0, 64.0, 48.0), gap=0.0, near=0.01), **change})

    bad(TypeError, "cfg must be a PoseDrawConfig", cfg=None)
    bad(ValueError, "z_range is a pair", cfg=cfg(z_range=(0.5, 1.0, 2.0)))
    bad(ValueError, "z_min <= z_max", cfg=cfg(z_range=(1.0, 0.5)))
    bad(ValueError, "z_range must be finite", cfg=cfg(z_range=(0.5, np.inf)))
    bad(TypeError, "z_range must hold numbers", cfg=cfg(z_range=("a", 1.0)))
    bad(ValueError, r"centre_box is \(x0, y0, x1, y1\)", cfg=cfg(centre_box=(0.0, 0.0, 1.0)))
    bad(ValueError, "centre_box .* is empty", cfg=cfg(centre_box=(2.0, 0.0, 1.0, 1.0)))
    bad(ValueError, "centre_box .* is empty", cfg=cfg(centre_box=(0.0, 2.0, 1.0, 1.0)))
    bad(ValueError, "centre_box must be finite", cfg=cfg(centre_box=(0.0, 0.0, np.nan, 1.0)))
    bad(ValueError, "gap must not be negative", cfg=cfg(gap=-0.001))
    bad(ValueError, "near must be finite", cfg=cfg(near=np.nan))
    bad(TypeError, "gap must hold numbers", cfg=cfg(gap=True))
    bad(TypeError, "seed must be a whole number", seed=1.5)
    bad(ValueError, "seed of 0 to", seed=2 ** 64)
    bad(TypeError, "scene_ids must be int32", scene_ids=c.scene_ids.astype(np.int64))
    bad(TypeError, "mesh_index must be int32", mesh_index=c.mesh_index.astype(np.int64))
    bad(TypeError, "radius must be float32", radius=c.radius.astype(np.float64))
    bad(ValueError, r"scene_ids has shape \(3, 1\)", scene_ids=c.scene_ids[:, None])
    bad(ValueError, r"mesh_index has shape \(2, 2\), expected \(3, M\)", mesh_index=c.mesh_index[:2])
    bad(ValueError, "1 to 64 slots per scene, got M = 65", mesh_index=np.zeros((3, 65), np.int32))
    bad(ValueError, "1 to 64 slots per scene, got M = 0", mesh_index=np.zeros((3, 0), np.int32))
    bad(ValueError, "radius must be finite and not negative", radius=np.array([0.1, -0.1, 0.1], np.float32))
    bad(ValueError, "radius must be finite and not negative", radius=np.array([0.1, np.inf, 0.1], np.float32))
    bad(ValueError, r"radius has shape \(0,\)", radius=np.zeros(0, np.float32))
    bad(ValueError, r"cam_K has shape \(2, 3, 3\)", cam_K=np.stack((c.cam_K, c.cam_K)))
    # the edges that are NOT refused: an empty z range, a box that is a line, a zero gap
    draw_scene_poses_host(**{**good, "cfg": cfg(z_range=(0.7, 0.7), centre_box=(3.0, 0.0, 3.0, 48.0))})


def test_the_device_wrappers_refusals():
    from lc_amd import posedraw, synthscene
    from lc_amd.posedraw import PoseDrawConfig

    c = cases.build("s3-m2")
    good = dict(seed=c.seed, scene_id=torch.from_numpy(c.scene_ids), mesh_index=torch.from_numpy(c.mesh_index), radius=torch.from_numpy(c.radius),
                cam_K=torch.from_numpy(c.cam_K))

    def bad(error, match, cfg=c.cfg, **change):
        with pytest.raises(error, match=match):
            posedraw.draw_scene_poses(cfg, **{**good, **change})

    bad(TypeError, "cfg must be a PoseDrawConfig", cfg={})
    bad(ValueError, "z_min <= z_max", cfg=PoseDrawConfig(z_range=(2.0, 1.0), centre_box=(0.0, 0.0, 1.0, 1.0)))
    bad(ValueError, "is empty", cfg=PoseDrawConfig(z_range=(1.0, 2.0), centre_box=(0.0, 3.0, 1.0, 1.0)))
    bad(TypeError, "scene_id must be a torch.Tensor", scene_id=c.scene_ids)
    bad(TypeError, "scene_id must be int32", scene_id=good["scene_id"].long())
    bad(ValueError, r"scene_id has shape \(3, 1\)", scene_id=good["scene_id"][:, None])
    bad(TypeError, "mesh_index must be int32", mesh_index=good["mesh_index"].long())
    bad(ValueError, r"mesh_index has shape \(2, 2\), expected \(3, \*\)", mesh_index=good["mesh_index"][:2])
    bad(ValueError, "1 to 64 slots per scene, got M = 65", mesh_index=torch.zeros(3, 65, dtype=torch.int32))
    bad(TypeError, "radius must be float32", radius=good["radius"].double())
    bad(ValueError, r"radius has shape \(3, 1\)", radius=good["radius"][:, None])
    bad(ValueError, "at least one", radius=good["radius"][:0])
    bad(TypeError, "cam_K must be float32", cam_K=good["cam_K"].double())
    bad(ValueError, r"cam_K has shape \(2, 3, 3\), expected \(3, 3, 3\)", cam_K=good["cam_K"].expand(2, 3, 3))
    bad(TypeError, "seed must be a whole number", seed=0.5)
    bad(ValueError, "seed of 0 to", seed=-1)
    bad(TypeError, "a seed tensor holds one uint64 or int64 element", seed=torch.zeros(2, dtype=torch.int64))
    bad(TypeError, "a seed tensor holds one", seed=torch.zeros(1, dtype=torch.int32))
    bad(RuntimeError, "scene_id is on cpu; the HIP path needs tensors on the MI355X")  # no CPU fallback
    with pytest.raises(TypeError, match="lc_amd.synthscene: meshes must be a MeshSet"):
        synthscene.synth_scenes(None, None, good["radius"], c.cfg, frame_hw=(48, 64), near=0.01, far=6.5, light=(0, 0, 0), phong=(1, 0, 0), delta=0.015,
                                **{k: v for k, v in good.items() if k != "radius"})


def test_the_argument_of_the_polynomial_is_still_exactly_reducible():
    """cos_sin_turns(x) takes the angle 4 pi x and reduces tau = 2 x exactly for x = n / 2^24.  At x = u / 2 = n / 2^25 every step of the
    reduction is still exact (checked in rational arithmetic at the edges of every octant and on random n), and the result is (cos, sin)
    of 2 pi u to a few fp64 ulps."""
    from lc_amd.geometry import cos_sin_turns

    rng = np.random.default_rng(5)
    edges = [o * 2 ** 21 + d for o in range(8) for d in (-1, 0, 1)] + [2 ** 24 - 1, 2 ** 24 - 2, 1, 2, 3]
    ns = np.array(sorted({n for n in edges if 0 <= n < 2 ** 24} | set(rng.integers(0, 2 ** 24, 2000).tolist())), dtype=np.int64)
    for n in ns.tolist():
        x = (n / 2.0 ** 24) * 0.5
        assert Fraction(x) == Fraction(n, 2 ** 25)
        tau = 2.0 * x
        f = tau - np.floor(tau)
        f8 = 8.0 * f
        o = np.floor(f8)
        g = f8 - o
        assert Fraction(tau) == Fraction(n, 2 ** 24) and Fraction(f) == Fraction(tau) and Fraction(float(f8)) == 8 * Fraction(n, 2 ** 24)
        assert Fraction(float(g)) == Fraction(float(f8)) - int(o) and Fraction(float(1.0 - g)) == 1 - Fraction(float(g))
    u = ns / 2.0 ** 24
    c, s = cos_sin_turns(u * 0.5)
    assert np.abs(c - np.cos(2 * np.pi * u)).max() <= 2 ** -50 and np.abs(s - np.sin(2 * np.pi * u)).max() <= 2 ** -50
    c0, s0 = cos_sin_turns(np.array([0.0, 0.125, 0.25, 0.375]))  # u = 0, 1/4, 1/2, 3/4: the axes, exactly
    assert c0.tolist() == [1.0, 0.0, -1.0, 0.0] and s0.tolist() == [0.0, 1.0, 0.0, -1.0]


def test_the_case_list_reaches_every_branch():
    from lc_amd import posedraw

    for name in ("s3-m1", "s3-m2", "s3-m64", "one"):
        r, _ = cases.reference(name)
        assert not r.info.any() and not r.tries.any(), name  # radii small enough that every slot is placed at try 0
    assert cases.build("s3-m64").mesh_index.shape == (3, posedraw.MAX_INSTANCES)
    r, _ = cases.reference("crowded")
    assert ((r.info == 0) & (r.tries > 0)).any() and (r.info == -1).any() and (r.tries[r.info == -1] == posedraw.TRIES).all()
    after = [(s, m) for s in range(3) for m in range(1, 8) if r.info[s, m] == 0 and (r.info[s, :m] == -1).any()]
    assert after, "a slot behind a slot without room is still placed"
    big = cases.build("crowded").mesh_index == 0
    assert any(big[s, m] and r.tries[s, m] > 0 for s, m in after)  # and not only because it is small: it had to avoid the placed ones
    r, _ = cases.reference("refusals")
    c = cases.build("refusals")
    assert r.info[0].tolist() == [0, -3, 0, -2, -2, -2]  # an empty slot between filled ones, unknown meshes on both sides, the near plane
    assert r.info[1].tolist() == [-3, -3, 0, 0, -3, 0]
    assert (r.info[2] == -2).all() and (r.info[3] == -2).all() and r.info[4].tolist() == [-2] * 5 + [-3]  # the cameras; an empty slot stays empty
    assert np.isinf(c.cam_K[2]).any() and c.cam_K[3, 1, 1] == 0 and np.isnan(c.cam_K[4]).any()
    assert float(c.cfg.z_range[0]) - float(c.radius[2]) <= c.cfg.near < float(c.cfg.z_range[0]) - float(c.radius[0])
    assert len(set(cases.build("mixed-radii").radius.tolist())) == 5
    z = cases.build("flat-z").cfg.z_range
    assert z[0] == z[1] and (cases.reference("flat-z")[0].tries > 0).any()
    x0, y0, x1, y1 = cases.build("big-box").cfg.centre_box
    assert x0 < 0 and y0 < 0 and x1 > cases.FRAME[1] and y1 > cases.FRAME[0]
    ids = cases.build("ids").scene_ids.tolist()
    assert ids[0] == ids[3] and ids[2] < 0 and sorted(set(ids)) != list(range(min(ids), min(ids) + len(set(ids))))
    assert cases.build("seed-high").seed >> 32 and cases.build("cam-bop").seed >> 32
    for name in ("cam-bop", "cam-stress"):
        K = cases.build(name).cam_K
        assert K[0, 0] != K[1, 1] and (K[0, 1] != 0) == (name == "cam-stress") and K[1, 0] == 0


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_host_statement_s_properties(name):
    from lc_amd import posedraw

    c = cases.build(name)
    (R, t, tries, info, out), pos = cases.reference(name)
    S, M = c.mesh_index.shape
    assert R.shape == (S, M, 3, 3) and t.shape == (S, M, 3) and R.dtype == t.dtype == np.float32
    assert tries.shape == info.shape == out.shape == (S, M) and tries.dtype == info.dtype == out.dtype == np.int32
    placed = info == 0
    assert np.isin(info, (0, -1, -2, -3)).all() and ((info == -3) == (c.mesh_index == -1)).all()
    assert np.array_equal(out, np.where(placed, c.mesh_index, -1)) and not R[~placed].any() and not t[~placed].any()
    assert ((tries >= 0) & (tries < posedraw.TRIES))[placed].all() and (tries[info == -1] == posedraw.TRIES).all() and not tries[info < -1].any()
    assert np.array_equal(t[placed], pos[placed].astype(np.float32)) and np.isnan(pos[~placed]).all()
    if not placed.any():
        return
    R64 = R[placed].astype(np.float64)
    assert np.abs(np.swapaxes(R64, 1, 2) @ R64 - np.eye(3)).max() <= 1e-6 and (np.linalg.det(R64) > 0).all()
    # Shoemake's formula by libm: the polynomial's fp64 error lies far below an fp32 half-ulp, so only a rounding tie can differ, by one
    # ulp of an entry of size at most 1
    s_of, m_of = np.nonzero(placed)
    libm = posedraw.shoemake_libm(*posedraw.rotation_draws(c.seed, c.scene_ids[s_of], m_of))
    assert np.abs(R64 - libm.astype(np.float32).astype(np.float64)).max() <= 2.0 ** -23
    assert np.abs(posedraw.shoemake(*posedraw.rotation_draws(c.seed, c.scene_ids[s_of], m_of)) - libm).max() <= 2.0 ** -48
    # every placed origin projects into the box and lies in the depth range, up to one fp32 rounding of t (and fp64's own of the check)
    K = np.broadcast_to(c.cam_K, (S, 3, 3)).astype(np.float64)[s_of]
    p = np.einsum("nij,nj->ni", K, pos[placed])
    x, y, z = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], pos[placed][:, 2]
    x0, y0, x1, y1 = c.cfg.centre_box
    eps = 1e-9 * max(1.0, abs(x0), abs(x1), abs(y0), abs(y1))
    assert (x >= x0 - eps).all() and (x <= x1 + eps).all() and (y >= y0 - eps).all() and (y <= y1 + eps).all()
    assert (z >= c.cfg.z_range[0]).all() and (z <= c.cfg.z_range[1]).all()
    z32 = t[placed][:, 2].astype(np.float64)
    assert (z32 >= c.cfg.z_range[0] * (1 - 2.0 ** -24)).all() and (z32 <= c.cfg.z_range[1] * (1 + 2.0 ** -24)).all()
    # t32 = t (1 + e), |e| <= 2^-24 per entry: xn and yn move by at most 2^-23 (1 + 2^-23) of themselves, px by |K00 dxn| + |K01 dyn|, py by |K11 dyn|
    t32 = t[placed].astype(np.float64)
    p32 = np.einsum("nij,nj->ni", K, t32)
    xn, yn = pos[placed][:, 0] / z, pos[placed][:, 1] / z
    tol_x = 2.0 ** -23 * 1.01 * (np.abs(K[:, 0, 0] * xn) + np.abs(K[:, 0, 1] * yn)) + eps
    tol_y = 2.0 ** -23 * 1.01 * np.abs(K[:, 1, 1] * yn) + eps
    x32, y32 = p32[:, 0] / p32[:, 2], p32[:, 1] / p32[:, 2]
    assert (x32 >= x0 - tol_x).all() and (x32 <= x1 + tol_x).all() and (y32 >= y0 - tol_y).all() and (y32 <= y1 + tol_y).all()
    # every pair of placed spheres of a scene satisfies the contract's own fp64 test
    r64 = c.radius.astype(np.float64)
    for s in range(S):
        ms = np.nonzero(placed[s])[0]
        for a in range(len(ms)):
            for b in range(a):
                d = pos[s, ms[a]] - pos[s, ms[b]]
                sep = (r64[c.mesh_index[s, ms[a]]] + r64[c.mesh_index[s, ms[b]]]) + c.cfg.gap
                assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] >= sep * sep, (name, s, ms[a], ms[b])
            # and the tries before the taken one were not good: the lowest good try is the one taken
            cand = posedraw.candidates(posedraw._config(c.cfg), c.seed, c.scene_ids[s], int(ms[a]), np.broadcast_to(c.cam_K, (S, 3, 3))[s].astype(np.float64))
            assert np.array_equal(cand[tries[s, ms[a]]], pos[s, ms[a]])
            for k in range(tries[s, ms[a]]):
                hit = False
                for b in range(a):
                    d = cand[k] - pos[s, ms[b]]
                    sep = (r64[c.mesh_index[s, ms[a]]] + r64[c.mesh_index[s, ms[b]]]) + c.cfg.gap
                    hit = hit or (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] < sep * sep
                assert hit, (name, s, ms[a], k)


def test_a_scene_does_not_depend_on_the_batch_and_depends_on_the_seed():
    from lc_amd.posedraw import draw_scene_poses_host

    for name in ("ids", "crowded", "refusals", "s3-m64"):
        c = cases.build(name)
        whole, _ = cases.reference(name)
        per_scene = c.cam_K.ndim == 3
        for s in range(len(c.scene_ids)):  # alone, and in another position among other scenes
            alone = draw_scene_poses_host(c.cfg, c.seed, c.scene_ids[s:s + 1], c.mesh_index[s:s + 1], c.radius, c.cam_K[s:s + 1] if per_scene else c.cam_K)
            for got, want in zip(alone, whole):
                assert np.array_equal(got[0].view(np.int32), want[s].view(np.int32)), (name, s)
        order = np.arange(len(c.scene_ids))[::-1].copy()
        rev = draw_scene_poses_host(c.cfg, c.seed, c.scene_ids[order], c.mesh_index[order], c.radius, c.cam_K[order] if per_scene else c.cam_K)
        for got, want in zip(rev, whole):
            assert np.array_equal(got.view(np.int32), want[order].view(np.int32)), name
    whole, _ = cases.reference("ids")
    for part in whole:  # the repeated scene id: the same scene in two batch positions
        assert np.array_equal(part[0].view(np.int32), part[3].view(np.int32))
    assert not np.array_equal(whole.R[0], whole.R[1]) and not np.array_equal(whole.t[0], whole.t[2])
    for name in ("ids", "seed-high", "cam-bop"):
        a, b = cases.reference(name)[0], cases.reference(name, 1)[0]
        assert not np.array_equal(a.R, b.R) and not np.array_equal(a.t, b.t), name
    c = cases.build("seed-high")  # the upper half counts
    low = draw_scene_poses_host(c.cfg, c.seed % 2 ** 32, c.scene_ids, c.mesh_index, c.radius, c.cam_K)
    assert not np.array_equal(low.R, cases.reference("seed-high")[0].R)


def test_mesh_radii_hold_every_vertex_and_round_up():
    from lc_amd.posedraw import mesh_radii
    from tests import render_cases

    meshes = [render_cases.box(), render_cases.icosphere(0, 0.1), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
              (np.array([[3.0, 4.0, 0.0]], np.float32), np.zeros((0, 3), np.int32))]
    r = mesh_radii(meshes)
    assert r.dtype == np.float32 and r.shape == (4,) and r[2] == 0 and r[3] == np.nextafter(np.float32(5.0), np.float32(6.0))
    for (v, _), rk in zip(meshes, r):
        if len(v):
            n = np.sqrt((v.astype(np.float64) ** 2).sum(1)).max()
            assert float(rk) >= n and float(rk) <= n * (1 + 2.0 ** -22)
