"""The shading library without a GPU (lc_amd/csrc/shade/, include/lc_amd_shade.h, lc_amd/shade.py): its place in the registry, header =
exports = ctypes table, its source hash, what the compiler made of the two kernels, every host refusal of the two entry points reached with
host pointers (nothing launches), the wrappers' refusals, `vertex_normals`, the oracle's properties, its planted mistakes, and the two
conditions (and the end-to-end cases' tie cap) that tests/test_gpu_shade.py relies on."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOURTEEN = ["main", "optim", "posecov", "render", "crop", "models", "symerr", "vsd", "gtinfo", "maskcrop", "augment", "rle", "geometry", "bgstore"]


def test_the_library_stands_in_the_third_tuple_behind_the_fourteen():
    import __graft_entry__ as entry
    from lc_amd import build, shade

    T = build.SHADE
    before = build.TARGETS + build.LATER_TARGETS
    assert [t.name for t in before] == FOURTEEN and T in build.EXTRA_TARGETS and T not in before  # (the tuple's length is the next library's business)
    every = before + build.EXTRA_TARGETS
    assert every.index(T) >= len(FOURTEEN)
    assert T == build._side("shade") and T.shared == ()
    assert T.src_dir == os.path.join(build.CSRC, "shade") and T.header == "lc_amd_shade.h" and T.hash_marker == b"LC_AMD_SHADE_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_shade.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_shade.so " in doc and "lc_amd/csrc/shade/ " in doc and "include/lc_amd_shade.h " in doc
    entry.build()
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = shade.load()
    assert lib.lc_amd_shade_version() == 1
    assert lib.lc_amd_shade_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert len({build.source_hash(t) for t in every}) == len({t.so_path for t in every}) == len({t.hash_marker for t in every}) == len(every)
    for other in every:  # no other library sees this one's directory or header, or carries its marker, and the reverse
        if other is T:
            continue
        assert not any("shade" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    # the hash covers the library's own two files and nothing of csrc/shared/
    assert {os.path.normpath(d) for d in build._deps(T)} == {os.path.join(T.src_dir, "lc_shade.hip"), os.path.join(ROOT, "include", T.header)}
    assert build.sources(T) == [os.path.join(T.src_dir, "lc_shade.hip")]
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_shade.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_SHADE_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert len(os.listdir(build.SHARED)) == 6
    # the walkers of "all libraries" walk the third tuple too
    assert "build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS" in open(os.path.join(ROOT, "scripts", "isa_identity.py")).read()
    assert build.build_later.__doc__ and "EXTRA_TARGETS" in build.build_later.__doc__


def test_header_exports_and_the_ctypes_table_agree():
    from lc_amd import build, render, shade

    T = build.SHADE
    shade.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(shade._SIGNATURES) and {"lc_shade_instances_u8", "lc_shade_scene_u8"} <= declared and len(declared) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert int(re.search(r"#define LC_AMD_SHADE_VERSION (\d+)", header).group(1)) == 1
    assert shade.MAX_SIZE == render.MAX_SIZE == int(re.search(r"#define LC_SHADE_MAX_SIZE (\d+)", header).group(1))
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f"}
    for name in ("lc_shade_instances_u8", "lc_shade_scene_u8"):
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "float": "f"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = shade._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)
    assert shade.DEFAULT_LIGHT == (400.0, -400.0, -400.0) and shade.DEFAULT_PHONG == (0.4, 0.8, 0.3)


def test_two_kernels_without_scratch_spills_or_lds(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, shade

    shade.load()
    res = kernel_resources(build.SHADE.so_path)
    assert len(res) == 2, sorted(res)
    for short in ("lc_shade_instances_kernel", "lc_shade_scene_kernel"):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == 256 and d.get("group_segment_fixed_size", 0) == 0, short


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import shade

    lib = shade.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_shade_last_error
    mesh = dict(verts=p, normals=p, colors=p, faces=p, table=p, n_meshes=2, total_verts=5, total_faces=4)
    rows = dict(mesh_index=p, R=p, t=p, K=p, light=p, phong=p, face=p)

    def inst(B=2, h=16, w=20, cx=0.5, cy=0.5, out=p, info=p, **kw):
        a = {**mesh, **rows, **kw}
        return lib.lc_shade_instances_u8(a["verts"], a["normals"], a["colors"], a["faces"], a["table"], a["n_meshes"], a["total_verts"], a["total_faces"],
                                         a["mesh_index"], a["R"], a["t"], a["K"], a["light"], a["phong"], a["face"], B, h, w, cx, cy, out, info, None)

    def scene(B=2, h=16, w=20, cx=0.5, cy=0.5, scene_index=p, origin=p, instance=p, frames=p, S=2, H=24, W=32, info=p, **kw):
        a = {**mesh, **rows, **kw}
        return lib.lc_shade_scene_u8(a["verts"], a["normals"], a["colors"], a["faces"], a["table"], a["n_meshes"], a["total_verts"], a["total_faces"],
                                     a["mesh_index"], scene_index, a["R"], a["t"], a["K"], a["light"], a["phong"], a["face"], origin, B, h, w, cx, cy, instance,
                                     frames, S, H, W, info, None)

    nothing = {k: None for k in ("verts", "normals", "colors", "faces", "table", *rows)}
    for fn, name in ((inst, b"lc_shade_instances_u8: "), (scene, b"lc_shade_scene_u8: ")):
        assert fn(B=-1) != 0 and name + b"B < 0" in msg()
        assert fn(B=0) == 0 and fn(B=0, info=None, **nothing) == 0
        assert fn(n_meshes=0) != 0 and name + b"n_meshes < 1" in msg()
        for k in ("total_verts", "total_faces"):
            assert fn(**{k: -1}) != 0 and b"total_verts < 0 or total_faces < 0" in msg(), k
        assert fn(table=None) != 0 and b"mesh_table must not be NULL" in msg()
        for k in ("verts", "normals", "colors"):
            assert fn(**{k: None}) != 0 and b"verts, normals and colors must not be NULL where total_verts > 0" in msg(), k
            assert fn(**{k: None}, total_verts=0, h=0) != 0 and b"h and w must be in" in msg(), k  # (passed the NULL rule)
        assert fn(faces=None) != 0 and b"faces must not be NULL where total_faces > 0" in msg()
        for k in rows:
            assert fn(**{k: None}) != 0 and b"mesh_index, R, t, K, light, phong and face must not be NULL" in msg(), k
        assert fn(info=None) != 0 and b"info must not be NULL" in msg()
        for bad in ((0, 20), (16, 0), (16385, 20), (16, 16385), (-1, 20)):
            assert fn(h=bad[0], w=bad[1]) != 0 and b"h and w must be in [1, 16384], got" in msg(), bad
        for bad in ((0.501, 0.5), (0.5, 64.5), (float("nan"), 0.5), (-65.0, 0.0)):
            assert fn(cx=bad[0], cy=bad[1]) != 0 and b"cx and cy must be multiples of 2^-8 in [-64, 64]" in msg(), bad
        for k in ("verts", "normals", "faces", "table"):
            assert fn(**{k: p + 2}) != 0 and b"verts, normals, faces and mesh_table must be aligned to 4 bytes" in msg(), k
        for k in rows:
            assert fn(**{k: p + 2}) != 0 and b"aligned to 4 bytes" in msg(), k
        assert fn(info=p + 2) != 0 and b"aligned to 4 bytes" in msg()
    assert inst(out=None) != 0 and b"out must not be NULL" in msg()
    assert scene(S=0) != 0 and b"S < 1" in msg()
    for k in ("scene_index", "instance", "frames"):
        assert scene(**{k: None}) != 0 and b"scene_index, instance and frames must not be NULL" in msg(), k
    for bad in ((0, 32), (24, 0), (16385, 32), (24, 16385)):
        assert scene(H=bad[0], W=bad[1]) != 0 and b"H and W must be in [1, 16384], got" in msg(), bad
    assert scene(origin=None) != 0 and b"without origin_xy the maps must have the frame's size" in msg()
    for k in ("scene_index", "instance", "origin"):
        assert scene(**{k: p + 2}) != 0 and b"scene_index, instance and origin_xy must be aligned to 4 bytes" in msg(), k


def _host_set(meshes):
    """A MeshSet stand-in on the host: refusals only."""
    from lc_amd.render import MeshSet

    ms = MeshSet.__new__(MeshSet)
    table, vo, fo = [], 0, 0
    for v, f in meshes:
        table.append((vo, len(v), fo, len(f)))
        vo, fo = vo + len(v), fo + len(f)
    ms.n_meshes, ms.total_verts, ms.total_faces, ms.table_host = len(meshes), vo, fo, np.asarray(table, np.int32)
    ms.verts = torch.from_numpy(np.concatenate([np.asarray(v, np.float32) for v, _ in meshes]))
    ms.faces = torch.from_numpy(np.concatenate([np.asarray(f, np.int32) for _, f in meshes]))
    ms.table, ms.device = torch.from_numpy(ms.table_host), torch.device("cpu")
    return ms


def test_wrapper_refusals():
    from lc_amd import shade
    from tests import shade_cases as cases

    ms = _host_set([cases.ICO, cases.QUAD])
    with pytest.raises(TypeError, match="meshes must be a MeshSet"):
        shade.Appearance([cases.ICO])
    with pytest.raises(ValueError, match=r"colors is a list of one \(Nv,3\) array per mesh \(2\)"):
        shade.Appearance(ms, [cases.QUAD_COLORS])
    with pytest.raises(TypeError, match="mesh 1: colors must be uint8, got float32"):
        shade.Appearance(ms, [None, cases.QUAD_COLORS.astype(np.float32)])
    with pytest.raises(ValueError, match=r"mesh 0: colors has shape \(4, 3\), expected \(12, 3\)"):
        shade.Appearance(ms, [cases.QUAD_COLORS, None])
    with pytest.raises(ValueError, match=r"mesh 1: normals has shape \(12, 3\), expected \(4, 3\)"):
        shade.Appearance(ms, None, [None, np.zeros((12, 3))])
    with pytest.raises(TypeError, match="mesh 1: normals must hold floats"):
        shade.Appearance(ms, None, [None, np.zeros((4, 3), np.int32)])
    with pytest.raises(ValueError, match="mesh 1: normals must be finite"):
        shade.Appearance(ms, None, [None, np.full((4, 3), np.nan)])
    ap = shade.Appearance(ms, [None, cases.QUAD_COLORS])
    assert ap.colors.shape == (16, 3) and (ap.colors[:12] == 128).all() and np.array_equal(ap.colors_host[12:], cases.QUAD_COLORS)
    assert np.array_equal(ap.normals_host[:12], shade.vertex_normals(*cases.ICO)) and ap.normals.dtype == torch.float32

    face, mi = torch.full((2, 8, 12), -1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    R, t, K = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.eye(3)

    def call(meshes=ms, appearance=ap, face=face, mesh_index=mi, R=R, t=t, K=K, **kw):
        return shade.shade(meshes, appearance, face, mesh_index, R, t, K, **{"light": shade.DEFAULT_LIGHT, "phong": shade.DEFAULT_PHONG, **kw})

    with pytest.raises(TypeError, match="meshes must be a MeshSet"):
        call(meshes=None)
    with pytest.raises(TypeError, match="appearance must be an Appearance"):
        call(appearance=None)
    with pytest.raises(ValueError, match="appearance was made for another MeshSet"):
        call(meshes=_host_set([cases.ICO, cases.QUAD]))
    with pytest.raises(TypeError, match="lc_amd.shade: face must be int32, got torch.int64"):
        call(face=face.long())
    with pytest.raises(ValueError, match=r"face has shape \(8, 12\)"):
        call(face=face[0])
    with pytest.raises(TypeError, match="mesh_index must be an int32 tensor"):
        call(mesh_index=mi.long())
    with pytest.raises(RuntimeError, match="R is on cpu.*no CPU fallback"):
        call()
    with pytest.raises(TypeError, match="R must be a torch.Tensor"):
        call(R=None)
    for bad in ((1.0, 2.0), "abc", (1.0, 2.0, float("inf")), None):
        with pytest.raises(ValueError, match="light is three finite numbers or a float32 tensor"):
            shade._per_row("light", bad, 2, torch.device("cpu"))
    with pytest.raises(TypeError, match="appearance must be an Appearance"):
        shade.render_color(ms, None, mi, R, t, K, (8, 12), near=0.1, far=2.0, light=shade.DEFAULT_LIGHT, phong=shade.DEFAULT_PHONG)
    with pytest.raises(TypeError, match="appearance must be an Appearance"):
        shade.render_scene(ms, None, mi, mi, R, t, K, (8, 12), 1, near=0.1, far=2.0, light=shade.DEFAULT_LIGHT, phong=shade.DEFAULT_PHONG)


def test_vertex_normals_on_a_cube_and_on_a_degenerate_face():
    from lc_amd.shade import vertex_normals
    from tests import render_cases

    v, f = render_cases.box((0.5, 0.5, 0.5))
    n = vertex_normals(v, f)
    assert n.dtype == np.float32 and n.shape == (8, 3)
    # a corner of a cube meets three faces; each adds its normal once or twice, as the cut of the face into two triangles meets the corner: every
    # component points the corner's way (outward or inward as the faces wind, the same at every corner), with weights 1 or 2 out of the sum
    sign = np.sign((n * v).sum(1))
    assert abs(sign.sum()) == 8 and np.array_equal(np.sign(n) * sign[:, None], np.sign(v))
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-7)
    for row in np.abs(n.astype(np.float64)):
        k = row / row.min()
        assert np.allclose(k, np.rint(k), atol=1e-6) and set(np.rint(k)) <= {1.0, 2.0}, row
    assert np.allclose(np.abs(n[[0, 7]]), 3 ** -0.5, atol=1e-7)  # the two corners every face meets with one triangle... or two: the diagonal
    # a face with a repeated vertex adds a zero cross product; a vertex of no other face stays zero, bit for bit
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    n2 = vertex_normals(v2, np.array([[0, 1, 2], [3, 3, 1]]))
    assert np.array_equal(n2[3], np.zeros(3, np.float32)) and np.array_equal(n2[:3], np.tile(np.float32([0, 0, 1]), (3, 1)))
    assert vertex_normals(v2, np.zeros((0, 3), np.int32)).tolist() == [[0.0] * 3] * 4
    with pytest.raises(ValueError, match=r"face indices must lie in \[0, 4\)"):
        vertex_normals(v2, np.array([[0, 1, 4]]))
    # two faces of opposite winding on the same vertices cancel: zero, not NaN
    assert np.array_equal(vertex_normals(v2, np.array([[0, 1, 2], [0, 2, 1]])), np.zeros((4, 3), np.float32))


def test_the_oracle_interpolates_and_lights_as_stated():
    from tests import shade_cases as cases
    from tests import shade_oracle as oracle

    for name in ("tilted-quad", "ico20", "grid-square"):
        c = cases.build(name)
        ys, xs = np.nonzero(c.face[0] >= 0)
        ambient = np.array([1.0, 0.0, 0.0], np.float32)
        px = oracle.shade_pixels(c.ms, 0, c.R[0], c.t[0], c.K[0], c.light[0], ambient, c.face[0, ys, xs], xs, ys)
        assert px.ok.all() and np.abs((px.lam[:, 0] + px.lam[:, 1]) + px.lam[:, 2] - 1.0).max() <= 2.0 ** -50, name
        assert (px.lam >= -2.0 ** -40).all(), name  # a hit pixel lies inside its face
        assert np.array_equal(px.pre, px.c) and np.array_equal(px.byte, np.rint(px.c).astype(np.uint8)), name  # ka = 1, kd = ks = 0: the interpolated colour itself
        # one colour on every vertex comes back on every hit pixel: the weights sum to 1 within 2^-50, far from the byte's rounding
        grey = c.ms._replace(colors=np.full_like(c.ms.colors, 201))
        assert (oracle.shade_pixels(grey, 0, c.R[0], c.t[0], c.K[0], c.light[0], ambient, c.face[0, ys, xs], xs, ys).byte == 201).all(), name
    # where the stated special values fall: d = 0 behind the surface, a zero normal, a zero light vector
    back, zero, lit = cases.reference("back-facing"), cases.reference("zero-normal"), cases.reference("light-on-surface")
    c = cases.build("back-facing")
    ys, xs = np.nonzero(c.face[0] >= 0)
    only_ambient = oracle.shade_pixels(c.ms, 0, c.R[0], c.t[0], c.K[0], c.light[0], np.float32([0.4, 0.8, 0.0]), c.face[0, ys, xs], xs, ys)
    assert np.array_equal(only_ambient.pre, np.float64(np.float32(0.4)) * only_ambient.c)  # kd d adds exactly nothing
    assert np.isfinite(zero.pre[zero.hit]).all() and np.isfinite(lit.pre[lit.hit]).all() and back.hit.any()
    c = cases.build("light-on-surface")
    assert lit.hit[0, 6, 4] and np.array_equal(lit.pre[0, 6, 4], np.float64(np.float32(0.4)) * oracle.shade_pixels(
        c.ms, 0, c.R[0], c.t[0], c.K[0], c.light[0], c.phong[0], [c.face[0, 6, 4]], [4], [6]).c[0])  # L = 0: d = 0 and s = 0
    sat = cases.reference("saturated")
    assert (sat.pre[sat.hit] > 255).any() and (sat.out[sat.hit][sat.pre[sat.hit] > 255] == 255).all()


def test_the_case_list_keeps_its_two_conditions_and_says_what_it_refuses():
    from tests import shade_cases as cases

    for name in cases.NAMES:
        c = cases.build(name)
        refs = [cases.reference(name)] + ([cases.scene_reference(name)] if c.scene is not None else [])
        for ref in refs:
            pre = ref.pre[ref.hit]
            assert ref.hit.any() and np.isfinite(pre).all(), name
            on_half = (2 * pre == np.rint(2 * pre)) & (pre != np.rint(pre))
            assert c.exact_halves or not on_half.any(), name
            near_half = np.abs(pre - np.floor(pre) - 0.5) < 2.0 ** -20
            assert not (near_half & ~on_half).any(), (name, pre[near_half & ~on_half])
            assert np.array_equal(ref.out[~ref.hit], cases.sentinel(ref.out.shape)[~ref.hit]), name  # misses keep the sentinel
        assert min(r.margin for r in c.renders if r is not None) >= 2.0 ** -30, name
    assert cases.build("grid-square").exact_halves and sum(cases.build(n).exact_halves for n in cases.NAMES) == 1
    ref = cases.reference("grid-square")
    pre = ref.pre[ref.hit]
    assert ((2 * pre == np.rint(2 * pre)) & (pre != np.rint(pre))).sum() >= 10  # halves to tell the two roundings by
    # what each case says about its rows
    assert cases.reference("batch").info.tolist() == [0, 0, -1, 0] and not cases.reference("batch").hit[2].any()
    assert cases.build("batch").ms.table[1][0] == 12  # the quad's vertices lie behind the icosahedron's
    planted = cases.reference("planted-face")
    assert planted.info.tolist() == [1] and planted.hit.sum() == (cases.build("planted-face").face >= 0).sum() - 2  # 20 and 2^30 stay out, and so does -2
    assert cases.scene_reference("scene").info.tolist() == [0, 0, 0, 0] and cases.scene_reference("scene-planted").info.tolist() == [1, 1, 0, 0]
    assert cases.scene_reference("scene-planted").hit.sum() == cases.scene_reference("scene").hit.sum()  # the four planted pixels were misses and stay unwritten
    for name in ("scene", "scene-full"):
        sc = cases.build(name).scene
        assert all((sc.instance == b).sum() > 50 for b in range(4)), name  # every instance shows, so both of each scene overlap and both win somewhere
    org = cases.build("scene").scene.origin_xy
    assert org.min() < 0 and (org[:, 0] + cases.WINDOW[1] > cases.FRAME[1]).any() and (org[:, 1] + cases.WINDOW[0] > cases.FRAME[0]).any()
    # the end-to-end cases: tie pixels, on which the device's rasteriser may choose another face, are at most 2 % of the hit pixels
    for name in cases.END_TO_END:
        c = cases.build(name)
        ties, hits = cases.tie_masks(c).sum(), sum(int(r.mask.sum()) for r in c.renders)
        assert ties <= 0.02 * hits, (name, ties, hits)
        if c.scene is not None:
            assert cases.scene_tie_mask(c).sum() <= 0.02 * (c.scene.instance >= 0).sum(), name


def test_the_scene_form_is_the_instance_form_pasted_by_the_instance_map():
    from tests import shade_cases as cases

    for name in ("scene", "scene-full"):
        c, rows, frames = cases.build(name), cases.reference(name), cases.scene_reference(name)
        sc = c.scene
        want = cases.sentinel(frames.out.shape)
        for s in range(sc.S):
            for Y, X in zip(*np.nonzero(sc.instance[s] >= 0)):
                b = sc.instance[s, Y, X]
                x0, y0 = (0, 0) if sc.origin_xy is None else sc.origin_xy[b]
                want[s, Y, X] = rows.out[b, Y - y0, X - x0]
        assert np.array_equal(frames.out, want), name


def test_every_planted_mistake_changes_the_oracle_s_bytes():
    from tests import shade_cases as cases
    from tests import shade_oracle as oracle

    assert oracle.MISTAKES == ("affine_weights", "normal_not_rotated", "light_in_gl_frame", "round_half_up", "misses_cleared", "vert_off_of_mesh_0")
    changed = {m: [n for n in cases.NAMES if not np.array_equal(cases.shade(cases.build(n), m).out, cases.reference(n).out)] for m in oracle.MISTAKES}
    assert all(changed.values()), changed
    assert "tilted-quad" in changed["affine_weights"] and "grid-square" not in changed["affine_weights"]  # one depth: the two weights agree
    assert changed["round_half_up"] == ["grid-square"]  # the one case that may sit on a half
    assert changed["misses_cleared"] == list(cases.NAMES)
    assert set(changed["vert_off_of_mesh_0"]) == {"batch", "scene", "scene-planted", "scene-full"}  # the cases with a second mesh
    for m in oracle.MISTAKES:  # and the scene form sees each of them too
        hit = [n for n in ("scene", "scene-full") if not np.array_equal(cases.shade_scene(cases.build(n), m).out, cases.scene_reference(n).out)]
        assert hit or m == "round_half_up", m
