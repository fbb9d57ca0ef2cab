"""The textured shading library without a GPU (lc_amd/csrc/texture/, include/lc_amd_texture.h, lc_amd/texture.py): its place in the
registry, header = exports = ctypes table, its source hash, what the compiler made of the three kernels, every host refusal of the three entry
points reached with host pointers (nothing launches), the wrappers' refusals, and `read_ply_textured` on files written here."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("lc_texshade_instances_kernel", "lc_texshade_scene_kernel", "lc_tex_mip_kernel")


def test_the_library_is_the_fourth_of_the_third_tuple_and_of_no_other():
    import __graft_entry__ as entry
    from lc_amd import build, texture

    T = build.TEXTURE
    assert build.EXTRA_TARGETS[:4] == (build.SHADE, build.OBOX, build.SYMFIND, T) and T not in build.TARGETS + build.LATER_TARGETS
    assert T == build._side("texture") and T.shared == ()
    assert T.src_dir == os.path.join(build.CSRC, "texture") and T.header == "lc_amd_texture.h" and T.hash_marker == b"LC_AMD_TEXTURE_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_texture.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_texture.so " in doc and "lc_amd/csrc/texture/ " in doc and "include/lc_amd_texture.h " in doc
    entry.build()
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = texture.load()
    assert lib.lc_amd_texture_version() == 1
    assert lib.lc_amd_texture_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    every = build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS
    assert every.count(T) == 1 and len({t.so_path for t in every}) == len({t.hash_marker for t in every}) == len(every)
    for other in every:  # no other library sees this one's files or carries its marker, and the reverse
        if other is T:
            continue
        assert not any("texture" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    assert {os.path.normpath(d) for d in build._deps(T)} == {os.path.join(T.src_dir, "lc_texture.hip"), os.path.join(ROOT, "include", T.header)}
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_texture.h"}  # no shared header
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_TEXTURE_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert source.count("hipMemsetAsync") == 1 and code.count("hipLaunchKernelGGL") == 2  # one memset and one launch per shading call; the mip launches


def test_header_exports_and_the_ctypes_table_agree():
    from lc_amd import build, shade, texture

    T = build.TEXTURE
    texture.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(texture._SIGNATURES) and {"lc_texshade_instances_u8", "lc_texshade_scene_u8", "lc_tex_build_mips_u8"} <= declared and len(declared) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert int(re.search(r"#define LC_AMD_TEXTURE_VERSION (\d+)", header).group(1)) == 1
    assert texture.TEX_MAX_SIZE == int(re.search(r"#define LC_TEX_MAX_SIZE (\d+)", header).group(1)) == 16384 == texture.MAX_SIZE == shade.MAX_SIZE
    assert texture.TEX_MAX_LEVELS == int(re.search(r"#define LC_TEX_MAX_LEVELS (\d+)", header).group(1)) == (16384).bit_length()
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_longlong: "l"}
    for name in ("lc_texshade_instances_u8", "lc_texshade_scene_u8", "lc_tex_build_mips_u8"):
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else "l" if a.split()[:2] == ["long", "long"] else {"int": "i", "float": "f"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = texture._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)
    for phrase in ("GL_LINEAR_MIPMAP_NEAREST", "no trilinear blend", "no anisotropic", "A NaN\n *       compares false", "+inf selects the last level"):
        assert phrase in header, phrase


def test_three_kernels_without_scratch_spills_or_lds(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, texture

    texture.load()
    res = kernel_resources(build.TEXTURE.so_path)
    assert len(res) == 3, sorted(res)
    for short in KERNELS:
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == 256 and d.get("group_segment_fixed_size", 0) == 0, short


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import texture

    lib = texture.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_texture_last_error
    mesh = dict(verts=p, normals=p, colors=p, faces=p, uv=p, table=p, tex_index=p, n_meshes=2, total_verts=5, total_faces=4, texels=p, tex_table=p, n_tex=1, total_texels=64)
    rows = dict(mesh_index=p, R=p, t=p, K=p, light=p, phong=p, wrap=p, face=p)

    def head(a):
        return (a["verts"], a["normals"], a["colors"], a["faces"], a["uv"], a["table"], a["tex_index"], a["n_meshes"], a["total_verts"], a["total_faces"], a["texels"],
                a["tex_table"], a["n_tex"], a["total_texels"])

    def inst(B=2, h=16, w=20, cx=0.5, cy=0.5, lod=1, out=p, info=p, **kw):
        a = {**mesh, **rows, **kw}
        return lib.lc_texshade_instances_u8(*head(a), a["mesh_index"], a["R"], a["t"], a["K"], a["light"], a["phong"], a["wrap"], a["face"], B, h, w, cx, cy, lod, out, info, None)

    def scene(B=2, h=16, w=20, cx=0.5, cy=0.5, lod=1, scene_index=p, origin=p, instance=p, frames=p, S=2, H=24, W=32, info=p, **kw):
        a = {**mesh, **rows, **kw}
        return lib.lc_texshade_scene_u8(*head(a), a["mesh_index"], scene_index, a["R"], a["t"], a["K"], a["light"], a["phong"], a["wrap"], a["face"], origin, B, h, w, cx, cy,
                                        lod, instance, frames, S, H, W, info, None)

    nothing = {k: None for k in ("verts", "normals", "colors", "faces", "uv", "table", "tex_index", "texels", "tex_table", *rows)}
    for fn, name in ((inst, b"lc_texshade_instances_u8: "), (scene, b"lc_texshade_scene_u8: ")):
        assert fn(B=-1) != 0 and name + b"B < 0" in msg()
        assert fn(B=0) == 0 and fn(B=0, info=None, **nothing) == 0
        assert fn(n_meshes=0) != 0 and name + b"n_meshes < 1" in msg()
        for k in ("total_verts", "total_faces"):
            assert fn(**{k: -1}) != 0 and b"total_verts < 0 or total_faces < 0" in msg(), k
        for k in ("n_tex", "total_texels"):
            assert fn(**{k: -1}) != 0 and b"n_tex < 0 or total_texels < 0" in msg(), k
        for k in ("table", "tex_index"):
            assert fn(**{k: None}) != 0 and b"mesh_table and tex_index must not be NULL" in msg(), k
        for k in ("verts", "normals", "colors"):
            assert fn(**{k: None}) != 0 and b"verts, normals and colors must not be NULL where total_verts > 0" in msg(), k
            assert fn(**{k: None}, total_verts=0, h=0) != 0 and b"h and w must be in" in msg(), k  # (passed the NULL rule)
        for k in ("faces", "uv"):
            assert fn(**{k: None}) != 0 and b"faces and uv must not be NULL where total_faces > 0" in msg(), k
            assert fn(**{k: None}, total_faces=0, h=0) != 0 and b"h and w must be in" in msg(), k
        for k in ("texels", "tex_table"):
            assert fn(**{k: None}) != 0 and b"texels and tex_table must not be NULL where n_tex > 0" in msg(), k
            assert fn(**{k: None}, n_tex=0, h=0) != 0 and b"h and w must be in" in msg(), k
        for k in rows:
            assert fn(**{k: None}) != 0 and b"mesh_index, R, t, K, light, phong, wrap and face must not be NULL" in msg(), k
        assert fn(info=None) != 0 and b"info must not be NULL" in msg()
        for bad in ((0, 20), (16, 0), (16385, 20), (16, 16385), (-1, 20)):
            assert fn(h=bad[0], w=bad[1]) != 0 and b"h and w must be in [1, 16384], got" in msg(), bad
        for bad in ((0.501, 0.5), (0.5, 64.5), (float("nan"), 0.5), (-65.0, 0.0)):
            assert fn(cx=bad[0], cy=bad[1]) != 0 and b"cx and cy must be multiples of 2^-8 in [-64, 64]" in msg(), bad
        for bad in (-1, 2):
            assert fn(lod=bad) != 0 and b"lod must be 0 or 1, got" in msg(), bad
        for k in ("verts", "normals", "faces", "uv", "table", "tex_index"):
            assert fn(**{k: p + 2}) != 0 and b"verts, normals, faces, uv, mesh_table and tex_index must be aligned to 4 bytes" in msg(), k
        assert fn(texels=p + 2) != 0 and b"texels must be aligned to 4 bytes and tex_table to 8" in msg()
        assert fn(tex_table=p + 4) != 0 and b"texels must be aligned to 4 bytes and tex_table to 8" in msg()
        for k in rows:
            assert fn(**{k: p + 2}) != 0 and b"wrap, face and info must be aligned to 4 bytes" in msg(), k
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

    # the mip builder reads its HOST table first and refuses an entry that is invalid or reaches outside the buffer
    def mips(entries, total, texels=p, n_tex=None, table=True):
        arr = (ctypes.c_longlong * (4 * len(entries)))(*[v for e in entries for v in e])
        return lib.lc_tex_build_mips_u8(texels, total, ctypes.addressof(arr) if table else None, len(entries) if n_tex is None else n_tex, None)

    me = b"lc_tex_build_mips_u8: "
    assert mips([], 0) == 0 and mips([], 0, texels=None, table=False) == 0
    assert mips([(0, 1, 1, 1)], 1, n_tex=-1) != 0 and me + b"n_tex < 0 or total_texels < 0" in msg()
    assert mips([(0, 1, 1, 1)], -1) != 0 and b"n_tex < 0 or total_texels < 0" in msg()
    assert mips([(0, 1, 1, 1)], 1, texels=None) != 0 and b"texels and tex_table_host must not be NULL" in msg()
    assert mips([(0, 1, 1, 1)], 1, table=False) != 0 and b"texels and tex_table_host must not be NULL" in msg()
    assert mips([(0, 1, 1, 1)], 1, texels=p + 2) != 0 and b"texels must be aligned to 4 bytes" in msg()
    for bad in ((0, 8, 8, 4), (-1, 2, 2, 1), (80, 2, 2, 2), (0, 0, 2, 1), (0, 2, 0, 1), (0, 2, 2, 0), (0, 2, 2, 16), (0, 16385, 1, 1), (2 ** 40, 2, 2, 1)):
        assert mips([(0, 2, 2, 1), bad], 84) != 0 and me + b"texture 1: the entry (" in msg() and b"reaches outside the 84 texels" in msg(), bad  # 8 x 8 with 4 levels: 85
    assert mips([(0, 1, 1, 1), (1, 1, 1, 1)], 2) == 0  # level 0 only: valid, and nothing to launch


def test_wrapper_refusals():
    from lc_amd import texture
    from tests import shade_cases as cases
    from tests.test_shade_host import _host_set

    ms = _host_set([cases.ICO, cases.QUAD])
    with pytest.raises(ValueError, match=r"images is a list of \(Ht,Wt,3\) uint8 arrays"):
        texture.TextureStore.from_images(np.zeros((4, 4, 3), np.uint8), "cuda")
    with pytest.raises(TypeError, match="image 1 must be uint8, got float32"):
        texture.TextureStore.from_images([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.float32)], "cuda")
    for bad in ((4, 4), (4, 4, 4), (0, 4, 3), (16385, 1, 3)):
        with pytest.raises(ValueError, match=r"image 0 has shape .*expected \(Ht,Wt,3\) with sides of 1 to 16384"):
            texture.TextureStore.from_images([np.zeros(bad, np.uint8)], "cuda")
    with pytest.raises(ValueError, match="levels"):
        texture.TextureStore.from_images([np.zeros((4, 4, 3), np.uint8)], "cuda", levels=0)
    with pytest.raises(RuntimeError, match="the store lives on the MI355X.*no CPU fallback"):
        texture.TextureStore.from_images([np.zeros((4, 4, 3), np.uint8)], "cpu")
    assert texture.level_sizes(3, 5, 4) == [(3, 5), (1, 2), (1, 1), (1, 1)]
    store = texture.TextureStore(torch.zeros(20, 4, dtype=torch.uint8), np.array([[0, 3, 5, 3], [18, 1, 2, 2]], np.int64))  # a stand-in on the host: refusals only
    assert tuple(store.level(0, 1).shape) == (1, 2, 3) and store.n_tex == 2 and store.total_texels == 20
    with pytest.raises(IndexError, match="texture 1 has 2 levels"):
        store.level(1, 2)

    per_vertex = np.random.default_rng(0).random((12, 2)).astype(np.float32)
    with pytest.raises(TypeError, match="textures must be a TextureStore"):
        texture.TexturedAppearance(ms, [None, None], [-1, -1], None)
    with pytest.raises(ValueError, match=r"uvs is a list of one array per mesh \(2\)"):
        texture.TexturedAppearance(ms, [per_vertex], [0, -1], store)
    with pytest.raises(ValueError, match=r"tex_index holds one whole number per mesh \(2\)"):
        texture.TexturedAppearance(ms, [per_vertex, None], [0], store)
    with pytest.raises(ValueError, match=r"tex_index must lie in \[-1, 2\), got \[-1, 2\]"):
        texture.TexturedAppearance(ms, [per_vertex, None], [2, -1], store)
    with pytest.raises(ValueError, match="mesh 1 has texture 0 and no uv"):
        texture.TexturedAppearance(ms, [per_vertex, None], [0, 0], store)
    with pytest.raises(ValueError, match=r"mesh 1: uv has shape \(3, 2\), expected per-corner \(2, 3, 2\) or per-vertex \(4, 2\)"):
        texture.TexturedAppearance(ms, [per_vertex, np.zeros((3, 2), np.float32)], [0, 1], store)
    with pytest.raises(TypeError, match="mesh 0: uv must hold floats"):
        texture.TexturedAppearance(ms, [np.zeros((12, 2), np.int32), None], [0, -1], store)
    ap = texture.TexturedAppearance(ms, [per_vertex, None], np.array([1, -1]), store, [None, cases.QUAD_COLORS])
    assert ap.uv.shape == (22, 3, 2) and ap.uv.dtype == torch.float32 and np.array_equal(ap.uv_host[:20], per_vertex[cases.ICO[1]]) and not ap.uv_host[20:].any()
    assert ap.tex_index_host.tolist() == [1, -1] and ap.tex_index.dtype == torch.int32 and np.array_equal(ap.colors_host[12:], cases.QUAD_COLORS)
    corner = np.random.default_rng(1).random((20, 3, 2))
    assert np.array_equal(texture.TexturedAppearance(ms, [corner, None], [0, -1], store).uv_host[:20], corner.astype(np.float32))

    face, mi = torch.full((2, 8, 12), -1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    R, t, K = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.eye(3)

    def call(meshes=ms, appearance=ap, face=face, mesh_index=mi, R=R, t=t, K=K, **kw):
        return texture.shade(meshes, appearance, face, mesh_index, R, t, K, **{"light": texture.DEFAULT_LIGHT, "phong": texture.DEFAULT_PHONG, **kw})

    with pytest.raises(TypeError, match="meshes must be a MeshSet"):
        call(meshes=None)
    with pytest.raises(TypeError, match="appearance must be a TexturedAppearance"):
        call(appearance=ap.base)
    with pytest.raises(ValueError, match="appearance was made for another MeshSet"):
        call(meshes=_host_set([cases.ICO, cases.QUAD]))
    with pytest.raises(TypeError, match="lod must be True or False"):
        call(lod=1)
    with pytest.raises(TypeError, match="lc_amd.texture: face must be int32, got torch.int64"):
        call(face=face.long())
    with pytest.raises(RuntimeError, match="R is on cpu.*no CPU fallback"):
        call()
    for bad in (2, -1, "mirror", True, 0.5):
        with pytest.raises(ValueError, match=r'wrap is 0 or "clamp", 1 or "repeat", or an int32 tensor of shape \(2,\)'):
            texture._wrap(bad, 2, torch.device("cpu"))
    assert texture._wrap("repeat", 2, torch.device("cpu")).tolist() == [1, 1] and texture._wrap(0, 3, torch.device("cpu")).tolist() == [0, 0, 0]
    with pytest.raises(TypeError, match="wrap must be int32"):
        texture._wrap(torch.zeros(2, dtype=torch.int64), 2, torch.device("cpu"))
    for bad in ((1.0, 2.0), "abc", None):
        with pytest.raises(ValueError, match="light is three finite numbers or a float32 tensor"):
            texture._per_row("light", bad, 2, torch.device("cpu"))
    with pytest.raises(TypeError, match="appearance must be a TexturedAppearance"):
        texture.render_color(ms, ap.base, mi, R, t, K, (8, 12), near=0.1, far=2.0, light=texture.DEFAULT_LIGHT, phong=texture.DEFAULT_PHONG)
    with pytest.raises(TypeError, match="appearance must be a TexturedAppearance"):
        texture.render_scene(ms, ap.base, mi, mi, R, t, K, (8, 12), 1, near=0.1, far=2.0, light=texture.DEFAULT_LIGHT, phong=texture.DEFAULT_PHONG)


def _write_ply(path, binary, per_face, colors=True):
    """A two-face quad with normals, written here: ascii or binary_little_endian, texture coordinates per vertex or per face corner."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]], np.float32)
    normals = np.array([[0, 0, 1]] * 4, np.float32)
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 8, 7]], np.uint8)
    vt = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    corner = np.array([[[0, 0], [0.5, 0], [0.5, 1]], [[0.25, 0], [1, 1], [0, 1]]], np.float32)  # vertex 0 and 2 differ between the faces: a seam
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment made by a test", "comment TextureFile quad tex.png", "element vertex 4",
            "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz"]
    if not per_face:
        head += ["property float texture_u", "property float texture_v"]
    if colors:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face 2", "property list uchar int vertex_indices"] + (["property list uchar float texcoord"] if per_face else []) + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for k in range(4):
            vals = [*verts[k], *normals[k]] + ([] if per_face else [*vt[k]])
            if binary:
                fh.write(struct.pack(f"<{len(vals)}f", *vals) + (bytes(rgb[k]) if colors else b""))
            else:
                fh.write((" ".join(repr(float(v)) for v in vals) + (" " + " ".join(str(int(c)) for c in rgb[k]) if colors else "") + "\n").encode())
        for f in range(2):
            if binary:
                fh.write(struct.pack("<B3i", 3, *faces[f]) + (struct.pack("<B6f", 6, *corner[f].reshape(-1)) if per_face else b""))
            else:
                fh.write((f"3 {' '.join(str(int(i)) for i in faces[f])}" + (" 6 " + " ".join(repr(float(v)) for v in corner[f].reshape(-1)) if per_face else "") + "\n").encode())
    return verts, normals, rgb, faces, (corner if per_face else vt[faces])


@pytest.mark.parametrize("per_face", [False, True])
@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_textured_reads_both_encodings_and_both_uv_forms(tmp_path, binary, per_face):
    from lc_amd import texture

    path = tmp_path / "quad.ply"
    verts, normals, rgb, faces, uv = _write_ply(path, binary, per_face)
    ply = texture.read_ply_textured(str(path))
    assert ply.verts.dtype == np.float32 and ply.faces.dtype == np.int32 and ply.colors.dtype == np.uint8 and ply.uv.dtype == np.float32
    assert np.array_equal(ply.verts, verts) and np.array_equal(ply.faces, faces) and np.array_equal(ply.colors, rgb) and np.array_equal(ply.normals, normals)
    assert ply.uv.shape == (2, 3, 2) and np.array_equal(ply.uv, uv) and ply.texture_file == "quad tex.png"
    _write_ply(path, binary, per_face, colors=False)
    assert texture.read_ply_textured(str(path)).colors is None


def test_read_ply_textured_refuses_what_it_does_not_read(tmp_path):
    from lc_amd import texture

    path = tmp_path / "bad.ply"
    path.write_bytes(b"plx\nend_header\n")
    with pytest.raises(ValueError, match="is not a PLY file"):
        texture.read_ply_textured(str(path))
    path.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="ascii and binary_little_endian are read"):
        texture.read_ply_textured(str(path))
    head = b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
    path.write_bytes(head + b"0 0 0\n1 0 0\n0 1 0\n4 0 1 2 2\n")
    with pytest.raises(ValueError, match="every face must be a triangle"):
        texture.read_ply_textured(str(path))
    path.write_bytes(head + b"0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n")
    with pytest.raises(ValueError, match=r"face indices must lie in \[0, 3\)"):
        texture.read_ply_textured(str(path))
    path.write_bytes(head + b"0 0 0\n1 0 0\n0 1 0\n3 0 1\n")
    with pytest.raises(ValueError, match="element face is cut short"):
        texture.read_ply_textured(str(path))
    path.write_bytes(head + b"0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    ply = texture.read_ply_textured(str(path))
    assert ply.uv is None and ply.colors is None and ply.normals is None and ply.texture_file is None and ply.faces.tolist() == [[0, 1, 2]]
