"""Host-side contract of the depth rasteriser's library (liblc_amd_render.so): header = exports = ctypes table, the embedded source hash,
the other libraries' sources and hashes untouched, every argument check of the entry point, kernel resources, and the host parts of the
Python surface (MeshSet validation, the PLY reader, the z_info encode / decode, the errors).  No GPU needed."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_ctypes_table_agree():
    from lc_amd import build, render

    lib = render.load()
    header = open(os.path.join(ROOT, "include", "lc_amd_render.h")).read()
    declared = set(re.findall(r"^(?:const\s+)?\w+\s+\*?(lc_\w+)\(", header, flags=re.M))
    assert declared == set(render._SIGNATURES) == {"lc_amd_render_version", "lc_amd_render_last_error", "lc_amd_render_source_hash",
                                                   "lc_render_workspace_bytes", "lc_render_depth_f32"}
    out = subprocess.run(["nm", "-D", "--defined-only", build.RENDER.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("lc_")} == declared, exported
    assert lib.lc_amd_render_version() == int(re.search(r"#define LC_AMD_RENDER_VERSION (\d+)", header).group(1)) == 1
    consts = dict(re.findall(r"#define (LC_RENDER_\w+) (\d+)", header))
    assert (int(consts["LC_RENDER_MAX_SIZE"]), int(consts["LC_RENDER_RECORD_BYTES"])) == (render.MAX_SIZE, render.RECORD_BYTES)
    proto = re.search(r"int lc_render_depth_f32\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(render._SIGNATURES["lc_render_depth_f32"][1])
    assert lib.lc_render_workspace_bytes(3, 100) == 3 * 100 * render.RECORD_BYTES and lib.lc_render_workspace_bytes(0, 5) == 0 == lib.lc_render_workspace_bytes(5, 0)
    assert lib.lc_render_workspace_bytes(65535, 2 ** 21) == 65535 * 2 ** 21 * 64  # beyond 2^32: size_t arithmetic


def test_embedded_source_hash_and_separate_sources():
    from lc_amd import build, render

    lib = render.load()
    assert lib.lc_amd_render_source_hash().decode() == build.source_hash(build.RENDER) == build.embedded_hash(build.RENDER.so_path, build.RENDER.hash_marker)
    assert build.sources(build.RENDER) == [os.path.join(build.CSRC, "render", "lc_render.hip")]
    for t in build.TARGETS:  # no other library hashes a file with this one's name in it (its directory and header: tests/test_libraries_host.py)
        assert t is build.RENDER or not any("render" in os.path.basename(s) for s in build._deps(t))
    for t in build.TARGETS:  # the other libraries, as built, still carry the hash of their sources
        assert t is build.RENDER or build.embedded_hash(t.so_path, t.hash_marker) in (None, build.source_hash(t))


def _call(lib, **over):
    """The entry point with host pointers (which never launch: every call here fails a check, or has nothing to do)."""
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    a = dict(verts=p, faces=p, table=p, index=p, n_meshes=1, total_verts=8, total_faces=4, max_faces=4, R=p, t=p, K=p, pix2k=None, B=1, H=8, W=8,
             near=0.01, far=6.5, cx=0.5, cy=0.5, depth=p, face=None, mask=None, homo=None, info=p, ws=p, ws_bytes=4096, stream=None)
    a.update(over)
    return lib.lc_render_depth_f32(*a.values()), lib.lc_amd_render_last_error()


def test_entry_point_checks_its_arguments():
    from lc_amd import render

    lib = render.load()
    assert _call(lib, B=0)[0] == 0  # nothing to do: no launch
    assert _call(lib, B=0, verts=None, depth=None)[0] == 0
    rc_, msg = _call(lib, B=-1)
    assert rc_ != 0 and b"B < 0" in msg
    for kw in (dict(H=0), dict(W=0), dict(H=render.MAX_SIZE + 1)):
        rc_, msg = _call(lib, **kw)
        assert rc_ != 0 and b"H and W" in msg
    for kw in (dict(near=1.0, far=1.0), dict(near=2.0, far=1.0), dict(near=float("nan"))):
        rc_, msg = _call(lib, **kw)
        assert rc_ != 0 and b"near < far" in msg
    for kw in (dict(cx=0.3), dict(cy=1.0 / 512), dict(cx=100.0), dict(cy=float("inf"))):
        rc_, msg = _call(lib, **kw)
        assert rc_ != 0 and b"2^-8" in msg
    for name in ("table", "index", "R", "t", "K", "verts", "faces", "depth", "info"):
        rc_, msg = _call(lib, **{name: None})
        assert rc_ != 0 and b"NULL" in msg, name
    rc_, msg = _call(lib, n_meshes=-1)
    assert rc_ != 0 and b"negative" in msg
    for kw in (dict(ws=None), dict(ws_bytes=255), dict(ws=torch.zeros(64).data_ptr() + 4)):
        rc_, msg = _call(lib, **kw)
        assert rc_ != 0 and b"workspace" in msg
    rc_, msg = _call(lib, B=70000, ws_bytes=70000 * 4 * 64)
    assert rc_ != 0 and b"too many" in msg


def test_kernels_use_no_scratch_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, render

    render.load()
    res = kernel_resources(build.RENDER.so_path)
    assert len(res) == 2 and sum("lc_render_setup_kernel" in n for n in res) == 1 and sum("lc_render_raster_kernel" in n for n in res) == 1
    for name, d in res.items():
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (name, d)
        assert d.get("group_segment_fixed_size", 0) <= 64 * 1024, name  # all LDS is static: the tile's 1024 keys and one counter
        if "raster" in name:
            assert 8192 <= d["group_segment_fixed_size"] <= 8192 + 64


def test_mesh_set_rejects_what_a_launch_could_fault_on():
    from lc_amd.render import MeshSet

    v, f = rc.MESHES["torus"]
    for bad, exc, msg in ((np.where(f == 3, len(v), f), ValueError, "face indices"), (np.where(f == 3, -1, f), ValueError, "face indices"),
                          (f.astype(np.float32), TypeError, "integers"), (f[:, :2], ValueError, r"\(Nf,3\)")):
        with pytest.raises(exc, match=msg):
            MeshSet([rc.MESHES["ico"], (v, bad)], "cuda")
    for val in (np.nan, np.inf, -np.inf):
        vb = v.copy()
        vb[5, 1] = val
        with pytest.raises(ValueError, match="finite"):
            MeshSet([(vb, f)], "cuda")
    with pytest.raises(ValueError, match="obj_ids"):
        MeshSet([(v, f), (v, f)], "cuda", obj_ids=[4, 4])
    with pytest.raises(ValueError, match="at least one"):
        MeshSet([], "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshSet([(v, f)], "cpu")


def test_dropin_native_depth_takes_the_stored_depth_out_of_the_reference_loader(monkeypatch, tmp_path):
    """A stub of the reference's `dataset` module whose loader does what dataset.py:287-291,381,444,460 do -- open `z_path`, deliver
    `homo_z_out` -- must, after the opt-in, neither touch the file nor deliver the key; everything else of the blob stays."""
    import types

    from lc_amd import dropin, gen_z, labels

    ds = types.ModuleType("dataset")

    class BOP_Dataset:
        def _get_homo_with_depth(self, annot, size_hw, fill_hole=True):
            with open(annot[1]["z_path"], "rb"):  # no z_crop directory: FileNotFoundError
                pass
            raise AssertionError("unreachable")

        def _get_single_item(self, index):
            homo_z, mask_full = self._get_homo_with_depth(({}, {"z_path": str(tmp_path / "z_crop" / "000000_000000.pkl.gz")}), (6, 8), False)
            assert homo_z.shape == (6, 8, 3) and homo_z.dtype == np.float32 and mask_full.shape == (6, 8) and not homo_z.any()
            return None if index < 0 else {"homo_z_out": homo_z[:4, :4], "msk_noc": np.ones((4, 4), bool), "obj_id": 5, "K_no_aug": np.eye(3)}

    ds.BOP_Dataset = BOP_Dataset
    monkeypatch.setitem(sys.modules, "dataset", ds)
    with pytest.raises(FileNotFoundError):
        BOP_Dataset()._get_single_item(0)
    seen = {}
    monkeypatch.setattr(gen_z, "load_models", lambda d, dev, scale: seen.update(dir=d, scale=scale) or "MESHES")
    monkeypatch.setattr(labels, "set_depth_source", lambda m, near, far: seen.update(m=m, near=near, far=far))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    assert dropin._install_depth("/data/models") is True
    assert seen == dict(dir="/data/models", scale=1.0, m="MESHES", near=10.0, far=6500.0)  # mm, as the poses of a BOP dataset
    blob = BOP_Dataset()._get_single_item(0)
    assert set(blob) == {"msk_noc", "obj_id", "K_no_aug"}
    assert BOP_Dataset()._get_single_item(-1) is None  # the loader's "try another sample" passes through
    assert dropin._detach_loader_from_z_crop() is True and set(BOP_Dataset()._get_single_item(0)) == {"msk_noc", "obj_id", "K_no_aug"}  # idempotent
    monkeypatch.setitem(sys.modules, "dataset", None)  # no reference loader: the opt-in says so
    assert dropin._detach_loader_from_z_crop() is False


def test_cpu_tensors_raise():
    from lc_amd import labels, render

    z = torch.zeros(1, 3, 3)
    with pytest.raises(TypeError, match="MeshSet"):
        render.render_depth(None, torch.zeros(1, dtype=torch.int32), z, torch.zeros(1, 3), z, (8, 8), near=0.1, far=1.0)
    ms = object.__new__(render.MeshSet)  # a set that was never uploaded: the tensor checks come first
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.render_depth(ms, torch.zeros(1, dtype=torch.int32), z, torch.zeros(1, 3), z, (8, 8), near=0.1, far=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.render_homo_z_out(ms, torch.zeros(1, dtype=torch.int32), z, torch.zeros(1, 3), z, z, (8, 8), near=0.1, far=1.0)
    with pytest.raises(TypeError, match="MeshSet"):
        labels.set_depth_source("models", 0.1, 1.0)
    labels.clear_depth_source()
    assert labels._DEPTH_SOURCE is None


def test_dropin_takes_the_native_depth_flag(monkeypatch, tmp_path):
    from lc_amd import dropin

    seen = {}
    monkeypatch.setattr(dropin, "install", lambda **kw: seen.update(kw) or {})
    script = tmp_path / "train.py"
    script.write_text("import sys\nARGS = list(sys.argv)\n")
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    dropin.main(["--native-depth", "/data/models", "--native-optim", str(script), "--cfg", "x.yaml"])
    assert seen == dict(native_labels=False, native_optim=True, native_depth="/data/models") and sys.argv == [str(script), "--cfg", "x.yaml"]
    with pytest.raises(SystemExit):
        dropin.main(["--native-depth"])


def _ply_ascii(path, v, f):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\ncomment extra properties and an extra element\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
                 f"property float z\nproperty float nx\nproperty uchar red\nelement face {len(f)}\nproperty list uchar int vertex_indices\n"
                 f"property list uchar float texcoord\nelement edge 2\nproperty int vertex1\nproperty int vertex2\nend_header\n")
        for p in v:
            fh.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 0.25 200\n")
        for t in f:
            fh.write(f"3 {t[0]} {t[1]} {t[2]} 2 0.5 0.5\n")
        fh.write("0 1\n1 2\n")


def _ply_binary(path, v, f, quads=()):
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty double x\nproperty float y\nproperty float z\n"
                  f"property float nx\nproperty uchar red\nproperty ushort q\nelement face {len(f) + len(quads)}\nproperty uchar flag\n"
                  f"property list uchar uint vertex_index\nproperty list uchar float texcoord\nend_header\n").encode())
        for p in v:
            fh.write(struct.pack("<dfffBH", float(p[0]), float(p[1]), float(p[2]), 0.5, 7, 9))
        for t in f:
            fh.write(struct.pack("<BBIIIBff", 1, 3, int(t[0]), int(t[1]), int(t[2]), 2, 0.5, 0.25))
        for t in quads:
            fh.write(struct.pack("<BBIIIIB", 1, 4, *[int(x) for x in t], 0))


def test_ply_reader_ascii_and_binary_with_properties_to_skip(tmp_path):
    from lc_amd.gen_z import read_ply

    v, f = rc.MESHES["torus"]
    _ply_ascii(tmp_path / "a.ply", v, f)
    va, fa = read_ply(tmp_path / "a.ply")
    assert va.dtype == np.float32 and fa.dtype == np.int32 and np.array_equal(va, v) and np.array_equal(fa, f)
    _ply_binary(tmp_path / "b.ply", v, f, quads=[(0, 1, 2, 3)])
    vb, fb = read_ply(tmp_path / "b.ply")
    assert np.array_equal(vb, v) and np.array_equal(fb[:-2], f) and fb[-2:].tolist() == [[0, 1, 2], [0, 2, 3]]  # a quad is fanned
    (tmp_path / "c.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="not supported"):
        read_ply(tmp_path / "c.ply")
    (tmp_path / "d.ply").write_bytes(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply(tmp_path / "d.ply")
    _ply_ascii(tmp_path / "e.ply", v[:10], f)
    with pytest.raises(ValueError, match="face indices"):
        read_ply(tmp_path / "e.ply")


def test_z_info_round_trip_follows_the_formulae():
    """encode: round((z - z_min) / (z_max - z_min + 1e-30) * 65534 + 1) on hit pixels, cropped to the hit box, z_max / z_min in mm;
    decode: (code - 1) (z_max - z_min) / 65534 + z_min.  The round trip is within half a step plus the fp32 arithmetic."""
    from lc_amd.render import decode_z_info, encode_z_info

    rng = np.random.default_rng(3)
    depth = np.zeros((48, 64), dtype=np.float32)
    depth[7:30, 11:50] = (0.4 + 0.3 * rng.random((23, 39))).astype(np.float32)
    depth[12:15, 20:25] = 0  # holes stay holes
    info = encode_z_info(torch.from_numpy(depth))
    m = depth > 0
    z_min, z_max = depth[m].min(), depth[m].max()
    assert info["xyxy"] == [11, 7, 49, 29] and info["z_crop"].dtype == np.uint16 and info["z_crop"].shape == (23, 39)
    assert np.float32(info["z_max"]) == z_max * 1000 and np.float32(info["z_min"]) == z_min * 1000
    want = np.where(m, (depth - z_min) / (z_max - z_min + 1e-30) * 65534 + 1, 0)[7:30, 11:50].round().astype(np.uint16)
    assert np.array_equal(info["z_crop"], want) and want.max() == 65535 and want[want > 0].min() == 1
    back, mask = decode_z_info(info, depth.shape)
    assert np.array_equal(mask, m)
    step = float(z_max - z_min) * 1000 / 65534
    assert np.abs(back.astype(np.float64) - depth.astype(np.float64) * 1000)[m].max() <= 0.5 * step + 8 * 2.0 ** -24 * 1000 * float(z_max)
    empty = encode_z_info(torch.zeros(48, 64))  # the reference's not-visible record (gen_z.py:161-166)
    assert empty["z_crop"].shape == (48, 64) and empty["z_crop"].dtype == np.uint16 and not empty["z_crop"].any() and empty["xyxy"] == [0, 0, 63, 47]
    assert empty["z_max"].shape == (1,) and empty["z_max"].dtype == np.float32 and empty["z_max"][0] == 0 == empty["z_min"][0]
