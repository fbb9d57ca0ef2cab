"""lc_amd.models / lc_amd.prep_models without a GPU: the oracle's own properties, the refusals and the workspace formula of the C entry
point (nothing is launched), the file formats, and the tool with `models.prepare` patched to the oracle."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

from tests import models_cases as mc
from tests.util import GOLDEN


def test_oracle_prefix_property():
    """The first n rows of a count-point result are the n-point result (the loader's `[:sparse_cnt]` relies on it)."""
    for v in (mc.cloud(300, 1), mc.cube_with_duplicates(), mc.collinear()):
        full_i, full_p = mc.fps(v, len(v) if len(v) < 64 else 64)
        for n in (1, 2, 16, len(full_i)):
            i, p = mc.fps(v, n)
            assert np.array_equal(i, full_i[:n]) and np.array_equal(p, full_p[:n])
        assert len(set(full_i[:8].tolist())) == 8  # distinct while distinct positions remain
    # ties: the cube's first pick is the lowest-index corner, its diameter pair the smallest (i, j) among 36 pairs of equal length
    v = mc.cube_with_duplicates()
    assert mc.fps(v, 1)[0][0] == 0
    d, (i, j) = mc.diameter(v)
    sq = mc.d2(v[:, None], v[None])
    cand = [(a, b) for a in range(len(v)) for b in range(a + 1, len(v)) if sq[a, b] == sq.max()]
    assert len(cand) == 36 and (i, j) == min(cand) and d == np.sqrt(np.float32(3.0), dtype=np.float32)


def test_oracle_diameter_against_fp64_brute_force():
    """Each d2 carries at most five fp32 roundings and the square root one more: below 4 * 2^-24 relative; the tolerance doubles it."""
    for v in (mc.cloud(700, 2), mc.cloud(300, 9, scale=40.0, offset=0.0), mc.collinear(), mc.cloud(2, 5)):
        d, (i, j) = mc.diameter(v)
        w = v.astype(np.float64)
        ref = np.sqrt(((w[:, None] - w[None]) ** 2).sum(-1)).max()
        assert abs(float(d) - ref) <= 2.0 ** -21 * ref
        assert i < j and abs(np.linalg.norm(w[i] - w[j]) - ref) <= 2.0 ** -21 * ref
    assert mc.diameter(mc.cloud(1, 3)) == (np.float32(0), (0, 0))


def test_header_exports_and_build_target_agree():
    """The library is one of its own: its header, its exports and its ctypes table name the same five symbols, it carries the hash of its
    sources (that no other library sees its directory: tests/test_libraries_host.py)."""
    import re
    import subprocess

    from lc_amd import build, models

    lib = models.load()
    root = os.path.join(os.path.dirname(GOLDEN), "..")
    header = open(os.path.join(root, "include", "lc_amd_models.h")).read()
    declared = set(re.findall(r"^(?:const\s+)?\w+\s+\*?(lc_\w+)\(", header, flags=re.M))
    assert declared == set(models._SIGNATURES) == {"lc_amd_models_version", "lc_amd_models_last_error", "lc_amd_models_source_hash",
                                                   "lc_model_workspace_bytes", "lc_model_prepare_f32"}
    out = subprocess.run(["nm", "-D", "--defined-only", build.MODELS.so_path], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("lc_")} == declared
    proto = re.search(r"int lc_model_prepare_f32\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(models._SIGNATURES["lc_model_prepare_f32"][1])
    assert lib.lc_amd_models_version() == 1 and not build.is_stale(build.MODELS)
    assert lib.lc_amd_models_source_hash().decode() == build.source_hash(build.MODELS)
    assert build.sources(build.MODELS) == [os.path.join(build.CSRC, "models", "lc_models.hip")]


def test_workspace_formula():
    from lc_amd import models

    lib = models.load()
    T, R = models.DIAM_TILE, models.FPS_RESIDENT
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "lc_amd_models.h")).read()
    assert f"#define LC_MODEL_DIAM_TILE {T}\n" in hdr and f"#define LC_MODEL_FPS_RESIDENT {R}\n" in hdr
    assert lib.lc_model_workspace_bytes(0, 100, 4) == 0 and lib.lc_model_workspace_bytes(3, 0, 4) == 0
    for n, V, c in ((1, 1, 0), (1, T, 16), (1, T + 1, 16), (3, 2 * T + 1, 0), (21, 5000, 256), (2, R, 256), (2, R + 1, 256), (2, R + 1, 0), (21, 250001, 256)):
        t = -(-V // T)
        want = 16 * n * t * (t + 1) // 2 + (4 * n * (-(-V // 4) * 4) if c > 0 and V > R else 0)
        assert lib.lc_model_workspace_bytes(n, V, c) == want == models.workspace_bytes(n, V, c), (n, V, c)


def test_every_refusal_comes_before_any_launch():
    """Follows test_ransac_workspace_contract: host memory stands in for every device pointer, so a call that got as far as a launch
    could not return its argument error."""
    from lc_amd import models

    lib = models.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    table = (ctypes.c_int * 8)(0, 10, 0, 0, 10, 5, 0, 0)  # two meshes: 10 and 5 vertices
    err = lambda: lib.lc_amd_models_last_error().decode()
    big = 1 << 20

    def call(verts=p, tab=p, host=table, n=2, mv=10, c=4, lo=p, hi=p, dia=p, pair=p, fps=p, idx=p, ws=p, wsb=big):
        return lib.lc_model_prepare_f32(verts, tab, host, n, mv, c, lo, hi, dia, pair, fps, idx, ws, wsb, None)

    assert call(n=0) != 0 and "n_meshes" in err()
    assert call(n=-1) != 0 and "n_meshes" in err()
    assert call(mv=0) != 0 and "max_verts" in err()
    assert call(mv=(1 << 30) // 3 * 2) != 0 and "2^31" in err()  # 32-bit coordinate indices
    assert call(c=-1) != 0 and "fps_count" in err()
    for kw in (dict(verts=None), dict(tab=None), dict(host=None)):
        assert call(**kw) != 0 and "null pointer" in err()
    assert call(lo=None, hi=None, dia=None, pair=None, fps=None, idx=None) != 0 and "no output" in err()
    assert call(c=6) != 0 and "fps_count 6 exceeds the 5 vertices of mesh 1" in err()
    assert call(c=6, fps=None, idx=None, lo=None, hi=None, ws=None) != 0 and "workspace" in err()  # fps skipped: its count is not judged
    assert call(mv=9) != 0 and "mesh 0" in err() and "max_verts" in err()
    assert call(host=(ctypes.c_int * 8)(0, 10, 0, 0, -1, 5, 0, 0)) != 0 and "mesh 1" in err()
    assert call(host=(ctypes.c_int * 8)(0, 0, 0, 0, 0, 5, 0, 0)) != 0 and "mesh 0" in err()
    assert call(ws=None) != 0 and "workspace is null" in err()
    need = lib.lc_model_workspace_bytes(2, 10, 4)
    assert need == 32 and call(wsb=need - 1) != 0 and "workspace too small" in err()
    assert call(ws=p + 4) != 0 and "aligned" in err()
    assert call(lo=p + 2) != 0 and "aligned" in err()
    # the streaming form's distances are part of the workspace
    host = (ctypes.c_int * 4)(0, 9000, 0, 0)
    need = lib.lc_model_workspace_bytes(1, 9000, 4)
    assert call(host=host, n=1, mv=9000, dia=None, pair=None, wsb=need - 1) != 0 and "workspace too small" in err()
    assert call(host=host, n=1, mv=9000, c=9001) != 0 and "exceeds" in err()


def test_fps_dict_has_the_format_of_the_reference_asset():
    from lc_amd import models

    with open(os.path.join(GOLDEN, "fps_lmo.pkl"), "rb") as f:
        asset = pickle.load(f)
    assert sorted(asset) == [1, 5, 6, 8, 9, 10, 11, 12]
    ids = sorted(asset)
    info = mc.prepare_oracle(mc.host_set([(asset[i], mc.FACES0) for i in ids], ids), 256, want_diameter=False)
    ours = models.to_fps_dict(info, ids)
    assert list(ours) == ids
    for k, a in asset.items():
        b = ours[k]
        assert type(k) is int and all(type(q) is int for q in ours)
        assert type(b) is type(a) is np.ndarray and b.dtype == a.dtype == np.float32 and b.shape == a.shape == (256, 3)
        assert sorted(map(tuple, b.tolist())) == sorted(map(tuple, a.tolist()))  # every point once: a permutation of the mesh
    unpickled = pickle.loads(pickle.dumps(ours))
    assert all(np.array_equal(unpickled[k], ours[k]) for k in ids)
    # object 1's 256 points as a mesh: the asset's own order is a farthest-point order from the box centre
    assert info.fps_index[0][:16].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    d, pair = mc.diameter(asset[1])
    assert (float(d), pair) == (float(np.float32(101.33025)), (0, 3))
    with pytest.raises(ValueError):
        models.to_fps_dict(info, ids[:-1])
    with pytest.raises(ValueError):
        models.to_models_info(info, ids)  # no diameter in it


def _write_ply(path, v, f):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for p in v:
            fh.write(" ".join(repr(float(c)) for c in p) + "\n")
        for t in f:
            fh.write("3 " + " ".join(str(int(c)) for c in t) + "\n")


def test_prep_models_tool(tmp_path, monkeypatch, capsys):
    from lc_amd import models, prep_models

    tet = np.array([[-10, -20, -30], [40, 0, 0], [0, 50, 0], [0, 0, 60], [5, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32)
    other = mc.cloud(40, 11, scale=25.0)
    _write_ply(tmp_path / "obj_000002.ply", tet, faces)
    _write_ply(tmp_path / "obj_000007.ply", other, faces)
    (tmp_path / "obj_notes.ply").write_text("not a model")  # not obj_<digits>.ply: ignored
    monkeypatch.setattr(prep_models, "_device", lambda: "host")
    monkeypatch.setattr(prep_models, "MeshSet", lambda meshes, device, obj_ids=None: mc.host_set(meshes, obj_ids))
    monkeypatch.setattr(models, "prepare", mc.prepare_oracle)
    info_path, fps_path = tmp_path / "models_info.json", tmp_path / "fps.pkl"

    assert prep_models.main([str(tmp_path), "--fps", "4", "--scale", "0.5"]) == 0
    out = capsys.readouterr().out
    assert out.count("obj 2: 5 vertices") == 1 and out.count("obj 7: 40 vertices") == 1
    stored = json.load(open(info_path))
    assert sorted(stored) == ["2", "7"]
    assert all(sorted(v) == sorted(["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"]) for v in stored.values())
    half = tet * np.float32(0.5)
    assert [stored["2"][k] for k in ("min_x", "min_y", "min_z")] == [-5.0, -10.0, -15.0]
    assert [stored["2"][k] for k in ("size_x", "size_y", "size_z")] == [25.0, 35.0, 45.0]
    assert stored["2"]["diameter"] == float(mc.diameter(half)[0])
    # read as model_transform.load_composed_model_info reads it: int keys, noc_scale = |min|
    infos = {int(k): v for k, v in stored.items()}
    noc_scale = abs(np.array([infos[2][k] for k in ("min_x", "min_y", "min_z")], dtype=np.float32))
    assert np.array_equal(noc_scale, np.abs(half.min(0)))
    fps = pickle.load(open(fps_path, "rb"))
    assert sorted(fps) == [2, 7] and all(v.dtype == np.float32 and v.shape == (4, 3) for v in fps.values())
    assert np.array_equal(fps[7], mc.fps(other * np.float32(0.5), 4)[1])

    # an existing pickle is refused; nothing is touched
    before = (info_path.read_bytes(), fps_path.read_bytes())
    assert prep_models.main([str(tmp_path), "--fps", "4"]) == 1
    assert "already exists" in capsys.readouterr().err and before == (info_path.read_bytes(), fps_path.read_bytes())
    # an existing models_info.json without --force: stored beside computed, the file stays; the pickle goes where it is asked to
    alt = tmp_path / "alt.pkl"
    assert prep_models.main([str(tmp_path), "--fps", "3", "--fps-out", str(alt)]) == 0
    out = capsys.readouterr().out
    assert out.count("stored in models_info.json") == 2 and "left as it is" in out and info_path.read_bytes() == before[0]
    assert pickle.load(open(alt, "rb"))[2].shape == (3, 3)
    # --force overwrites both (scale 1 now)
    assert prep_models.main([str(tmp_path), "--fps", "5", "--force"]) == 0
    capsys.readouterr()
    assert json.load(open(info_path))["2"]["min_z"] == -30.0 and pickle.load(open(fps_path, "rb"))[2].shape == (5, 3)
    # more points than an object has vertices: refused with the object named
    assert prep_models.main([str(tmp_path), "--fps", "6", "--force"]) == 1
    assert "(2, 5)" in capsys.readouterr().err
    # --fps 0: the info file alone
    only = tmp_path / "only.json"
    assert prep_models.main([str(tmp_path), "--fps", "0", "--info-out", str(only), "--fps-out", str(tmp_path / "none.pkl")]) == 0
    capsys.readouterr()
    assert only.exists() and not (tmp_path / "none.pkl").exists()
    with pytest.raises(FileNotFoundError):
        prep_models.main([str(tmp_path / "empty")])


# ---- the tied cases: exact, spanning the merge level they name, and telling every planted mistake from the definition ----

@pytest.fixture(scope="module")
def tied():
    """name -> the case with the oracle's answers on it: computed once, shared, read only."""
    from types import SimpleNamespace

    from lc_amd import models

    out = {}
    for name, c in mc.tied_cases(models.DIAM_TILE, models.FPS_RESIDENT).items():
        ties = []
        idx, pts = mc.fps(c.verts, c.fps_count, ties=ties)
        top, pairs = mc.maximal_pairs(c.verts)
        out[name] = SimpleNamespace(case=c, tile=models.DIAM_TILE, diameter=mc.diameter(c.verts), idx=idx, pts=pts, ties=ties, top=top, pairs=pairs)
    return out


def _d2_64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a - b) ** 2).sum(-1)


def test_tied_case_names():
    from lc_amd import models

    assert tuple(mc.tied_cases(models.DIAM_TILE, models.FPS_RESIDENT)) == mc.TIED_NAMES


@pytest.mark.parametrize("name", mc.TIED_NAMES)
def test_tied_cases_are_exact(tied, name):
    """Every coordinate is an integer of at most 72 lattice steps, so every d2 is an integer below 3 * 144^2 < 2^24 in lattice units:
    exact in fp32 whatever the order.  Beside that argument, the fp64 value itself: of every pair of a mesh up to 2500 vertices, of every
    pair that touches a vertex of a maximal pair in a larger one, and of every distance the selection compares."""
    t = tied[name]
    v = t.case.verts
    steps = v.astype(np.float64) * 2.0 ** mc.LATTICE_BITS
    assert v.dtype == np.float32 and np.array_equal(steps, np.round(steps)) and np.abs(steps).max() <= 72
    rows = np.arange(len(v)) if len(v) <= 2500 else np.unique(np.asarray(t.pairs).ravel())
    for r0 in range(0, len(rows), 256):
        r = rows[r0:r0 + 256]
        assert np.array_equal(mc.d2(v[r, None], v[None]).astype(np.float64), _d2_64(v[r, None], v[None]))
    lo, hi = mc.extents(v)
    c32, c64 = (lo + hi) * np.float32(0.5), (lo.astype(np.float64) + hi) * 0.5
    assert np.array_equal(c32.astype(np.float64), c64)
    m32, m64 = mc.d2(v, c32), _d2_64(v, c64)
    for k in t.idx:
        assert np.array_equal(m32.astype(np.float64), m64) and m32.argmax() == k
        m32, m64 = np.minimum(m32, mc.d2(v, v[k])), np.minimum(m64, _d2_64(v, v[k]))


@pytest.mark.parametrize("name", mc.TIED_NAMES)
def test_tied_cases_span_the_merge_they_name(tied, name):
    t = tied[name]
    c = t.case
    d, pair = t.diameter
    assert pair == min(t.pairs) and d == np.sqrt(t.top, dtype=np.float32) and mc.diameter_tiled(c.verts, t.tile) == (d, pair)
    if c.pair is not None:
        assert pair == c.pair
    tiles = sorted({mc.tile_number(i, j, t.tile) for i, j in t.pairs})
    print(f"{name}: {len(c.verts)} vertices, {len(t.pairs)} maximal pairs in {len(tiles)} tiles (numbers {tiles[0]}..{tiles[-1]}), pair {pair}: {c.forces}")
    if c.spans is not None:
        assert c.spans(t.pairs)
    if c.fps_spans:
        waves = [len({(int(i) // mc.WAVE) % (mc.POINT_THREADS // mc.WAVE) for i in tie}) for tie in t.ties]
        slots = [len({int(i) // mc.POINT_THREADS for i in tie}) for tie in t.ties]
        ok = [n for n in range(len(t.ties)) if ("waves" not in c.fps_spans or waves[n] >= 2) and ("slots" not in c.fps_spans or slots[n] >= 2)]
        assert ok, (waves, slots)
        n = ok[0]
        print(f"{name}: pick {n} has {len(t.ties[n])} tied maxima from index {t.ties[n][0]} to {t.ties[n][-1]}, in {waves[n]} waves and {slots[n]} slots; taken: {t.idx[n]}")
        assert t.idx[n] == t.ties[n][0]
    if name == "all-identical":
        lo, hi = mc.extents(c.verts)
        assert d == 0 and pair == (0, 1) and np.array_equal(lo, hi) and not t.idx.any() and len(t.pairs) == len(c.verts) * (len(c.verts) - 1) // 2


@pytest.mark.parametrize("name", mc.TIED_NAMES)
def test_every_planted_mistake_changes_the_answer(tied, name):
    """The inputs discriminate: a kernel with one of the case's mistakes could not give the oracle's answer on it."""
    t = tied[name]
    c = t.case
    assert c.mistakes and set(c.mistakes) <= set(mc.DIAMETER_MISTAKES + mc.FPS_MISTAKES)
    for m in c.mistakes:
        if m in mc.DIAMETER_MISTAKES:
            wrong = mc.diameter(c.verts, mistake=m, tile=t.tile)
            print(f"{name}: {m} gives pair {wrong[1]}, diameter {float(wrong[0])} for {t.diameter[1]}, {float(t.diameter[0])}")
            assert wrong != t.diameter
        else:
            wrong = mc.fps(c.verts, c.fps_count, mistake=m)[0]
            n = int(np.flatnonzero(wrong != t.idx)[0]) if (wrong != t.idx).any() else None
            print(f"{name}: {m} first differs at pick {n}")
            assert n is not None and wrong[n] != t.idx[n]


def test_every_mistake_is_detected_by_a_case_and_none_is_on_by_default():
    from lc_amd import models

    T, R = models.DIAM_TILE, models.FPS_RESIDENT
    listed = {m for c in mc.tied_cases(T, R).values() for m in c.mistakes}
    assert listed == set(mc.DIAMETER_MISTAKES + mc.FPS_MISTAKES)
    with pytest.raises(ValueError):
        mc.diameter(mc.cloud(5, 1), mistake="none")
    with pytest.raises(ValueError):
        mc.fps(mc.cloud(5, 1), 2, mistake="none")

    def fps_as_it_was(v, count):
        lo, hi = mc.extents(v)
        mind = mc.d2(v, (lo + hi) * np.float32(0.5))
        idx = np.empty(count, np.int32)
        for n in range(count):
            idx[n] = k = int(mind.argmax())
            mind = np.minimum(mind, mc.d2(v, v[k]))
        return idx

    for name, (v, counts, want_d) in mc.named_cases(T, R).items():
        d, pair = mc.diameter(v)
        assert mc.diameter(v, mistake=None, tile=T) == (d, pair) == mc.diameter_tiled(v, T), name
        if 1 < len(v) <= 1100:  # the definition by enumeration: the smallest (i, j) among the pairs of the largest d2
            top, pairs = mc.maximal_pairs(v)
            assert pair == min(pairs) and d == np.sqrt(top, dtype=np.float32), name
        idx, pts = mc.fps(v, max(counts), mistake=None)
        assert np.array_equal(idx, fps_as_it_was(v, max(counts))) and np.array_equal(pts, v[idx]), name
