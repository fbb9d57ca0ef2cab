"""The oriented-box library without a GPU (lc_amd/csrc/obox/, include/lc_amd_obox.h, lc_amd/obox.py): its place in the build, header =
exports = ctypes table, its constants, what the compiler made of the four kernels, the workspace formula, every host refusal of the entry
point reached with host pointers (nothing launches), the wrappers' refusals, the properties of the definition on the numpy oracle, the
format of the reference's shipped models_xform.json and of `to_models_xform`, the tool's `--xform` flags, and the conditions
tests/test_gpu_obox.py relies on."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import obox_cases as cases
from tests import obox_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "models_xform_ycbv.json")
F32 = np.float32


def test_the_library_joins_the_third_tuple_behind_shade():
    import __graft_entry__ as entry
    from lc_amd import build, obox

    T = build.OBOX
    assert build.EXTRA_TARGETS[:2] == (build.SHADE, T) and T not in build.TARGETS + build.LATER_TARGETS
    assert T == build._side("obox") and T.shared == ()
    assert T.src_dir == os.path.join(build.CSRC, "obox") and T.header == "lc_amd_obox.h" and T.hash_marker == b"LC_AMD_OBOX_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_obox.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_obox.so " in doc and "lc_amd/csrc/obox/ " in doc and "include/lc_amd_obox.h " in doc
    entry.build()  # through build_later
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = obox.load()
    assert lib.lc_amd_obox_version() == 1
    assert lib.lc_amd_obox_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    every = build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS
    for other in every:  # no other library sees this one's directory or header, or carries its marker, and the reverse
        if other is T:
            continue
        assert not any("obox" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    assert {os.path.normpath(d) for d in build._deps(T)} == {os.path.join(T.src_dir, "lc_obox.hip"), os.path.join(ROOT, "include", T.header)}
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_obox.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_OBOX_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and not re.search(r"\b(sinf?|cosf?|acosf?|atan2f?|expf?|powf?)\s*\(", code)  # no libm on the device
    assert "lc_amd.obox" in __import__("lc_amd").__doc__


def test_header_exports_constants_and_the_ctypes_table_agree():
    from lc_amd import build, obox

    T = build.OBOX
    obox.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(obox._SIGNATURES) and {"lc_obox_search_f32", "lc_obox_workspace_bytes"} <= declared and len(declared) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    m = re.search(r"int lc_obox_search_f32\((.*?)\);", text, flags=re.S)
    kinds = ["p" if "*" in a else {"int": "i", "size_t": "z"}[a.split()[0]] for a in m.group(1).split(",")]
    res, args = obox._SIGNATURES["lc_obox_search_f32"]
    of = {ctypes.c_void_p: "p", ctypes.POINTER(ctypes.c_int): "p", ctypes.c_int: "i", ctypes.c_size_t: "z"}
    assert res is ctypes.c_int and kinds == [of[a] for a in args]
    define = lambda name: int(re.search(rf"#define {name} (\d+)\n", header).group(1))
    assert define("LC_AMD_OBOX_VERSION") == 1
    assert (define("LC_OBOX_TILE"), define("LC_OBOX_SPLIT")) == (obox.TILE, obox.SPLIT) == (cases.TILE, cases.SPLIT)
    assert (define("LC_OBOX_MAX_LEVELS"), define("LC_OBOX_MAX_CAND")) == (obox.MAX_LEVELS, obox.MAX_CAND)
    assert define("LC_OBOX_STEP0_DEG") == obox.STEP0_DEG == 9 and obox.STEP0 == oracle.STEP0 == np.pi / 20
    assert define("LC_OBOX_GRID_RADIUS") == obox.GRID_RADIUS == oracle.GRID_RADIUS
    assert define("LC_OBOX_LEVEL0_COUNT") == obox.LEVEL0_COUNT == len(oracle.level_vectors(None, 0)) == 1419
    assert define("LC_OBOX_AXIS_LEVEL0_COUNT") == obox.AXIS_LEVEL0_COUNT == oracle.AXIS_LEVEL0_COUNT == len(oracle.level_vectors(1, 0))
    assert obox.DEFAULT_LEVELS == oracle.DEFAULT_LEVELS == 6
    # the level-0 counts the GPU cases meet are no multiples of the wave or of a workgroup's candidates
    assert obox.LEVEL0_COUNT % 64 and obox.LEVEL0_COUNT % 128 and obox.AXIS_LEVEL0_COUNT % 64 and 125 % 64


def test_four_kernels_without_scratch_or_spills(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, obox

    obox.load()
    res = kernel_resources(build.OBOX.so_path)
    assert len(res) == 4, sorted(res)
    for short, threads, lds in (("lc_obox_init_kernel", 256, 0), ("lc_obox_score_kernel", 128, 16 * obox.TILE), ("lc_obox_pick_kernel", 64, 0),
                                ("lc_obox_finish_kernel", 64, 0)):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == threads and d.get("group_segment_fixed_size", 0) == lds, short


def test_the_tables_are_the_stated_ones():
    from lc_amd import obox

    for axis in (None, 0, 1, 2):
        deltas, n0, n1 = obox.delta_table(axis, 3)
        assert (n0, n1) == ((1419, 125) if axis is None else (10, 5)) and deltas.shape == (n0 + 3 * n1, 4) and deltas.dtype == np.float64
        want = np.concatenate([oracle.level_quats(axis, l) for l in range(4)])
        assert np.array_equal(deltas.view(np.int64), want.view(np.int64)), axis  # two statements of the same arithmetic
        assert np.abs(np.linalg.norm(deltas, axis=1) - 1).max() < 1e-15
        for level in range(3):
            vec = oracle.level_vectors(axis, level)
            assert vec[0] == (0, 0, 0) and len(set(vec)) == len(vec)
            assert tuple(deltas[0 if level == 0 else n0 + (level - 1) * n1]) == (1.0, 0.0, 0.0, 0.0)
            if axis is None or level > 0:
                assert {tuple(-c for c in p) for p in vec} == set(vec)  # symmetric under negation
                assert [oracle._n2(p) for p in vec] == sorted(oracle._n2(p) for p in vec)
            if axis is not None:
                others = [a for a in range(3) if a != axis]
                assert all(p[a] == 0 for p in vec for a in others)
                q = deltas[:n0] if level == 0 else deltas[n0 + (level - 1) * n1:n0 + level * n1]
                assert not q[:, [1 + a for a in others]].any()  # exactly zero
        assert obox.delta_table(axis, 0)[0].shape == (n0, 4)
    assert obox.delta_table("y", 1)[0].tolist() == obox.delta_table(1, 1)[0].tolist()
    vec = oracle.level_vectors(None, 0)
    assert max(oracle._n2(p) for p in vec) == 49 and [p for p in vec if oracle._n2(p) == 1] == [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    assert [p[2] for p in oracle.level_vectors(2, 0)] == list(range(10)) and [p[0] for p in oracle.level_vectors(0, 2)] == [0, -1, 1, -2, 2]
    # the ball of 63 degrees holds every orientation modulo the cube's rotations: the farthest turns by 2 acos((2 + sqrt 2) / 4) = 62.8 degrees
    assert 62.79 < np.degrees(2 * np.arccos((2 + np.sqrt(2)) / 4)) < 62.81 < 7 * 9
    for bad in (3, -1, "w", 1.0, True):
        with pytest.raises(ValueError, match="axis must be None, 0, 1, 2 or 'x', 'y', 'z'"):
            obox.delta_table(bad, 1)
    for bad in (-1, 17, 2.0, None, True):
        with pytest.raises(ValueError, match="levels must be an integer in 0..16"):
            obox.delta_table(None, bad)


def test_workspace_formula():
    from lc_amd import obox

    lib = obox.load()
    assert lib.lc_obox_workspace_bytes(0, 10) == 0 and lib.lc_obox_workspace_bytes(3, 0) == 0 and obox.workspace_bytes(0) == 0
    for n, c in ((1, 1), (1, 1419), (3, 125), (4, 10), (5, 5), (21, 1419)):
        assert lib.lc_obox_workspace_bytes(n, c) == 32 * n + -(-4 * n // 16) * 16 + 24 * n * c, (n, c)
    for n in (1, 4, 21):
        assert obox.workspace_bytes(n) == lib.lc_obox_workspace_bytes(n, 1419) == obox.workspace_bytes(n, None, 0)
        assert obox.workspace_bytes(n, "z", 2) == lib.lc_obox_workspace_bytes(n, 10) == obox.workspace_bytes(n, 0, 0)


def test_every_refusal_comes_before_any_launch():
    """Host memory stands in for every device pointer, so a call that got as far as a launch could not return its argument error."""
    from lc_amd import obox

    lib = obox.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    table = (ctypes.c_int * 8)(0, 10, 0, 0, 10, 5, 0, 0)  # two meshes: 10 and 5 vertices
    err = lambda: lib.lc_amd_obox_last_error().decode()
    big = 1 << 30

    def call(verts=p, total=15, tab=p, host=table, n=2, mv=10, deltas=p, n0=7, n1=5, levels=2, xform=p, scale=p, vol=p, aabb=p, path=p, info=p, ws=p, wsb=big):
        return lib.lc_obox_search_f32(verts, total, tab, host, n, mv, deltas, n0, n1, levels, xform, scale, vol, aabb, path, info, ws, wsb, None)

    for n in (0, -1, 65536):
        assert call(n=n) != 0 and "n_meshes must be in 1..65535" in err()
    assert call(total=0) != 0 and "total_verts must be positive" in err()
    assert call(mv=0) != 0 and "max_verts must be positive" in err()
    assert call(mv=(1 << 30) // 3 * 2) != 0 and "2^31" in err()
    for levels in (-1, 17):
        assert call(levels=levels) != 0 and "levels must be in 0..16" in err()
    for n0 in (0, 65537):
        assert call(n0=n0) != 0 and "n_level0 must be in 1..65536" in err()
    for n1 in (0, 65537):
        assert call(n1=n1) != 0 and "n_refine must be in 1..65536" in err()
        assert call(n1=n1, levels=0, wsb=0) != 0 and "workspace too small" in err()  # without refinement its count is not judged
    for kw in (dict(verts=None), dict(tab=None), dict(host=None), dict(deltas=None)):
        assert call(**kw) != 0 and "null pointer" in err()
    for k in ("xform", "scale", "vol", "aabb", "path", "info"):
        assert call(**{k: None}) != 0 and "null output" in err(), k
    assert call(mv=9) != 0 and "mesh 0" in err() and "max_verts" in err()
    assert call(host=(ctypes.c_int * 8)(0, 10, 0, 0, -1, 5, 0, 0)) != 0 and "mesh 1" in err()
    assert call(host=(ctypes.c_int * 8)(0, 0, 0, 0, 0, 5, 0, 0)) != 0 and "mesh 0" in err()
    assert call(total=14) != 0 and "mesh 1: vertices 10 + 5 end behind total_verts 14" in err()
    assert call(n=65535, host=(ctypes.c_int * (4 * 65535))(*([0, 1, 0, 0] * 65535)), n0=65536) != 0 and "2^31 extrema slots or more" in err()
    assert call(ws=None) != 0 and "workspace is null" in err()
    need = lib.lc_obox_workspace_bytes(2, 7)
    assert need == 64 + 16 + 24 * 2 * 7 and call(wsb=need - 1) != 0 and "workspace too small" in err()
    assert call(n1=9, wsb=need) != 0 and "workspace too small" in err()  # the larger of the two tables sizes it
    assert call(ws=p + 8) != 0 and "workspace not 16-byte aligned" in err()
    assert call(deltas=p + 4) != 0 and "deltas not 8-byte aligned" in err()
    for k in ("verts", "tab", "xform", "scale", "vol", "aabb", "path", "info"):
        assert call(**{k: p + 2}) != 0 and "pointer not 4-byte aligned" in err(), k


def test_wrapper_refusals():
    from lc_amd import obox

    with pytest.raises(TypeError, match="meshes must be a MeshSet"):
        obox.oriented_box([cases.mesh("cloud:65")])
    with pytest.raises(ValueError, match="xform must be"):
        obox.to_models_xform(oracle.Box(np.zeros((2, 3, 4), F32), np.zeros((2, 3), F32), None, None, None, None, None), [1, 2])
    box = cases.reference("cloud:65")
    for ids in ([], [1, 2]):
        with pytest.raises(ValueError, match="object ids for 1 meshes"):
            obox.to_models_xform(box, ids)


@pytest.mark.parametrize("axis", [None, 0, 1, 2])
def test_the_definition_s_properties_on_the_oracle(axis):
    for name in ("cloud:65", "cloud:257", "cloud:1025", "offgrid:0", "offgrid:3", "tie-cube"):
        v, r = cases.mesh(name), cases.reference(name, axis)
        X, scale, path = r.xform[0], r.noc_scale[0], r.path[0]
        assert path.shape == (7,) and r.info[0] == 0
        # the score never rises along the path, and starts at or below the identity's
        won = [r.scores[0][l][path[l]] for l in range(7)]
        assert all(b <= a for a, b in zip(won, won[1:])) and won[0] <= r.aabb_volume[0] and won[-1] == r.volume[0] <= r.aabb_volume[0], name
        assert all(r.scores[0][l][0] == won[l - 1] for l in range(1, 7)), name  # candidate 0 IS the winner before: the same bits
        e = v.max(0) - v.min(0)
        assert r.scores[0][0][0] == r.aabb_volume[0] == (e[0] * e[1]) * e[2] and e.dtype == F32, name  # the identity is exact: the mesh's own box
        for l in range(7):  # lowest score, lowest index among equals
            s = r.scores[0][l]
            assert s[path[l]] == s.min() and path[l] == int(np.nonzero(s == s.min())[0][0]), (name, l)
        # a rigid transform: orthonormal to fp32's rounding, determinant +1, last row 0 0 0 1
        R = X[:3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6 and X[3].tolist() == [0, 0, 0, 1], name
        # the enclosure holds exactly in fp32, and the box is tight: some vertex touches every face
        q = oracle.transformed(X, v)
        assert q.dtype == F32 and (np.abs(q) <= scale).all() and (np.abs(q).max(0) == scale).all() and (scale > 0).all(), name
        lo, hi = oracle.extents(X[:3, :3], v)
        assert r.volume[0] == ((hi - lo)[0] * (hi - lo)[1]) * (hi - lo)[2]
        if axis is not None:  # the chosen axis' row and column stay at the unit vector
            unit = np.eye(3, dtype=F32)[axis]
            assert np.array_equal(X[axis, :3], unit) and np.array_equal(X[:3, axis], unit), (name, axis)
    assert cases.reference("cloud:1025", axis).volume[0] < 0.9 * cases.reference("cloud:1025", axis).aabb_volume[0]  # the search finds something


def test_a_box_turned_by_the_inverse_of_a_grid_rotation_is_recovered_by_that_candidate():
    """The corners of an axis-aligned box turned by R_k^T, R_k the fp32 matrix of level-0 candidate k: the level-0 search gives exactly the
    score of candidate k, which is the box's own volume up to fp32's rounding.  (Candidates of small angle only: one near the rim of the
    ball has a second member of its class modulo the cube's rotations inside the ball, which scores the same box within a rounding.)"""
    _, mats = oracle.level_matrices((1.0, 0.0, 0.0, 0.0), None, 0)
    true = 8 * float(np.prod(cases.BOX_HALF))
    for k in (0, 5, 77, 400, 1000):
        v = (cases.box_corners() @ mats[k].astype(np.float64)).astype(F32)  # rows R^T b
        r = oracle.oriented_box_host([v], None, 0)
        assert r.volume[0] == r.scores[0][0][k] == oracle.score(mats[k], v) and abs(r.volume[0] / true - 1) < 1e-5, k
        assert k == 0 or r.volume[0] < 0.8 * r.aabb_volume[0], k


def test_degenerate_meshes_keep_the_identity():
    """A mesh whose box under the identity has volume 0 -- one vertex, or 2, 3 or many vertices flat along a model axis -- meets 0, the lowest
    score there is, at candidate 0 of every level.  (Two or three vertices in general position span a box of positive volume under the identity
    and are searched like any mesh: tests/test_gpu_obox.py has them among its sizes.)"""
    flat_names = [("flat", cases.mesh("flat")), ("V=1", cases.cloud(1))] + [(f"flat V={n}", cases.mesh("flat")[:n]) for n in (1, 2, 3)]
    for axis in (None, 1):
        for name, v in flat_names:
            r = oracle.oriented_box_host([v], axis)
            assert not r.path.any() and r.volume[0] == 0 == r.aabb_volume[0] and np.array_equal(r.xform[0, :3, :3], np.eye(3, dtype=F32)), name
            assert all(s[0] == 0 and (s >= 0).all() for s in r.scores[0]), name
            lo, hi = v.min(0), v.max(0)
            assert np.array_equal(-r.xform[0, :3, 3], (lo + hi) * F32(0.5)) and (np.abs(oracle.transformed(r.xform[0], v)) <= r.noc_scale[0]).all(), name
    assert all((s == 0).all() for s in oracle.oriented_box_host([cases.cloud(1)]).scores[0])  # one vertex: every candidate ties
    assert cases.reference("cloud:2").path[0, 0] > 0 and cases.reference("cloud:3").aabb_volume[0] > 0
    # a flat mesh turned off the axes has a box of positive volume under the identity and is laid flat again (volume far below it)
    tilted = (cases.mesh("flat").astype(np.float64) @ cases.rotation((20.0, 10.0, -35.0)).T).astype(F32)
    r = oracle.oriented_box_host([tilted])
    assert 0 < r.volume[0] < 0.01 * r.aabb_volume[0] and r.path[0, 0] != 0
    nan = np.array(cases.cloud(65))
    nan[17, 1] = np.nan
    assert oracle.oriented_box_host([nan, cases.cloud(65)]).info.tolist() == [1, 0]


def test_the_conditions_the_gpu_cases_rely_on():
    # the tie case: two level-0 candidates of different index share the LOWEST score, and the lower index wins
    for levels in (0, oracle.DEFAULT_LEVELS):
        r = cases.reference("tie-cube", None, levels)
        s = r.scores[0][0]
        tied = np.nonzero(s == s.min())[0]
        vec = oracle.level_vectors(None, 0)
        assert len(tied) == 2 and [vec[k] for k in tied] == [(0, 0, -5), (0, 0, 5)] and r.path[0, 0] == tied[0] > 0
    s = cases.reference("tie-cube", 2, 0).scores[0][0]
    assert len(set(s.tolist())) < len(s)  # ties below the winner in axis mode too
    # the sizes straddle one wave, the LDS tile and the vertex split, and one has three chunks
    assert {63, 64, 65, cases.TILE - 1, cases.TILE, cases.TILE + 1, cases.SPLIT - 1, cases.SPLIT, cases.SPLIT + 1} < set(cases.SIZES)
    assert max(cases.SIZES) > 2 * cases.SPLIT and max(cases.SIZES) % cases.TILE
    # the searches of the larger clouds move at every level kind: a kernel that ignored the base or a table would be seen
    for V in (257, 1025):
        path = cases.reference(f"cloud:{V}").path[0]
        assert path[0] > 0 and (path[1:] > 0).sum() >= 3, (V, path)
    # off-grid boxes: the recovered volume exceeds the true one by well under a percent (recorded: profiles/obox/offgrid_ratio.json)
    true = np.prod(np.asarray(cases.BOX_HALF, np.float64) * 2)
    recorded = json.load(open(os.path.join(ROOT, "profiles", "obox", "offgrid_ratio.json")))
    for i in range(len(cases.OFF_GRID)):
        r = cases.reference(f"offgrid:{i}")
        ratio = float(r.volume[0]) / true
        assert 1 - 1e-5 < ratio < float(r.aabb_volume[0]) / true
        # the record is the oracle's figure; where another host's libm rounds a table entry the other way a score moves by an fp32 rounding
        # (1e-7), and a path that flips between two near-equal candidates moves the volume by no more than they differ: far below 1e-4
        assert recorded["rows"][i]["rotvec_deg"] == list(cases.OFF_GRID[i]) and abs(recorded["rows"][i]["volume_over_true"] - ratio) < 1e-4


def test_the_shipped_file_has_the_format_and_the_invariants_this_project_writes():
    """tests/golden/models_xform_ycbv.json is the reference's shipped file (settings only), read as model_transform.py:35-37 reads it."""
    from lc_amd import obox

    shipped = json.load(open(GOLDEN))
    assert len(shipped) == 12 and all(re.fullmatch(r"\d+", k) for k in shipped)
    names = [f"cloud:{V}" for V in (65, 257)]
    ours = obox.to_models_xform(oracle.Box(*(np.concatenate([getattr(cases.reference(n), f) for n in names]) for f in cases.FIELDS), None), [4, 9])
    ours = json.loads(json.dumps(ours))
    assert list(ours) == ["4", "9"]
    for entries in (shipped, ours):
        for k, e in entries.items():
            assert sorted(e) == ["xform", "xformed_noc_scale"] and len(e["xform"]) == 16 and len(e["xformed_noc_scale"]) == 3, k
            assert all(type(x) is float for x in e["xform"] + e["xformed_noc_scale"]) or entries is shipped, k
            assert all(isinstance(x, (int, float)) for x in e["xform"] + e["xformed_noc_scale"]), k
            X = np.array(e["xform"], dtype=np.float32).reshape(4, 4)
            scale = np.array(e["xformed_noc_scale"], dtype=np.float32)
            R = X[:3, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6, k
            assert X[3].tolist() == [0, 0, 0, 1] and (scale > 0).all(), k
    # objects 5 and 7 of the shipped file are turned about z alone: the form of axis mode
    for k in ("5", "7"):
        X = np.array(shipped[k]["xform"], dtype=np.float32).reshape(4, 4)
        assert np.array_equal(X[2, :3], [0, 0, 1]) and np.array_equal(X[:3, 2], [0, 0, 1]) and X[0, 1] != 0


def test_the_json_round_trip_gives_back_the_float32_bits():
    from lc_amd import obox

    odd = np.array([0.1, -0.0, 1e-38, 1e-45, 3.4028235e38, 1 / 3, -2.5e-7, 1.0], F32)
    box = oracle.Box(np.concatenate([odd, odd[::-1]]).reshape(1, 4, 4), odd[None, 3:6], None, None, None, None, None)
    for b, ids in ((box, [3]), (cases.reference("cloud:1025"), [15]), (cases.reference("offgrid:1", 2), [0])):
        back = json.loads(json.dumps(obox.to_models_xform(b, ids), indent=2))[str(ids[0])]
        assert cases.same_bits(np.array(back["xform"], dtype=np.float32).reshape(4, 4), b.xform[0])
        assert cases.same_bits(np.array(back["xformed_noc_scale"], dtype=np.float32), b.noc_scale[0])
        assert cases.same_bits(np.array([np.float32(x) for x in back["xform"]]), b.xform[0].reshape(16))


def _write_ply(path, v):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face 0\nproperty list uchar int vertex_indices\nend_header\n")
        for p in v:
            fh.write(" ".join(repr(float(c)) for c in p) + "\n")


class _HostSet:
    def __init__(self, meshes, obj_ids):
        self.meshes, self.obj_ids = [np.asarray(v, F32) for v, _ in meshes], obj_ids


def test_the_tool_writes_models_xform_json_only_when_asked(tmp_path, monkeypatch, capsys):
    import torch

    from lc_amd import models, obox, prep_models

    a, b = np.array(cases.cloud(65)), np.array(cases.turned_box(cases.OFF_GRID[3]))
    _write_ply(tmp_path / "obj_000003.ply", a)
    _write_ply(tmp_path / "obj_000011.ply", b)
    seen = []

    def host_box(ms, *, axis=None, levels=6):
        seen.append(axis)
        r = oracle.oriented_box_host(ms.meshes, obox._axis(axis), levels)
        return obox.OrientedBox(*(torch.from_numpy(getattr(r, f)) for f in cases.FIELDS))

    monkeypatch.setattr(prep_models, "_device", lambda: "host")
    monkeypatch.setattr(prep_models, "MeshSet", lambda meshes, device, obj_ids=None: _HostSet(meshes, obj_ids))
    monkeypatch.setattr(models, "prepare", lambda ms, fps: None)
    monkeypatch.setattr(models, "to_models_info", lambda info, ids: {i: dict.fromkeys(prep_models._KEYS, 0.0) for i in ids})
    monkeypatch.setattr(obox, "oriented_box", host_box)
    path = tmp_path / "models_xform.json"
    assert prep_models.main([str(tmp_path), "--fps", "0"]) == 0 and not path.exists() and not seen  # off by default
    assert prep_models.main([str(tmp_path), "--fps", "0", "--xform-axis", "z"]) == 2 and "--xform-axis needs --xform" in capsys.readouterr().err
    assert prep_models.main([str(tmp_path), "--fps", "0", "--xform"]) == 0 and seen == [None]
    out = capsys.readouterr().out
    assert out.count("oriented box volume") == 2 and f"wrote {path}" in out
    stored = json.load(open(path))
    assert list(stored) == ["3", "11"]
    for k, v in (("3", a), ("11", b)):
        want = oracle.oriented_box_host([v])
        assert cases.same_bits(np.array(stored[k]["xform"], dtype=np.float32).reshape(4, 4), want.xform[0])
        assert cases.same_bits(np.array(stored[k]["xformed_noc_scale"], dtype=np.float32), want.noc_scale[0])
    before = path.read_bytes()
    assert prep_models.main([str(tmp_path), "--fps", "0", "--xform"]) == 1 and "already exists" in capsys.readouterr().err and path.read_bytes() == before
    alt = tmp_path / "about_z.json"
    assert prep_models.main([str(tmp_path), "--fps", "0", "--xform", str(alt), "--xform-axis", "z"]) == 0 and seen[-1] == "z"
    X = np.array(json.load(open(alt))["11"]["xform"], dtype=np.float32).reshape(4, 4)
    assert np.array_equal(X[2, :3], [0, 0, 1]) and np.array_equal(X[:3, 2], [0, 0, 1]) and path.read_bytes() == before
    assert prep_models.main([str(tmp_path), "--fps", "0", "--xform", "--xform-axis", "x", "--force"]) == 0 and path.read_bytes() != before
