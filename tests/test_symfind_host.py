"""The symmetry-deviation library without a GPU (lc_amd/csrc/symfind/, include/lc_amd_symfind.h, lc_amd/symfind.py): its place in the build,
header = exports = ctypes table, its constants, what the compiler made of the three kernels, every host refusal of the entry point reached
with host pointers (nothing launches), the properties of the definition on the numpy oracle -- each listed mistake changes its answer on
some case and `mistake=None` is the plain definition, the NaN rule -- the conditions tests/test_gpu_symfind.py relies on, and the two
tools' host logic with the oracle standing in for the device call."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import models_cases
from tests import symfind_cases as cases
from tests import symfind_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_the_library_joins_the_third_tuple_behind_obox():
    import __graft_entry__ as entry
    from lc_amd import build, symfind

    T = build.SYMFIND
    assert build.EXTRA_TARGETS[:3] == (build.SHADE, build.OBOX, T) and T not in build.TARGETS + build.LATER_TARGETS
    assert T == build._side("symfind") and T.shared == () and T.hash_marker == b"LC_AMD_SYMFIND_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_symfind.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_symfind.so " in doc and "lc_amd/csrc/symfind/ " in doc and "include/lc_amd_symfind.h " in doc
    entry.build()  # through build_later
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = symfind.load()
    assert lib.lc_amd_symfind_version() == 1
    assert lib.lc_amd_symfind_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    for other in build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS:  # no other library sees this one's files or carries its marker
        if other is T:
            continue
        assert not any("symfind" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    assert {os.path.normpath(d) for d in build._deps(T)} == {os.path.join(T.src_dir, "lc_symfind.hip"), os.path.join(ROOT, "include", T.header)}
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_symfind.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_SYMFIND_SRC_HASH"}  # no build switch
    assert "asm" not in re.sub(r"//.*", "", source)
    assert "lc_amd.symfind" in __import__("lc_amd").__doc__


def test_header_exports_constants_and_the_ctypes_table_agree():
    from lc_amd import build, symfind

    T = build.SYMFIND
    symfind.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(symfind._SIGNATURES) and {"lc_symfind_deviation_f32", "lc_symfind_workspace_bytes"} <= declared and len(declared) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if " T " in line} == declared
    m = re.search(r"int lc_symfind_deviation_f32\((.*?)\);", text, flags=re.S)
    kinds = ["p" if "*" in a else {"int": "i", "size_t": "z"}[a.split()[0]] for a in m.group(1).split(",")]
    res, args = symfind._SIGNATURES["lc_symfind_deviation_f32"]
    of = {ctypes.c_void_p: "p", ctypes.POINTER(ctypes.c_int): "p", ctypes.c_int: "i", ctypes.c_size_t: "z"}
    assert res is ctypes.c_int and kinds == [of[a] for a in args]
    define = lambda name: int(re.search(rf"#define {name} (\d+)\n", header).group(1))
    assert define("LC_AMD_SYMFIND_VERSION") == 1
    assert define("LC_SYMFIND_TILE") == symfind.TILE == oracle.TILE == cases.T and define("LC_SYMFIND_QUERIES") == symfind.QUERIES == oracle.QUERIES == cases.Q
    lib = symfind.load()
    for n, k in ((1, 1), (3, 5), (7, 384), (0, 4), (4, 0)):
        assert lib.lc_symfind_workspace_bytes(n, k) == symfind.workspace_bytes(n, k) == (0 if n * k == 0 else -(-8 * n * k // 16) * 16)


def test_three_kernels_without_scratch_or_spills(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, symfind

    symfind.load()
    res = kernel_resources(build.SYMFIND.so_path)
    assert len(res) == 3, sorted(res)
    for short, threads, lds in (("lc_symfind_clear_kernel", 256, 0), ("lc_symfind_walk_kernel", 128, 16 * symfind.TILE + 16), ("lc_symfind_finish_kernel", 256, 32)):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == threads and d.get("group_segment_fixed_size", 0) == lds, short


def test_every_host_refusal_before_anything_launches():
    from lc_amd import symfind

    lib = symfind.load()
    err = lambda: lib.lc_amd_symfind_last_error().decode()
    buf = (ctypes.c_double * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    host = (ctypes.c_int * 8)(0, 5, 0, 0, 5, 3, 0, 0)

    def run(**kw):
        a = dict(verts=P, total=8, tab=P, host=host, n=2, mv=5, table=P, rows=4, mi=P, ro=P, rk=P, G=2, max_k=3, qi=None, qo=None, qn=None, tq=0, mq=0, d2=P, aq=P,
                 at=P, info=P, ws=P, wsb=64)
        a.update(kw)
        return lib.lc_symfind_deviation_f32(a["verts"], a["total"], a["tab"], a["host"], a["n"], a["mv"], a["table"], a["rows"], a["mi"], a["ro"], a["rk"], a["G"],
                                            a["max_k"], a["qi"], a["qo"], a["qn"], a["tq"], a["mq"], a["d2"], a["aq"], a["at"], a["info"], a["ws"], a["wsb"], None)

    odd = ctypes.c_void_p(P.value + 2)
    for kw, text in ((dict(n=0), "n_meshes"), (dict(G=0), "n_jobs"), (dict(G=65536), "n_jobs"), (dict(total=0), "total_verts"), (dict(mv=0), "max_verts"),
                     (dict(mv=(1 << 30) // 3 * 2), "2^31"), (dict(rows=0), "total_rows"), (dict(max_k=0), "max_k"), (dict(max_k=5), "max_k"),
                     (dict(verts=None), "null pointer"), (dict(host=None), "null pointer"), (dict(table=None), "null pointer"), (dict(rk=None), "null job array"),
                     (dict(qi=P), "query_off"), (dict(qi=P, qo=P, qn=P), "total_queries"), (dict(qi=P, qo=P, qn=P, tq=4), "max_queries"),
                     (dict(qi=P, qo=P, qn=P, tq=4, mq=5), "max_queries"), (dict(at=None), "null output"), (dict(info=None), "null output"),
                     (dict(mv=4), "mesh 0"), (dict(total=7), "mesh 1"), (dict(host=(ctypes.c_int * 8)(-1, 5, 0, 0, 5, 3, 0, 0)), "mesh 0"),
                     (dict(ws=None), "workspace is null"), (dict(wsb=47), "workspace too small"), (dict(ws=ctypes.c_void_p(P.value + 8)), "16-byte"),
                     (dict(table=ctypes.c_void_p(P.value + 4)), "8-byte"), (dict(mi=odd), "4-byte"), (dict(d2=odd), "4-byte")):
        assert run(**kw) == 1 and text in err(), (kw, err())
    assert lib.lc_symfind_workspace_bytes(2, 3) == 48


def test_wrapper_refusals():
    from lc_amd import symfind

    with pytest.raises(TypeError, match="MeshSet"):
        symfind.deviation([cases.cloud(5, 1)], cases.IDENTITY[None], [0], [0], [1])


def _naive(v, row, queries=None):
    """The definition with scalar loops, one query and one target at a time."""
    m = np.asarray(row, np.float64).reshape(3, 4)
    q = range(len(v)) if queries is None else queries
    best = (F32(-1), -1, -1)
    for i in q:
        if not 0 <= i < len(v):
            continue
        x, y, z = (np.float64(c) for c in v[i])
        p = [F32(((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]) for r in range(3)]
        n, w = F32(np.inf), 0
        for j in range(len(v)):
            dx, dy, dz = (F32(p[c] - v[j][c]) for c in range(3))
            d = F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))
            if d < n:
                n, w = d, j
        if n > best[0]:
            best = (n, int(i), w)
    return best


def test_the_plain_oracle_is_the_definition_and_every_mistake_changes_some_answer():
    for name in ("size:2", "queries:255", "repeats-descending"):
        c = cases.named(name)
        v, want = c.meshes[0][:40], None
        q = None if c.query_idx is None else np.asarray(c.query_idx[:30]) % 40
        for row in c.table:
            got = oracle.deviation_row(v, row, q)
            assert (got[0].tobytes(), got[1], got[2]) == (_naive(v, row, q)[0].tobytes(),) + _naive(v, row, q)[1:], name
    changed = {m: [] for m in oracle.MISTAKES}
    calls = {n: cases.tied(n).call for n in cases.TIED}
    calls.update({n: cases.named(n) for n in ("size:513", "queries:257", "repeats-descending", "all-identical")})
    for name, c in calls.items():
        want = oracle.deviation(c.meshes, *c.args())
        for m in oracle.MISTAKES:
            got = oracle.deviation(c.meshes, *c.args(), mistake=m)
            if not all(cases.same_bits(getattr(got, f), getattr(want, f)) for f in cases.FIELDS):
                changed[m].append(name)
    assert all(changed.values()), changed
    for name, t in ((n, cases.tied(n)) for n in cases.TIED):  # and each tied case tells the mistakes it is listed for
        assert all(name in changed[m] for m in t.mistakes), (name, t.mistakes, {m: name in changed[m] for m in t.mistakes})


def test_the_planted_ties_are_what_the_cases_say():
    for name in cases.TIED:
        t = cases.tied(name)
        c = t.call
        v, q, row = c.meshes[0], c.query_idx, c.table[1]
        D = oracle.d2(oracle.transform(row, v[q]), v)
        n = D.min(1)
        assert n.max() == F32(64 * cases.STEP ** 2) and np.sort(n)[-len(t.plants) - 1] == 0, name
        tied_pos = np.flatnonzero(n == n.max())
        assert sorted(tied_pos.tolist()) == sorted(p for p, _ in t.plants), name  # the planted minima are the strict maximum of the others
        for pos, targets in t.plants:
            assert sorted(np.flatnonzero(D[pos] == n[pos]).tolist()) == sorted(targets), (name, pos)
        want = cases.reference(name)
        pos, targets = min(t.plants)
        assert (int(want.arg_query[0, 1]), int(want.arg_target[0, 1])) == (int(q[pos]), min(targets)), name
        assert want.dev2[0, 0] == 0 and want.arg_query[0, 0] == q[0]  # the identity row: every query tied at 0, position 0 wins
    box = cases.reference("half-turns")
    assert box.dev2.tobytes() == np.zeros((1, 3), F32).tobytes() and (box.arg_query == 0).all()
    assert not np.array_equal(cases.half_turn_rows()[2].reshape(3, 4)[:, :3], np.diag([-1.0, -1.0, 1.0]))  # rodrigues' sin(pi) is in the rows
    same = cases.reference("all-identical")
    assert same.dev2[0].tolist() == [0.0, float(F32(25 * cases.STEP ** 2))] and same.arg_query[0].tolist() == [0, 0] and same.arg_target[0].tolist() == [0, 0]


def test_the_nan_rule_on_the_oracle():
    """A NaN d2 never wins a min: n_i is the least d2 that is no NaN, +inf with target 0 if there is none; the max then meets no NaN."""
    v = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0]], F32)
    d, i, j, _ = oracle.deviation_row(v, cases.IDENTITY, [0, 1, 3])
    assert (float(d), i, j) == (0.0, 0, 0)  # the NaN vertex is a target of every query and wins none
    d, i, j, _ = oracle.deviation_row(v, cases.IDENTITY, None)
    assert (float(d), i, j) == (float("inf"), 2, 0)  # as a query all its d2 are NaN: +inf, target 0, and +inf is the max
    empty = oracle.deviation([np.zeros((0, 3), F32), v], cases.IDENTITY[None], [0, 1], [0, 0], [1, 1], [0, 7, 1], [0, 2], [2, 1])
    assert empty.info.tolist() == [0, 0] and empty.dev2[:, 0].tolist() == [-1.0, 0.0]  # an empty mesh comes before its query list: nothing is skipped
    shift = np.concatenate((np.eye(3), [[0.25], [0], [0]]), 1).reshape(12)
    d, i, j, _ = oracle.deviation_row(v, shift, [0, 1, 3])
    assert (float(d), i, j) == (0.0625, 0, 0)


# ---- the tools' host logic, the oracle standing in for the device call ----

def _frames(name):
    from lc_amd import symfind

    v, kind = cases.tool_mesh(name), cases.TOOL_SHAPES[name][1]
    if kind == "model":
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        return [(lo + 0.5 * (hi - lo), np.eye(3))]
    from tests import obox_oracle

    return [symfind.frame_of_xform(obox_oracle.oriented_box_host([(v, None)], None, 6).xform[0])]


_PROPOSED = {}


def _propose(name):
    from lc_amd import symfind

    if name not in _PROPOSED:
        v, eps = cases.tool_mesh(name), cases.TOOL_SHAPES[name][2]
        dia = float(models_cases.diameter(v)[0])
        _PROPOSED[name] = symfind.propose_symmetries(oracle.scorer([v]), [1], _frames(name), [dia], eps_abs=eps, eps_rel=0.0,
                                                     frame_kind=cases.TOOL_SHAPES[name][1]) + (dia,)
    return _PROPOSED[name]


@pytest.mark.parametrize("name", list(cases.TOOL_SHAPES))
def test_proposals_of_the_shapes_and_their_margins(name):
    from lc_amd import symfind
    from lc_amd.symmetry import models_info_transforms

    _, kind, eps, n_disc, n_cont, closed, truncated = cases.TOOL_SHAPES[name]
    assert 100 <= len(cases.tool_mesh(name)) <= 1600
    proposal, sidecar, dia = _propose(name)
    side = sidecar["objects"]["1"]
    devs = np.array([d for c in side["candidates"] for d in c["turns"] + [e["dev"] for e in c["extra"]]] + [e["dev"] for e in side["elements"]])
    assert len(devs) >= 3 * len(symfind.axis_turns()) and (np.abs(devs - eps) >= 0.1 * eps).all(), (name, np.sort(np.abs(devs - eps))[:3])  # no decision near eps
    out = proposal[1]
    assert len(out.get("symmetries_discrete", ())) == n_disc and len(out.get("symmetries_continuous", ())) == n_cont, (name, side["folds"], side["continuous_axis"])
    assert (side["closed"], side["truncated"]) == (closed, truncated)
    info = {"1": dict(diameter=dia, **out)}
    (R, t), = models_info_transforms(json.loads(json.dumps(info)), None, 384)[1]
    assert len(R) == (1 + n_disc) * (384 if n_cont else 1)
    v = cases.tool_mesh(name)
    report = symfind.check_symmetries(oracle.scorer([v]), [1], info, [dia], eps_abs=eps, eps_rel=0.0)
    assert report["ok"] and symfind.failed_entries(report) == []
    assert len(report["objects"]["1"]["symmetries_discrete"]) == n_disc and len(report["objects"]["1"]["symmetries_continuous"]) == n_cont
    if n_disc or n_cont:
        spoilt = {"1": cases.spoil_turn(info["1"]) if n_disc else cases.spoil_axis(info["1"])}
        bad = symfind.check_symmetries(oracle.scorer([v]), [1], spoilt, [dia], eps_abs=eps, eps_rel=0.0)
        assert not bad["ok"] and symfind.failed_entries(bad) == ["obj 1 symmetries_discrete[0]" if n_disc else "obj 1 symmetries_continuous[0]"]
        worst = [e for k in ("symmetries_discrete", "symmetries_continuous") for e in bad["objects"]["1"][k] if not e["ok"]][0]
        assert worst["dev"] >= 1.1 * eps


def test_the_fast_scorer_is_the_definition_on_the_tools_shapes():
    from lc_amd import symfind

    for name in ("square-prism", "revolution-cone"):
        v = cases.tool_mesh(name)
        c = 0.5 * (v.min(0).astype(np.float64) + v.max(0))
        rows = np.stack([symfind.turn_row(np.eye(3)[a], c, ang) for a in range(3) for _, ang in symfind.axis_turns()[::37]])
        fast, full = oracle.scorer([v])([(0, rows, None)])[0], oracle.scorer([v], fast=False)([(0, rows, None)])[0]
        assert np.array_equal(fast, full), name


def test_turns_closure_and_the_cap():
    from lc_amd import symfind

    turns = symfind.axis_turns(12, 384)
    labels = [l for l, _ in turns]
    assert labels[:383] == [("s", s) for s in range(1, 384)] and len(set(labels)) == len(labels)
    extra = [(l[1], l[2]) for l in labels[383:]]
    assert extra == [(n, k) for n in range(2, 13) for k in range(1, n) if (384 * k) % n] and {n for n, _ in extra} == {5, 7, 9, 10, 11}
    for n in range(2, 13):
        at = symfind._fold_positions(turns, n, 384)
        assert np.allclose([turns[i][1] for i in at], [2 * math.pi * k / n for k in range(1, n)], rtol=0, atol=1e-15)
    c = np.array([3.0, -2.0, 5.0])
    quarter = [symfind.turn_row(np.eye(3)[a], c, math.pi / 2 * k) for a in range(3) for k in (1, 2, 3)]
    group, truncated = symfind.close_group(quarter)
    assert len(group) == 23 and not truncated and len(symfind.close_group(quarter[:3] + [quarter[4], quarter[7]])[0]) == 7
    assert all(symfind.same(symfind.compose(g, inv), symfind._IDENTITY) for g, inv in zip(group, symfind.inverse_rows(group)))
    capped, truncated = symfind.close_group(quarter, cap=10)
    assert truncated and len(capped) == 10 and all(symfind.same(a, b) for a, b in zip(capped, group))
    fifth = [symfind.turn_row(np.eye(3)[2], c, 2 * math.pi / 5), symfind.turn_row(np.eye(3)[0], c, 2 * math.pi / 5)]  # generate the 59 rotations of an icosahedron
    group, truncated = symfind.close_group(fifth)
    assert len(group) == symfind.MAX_DISCRETE == 47 and truncated


def test_a_closure_element_above_eps_is_dropped_and_reported():
    """On the tilted cuboid eps accepts the half turns about x and y and not their product, the half turn about z: the proposal keeps the two,
    drops the third, says `closed: false`, and the file still reads back."""
    from lc_amd import symfind
    from lc_amd.symmetry import models_info_transforms

    proposal, sidecar, dia = _propose("cuboid-tilted")
    side = sidecar["objects"]["1"]
    assert side["closed"] is False and side["truncated"] is False and side["continuous_axis"] is None and side["folds"] == [2, 2, 0]
    assert [(e["candidate"], e["kept"]) for e in side["elements"]] == [(True, True), (True, True), (True, False)]
    assert side["elements"][2]["dev"] > 1.1 * side["eps"] and side["elements"][2]["dev"] == side["candidates"][2]["turns"][191]
    kept = np.asarray(proposal[1]["symmetries_discrete"]).reshape(-1, 4, 4)
    c = np.asarray(side["frame"]["centre"])
    half = lambda a: np.concatenate((symfind.turn_row(np.eye(3)[a], c, math.pi).reshape(3, 4), [[0, 0, 0, 1]]))
    assert len(kept) == 2 and np.array_equal(kept[0], half(0)) and np.array_equal(kept[1], half(1))
    assert not any(np.abs(k - half(2)).max() < 1e-6 for k in kept)  # the dropped element is not in the file
    (R, t), = models_info_transforms(json.loads(json.dumps({"1": dict(diameter=dia, **proposal[1])})), None, 384)[1]
    assert len(R) == 3
