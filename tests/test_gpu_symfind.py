"""lc_amd.symfind on the GPU: every output of `deviation` EQUAL to the numpy oracle's (tests/symfind_oracle.py), scores and both witnesses,
no tolerance -- at the edges of the target tile and the query tile, with several unequal jobs in one call and the same jobs shuffled, with
repeated and descending query lists, on lattice meshes whose planted exact ties every merge level has to break, on an all-identical mesh,
on exact half turns given through `rodrigues`, on the device's refusals, under a captured graph whose table is overwritten in place, and
with a caller's workspace reused uncleared; and the two tools of `python -m lc_amd.prep_models` end to end on every shape of
tests/symfind_cases.py.  tests/test_symfind_host.py checks the conditions these cases rely on."""
import json
import os

import numpy as np
import pytest
import torch

from tests import symfind_cases as cases
from tests import symfind_oracle as oracle

pytestmark = pytest.mark.gpu
FACES0 = np.zeros((0, 3), np.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def _set(dev, meshes):
    from lc_amd.render import MeshSet

    return MeshSet([(np.asarray(v, np.float32), FACES0) for v in meshes], dev)


def _host(out):
    return {f: getattr(out, f).cpu().numpy() for f in cases.FIELDS}


def _run(dev, c, **kw):
    from lc_amd import symfind

    return symfind.deviation(_set(dev, c.meshes), *c.args(), **kw)


def _equal(got, want, what):
    for f in cases.FIELDS:
        assert cases.same_bits(got[f], getattr(want, f)), (what, f, got[f], getattr(want, f))


@pytest.mark.parametrize("name", cases.NAMES)
def test_named_calls_equal_the_oracle(dev, name):
    out = _run(dev, cases.named(name))
    want = cases.reference(name)
    _equal(_host(out), want, name)
    assert np.array_equal(out.dev.cpu().numpy(), want.dev, equal_nan=True)
    if name == "identity":
        assert (float(out.dev2[0, 0]), int(out.arg_query[0, 0]), int(out.arg_target[0, 0])) == (0.0, 0, 0)
    if name == "half-turns":
        assert out.dev2.cpu().numpy().tobytes() == np.zeros((1, 3), np.float32).tobytes()  # exactly +0.0


@pytest.mark.parametrize("name", sorted(cases.TIED))
def test_planted_ties_go_to_the_lowest_index_at_every_level(dev, name):
    _equal(_host(_run(dev, cases.tied(name).call)), cases.reference(name), name)


def test_shuffled_jobs_give_each_job_the_same_bits(dev):
    a, b = _host(_run(dev, cases.named("jobs"))), _host(_run(dev, cases.named("jobs-shuffled")))
    for place, g in enumerate(cases.JOB_SHUFFLE):
        for f in cases.FIELDS:
            assert cases.same_bits(a[f][g], b[f][place]), (g, f)


def test_refusals_on_the_device(dev):
    from lc_amd import symfind

    meshes = [cases.cloud(65, 1), cases.cloud(cases.T + 1, 2)]
    ms = _set(dev, meshes)
    table = cases.random_rows(6, 3)
    good = dict(mesh_index=[0, 1, 1, 0, 1, 0], row_off=[0, 2, 0, 0, 1, 3], row_k=[2, 3, 6, 1, 2, 3])
    queries = dict(query_idx=[0, 5, 64, 3, 3, 9, 2, 1], query_off=[0, 3, 3, 3, 5, 6], query_n=[3, 0, 2, 2, 1, 2])
    bad = dict(good, mesh_index=[0, 2, 1, -1, 1, 0], row_off=[0, 2, 1, 0, 1, -1])  # jobs 1, 3: no such mesh; job 2: rows 1..7 of 6; job 5: a negative offset
    badq = dict(queries, query_idx=[0, 65, 64, 3, 3, -1, 2, 1], query_n=[3, 0, 2, 2, 1, 3])  # job 0: index 65 of 65 vertices; job 4: only -1; job 5: 3 entries from 6 of 8
    for jobs, q in ((good, queries), (bad, queries), (good, badq), (bad, badq), (bad, None)):
        args = dict(jobs, **(q or {}))
        out = symfind.deviation(ms, table, **args)
        want = oracle.deviation(meshes, table, **args)
        _equal(_host(out), want, (jobs is bad, q is badq))
    out = _host(symfind.deviation(ms, table, **good, **badq))
    assert out["info"].tolist() == [1, 0, 0, 0, 1, -1]
    assert (out["dev2"][1] == -1).all() and (out["arg_query"][1] == -1).all()  # zero queries
    assert (out["dev2"][0, :2] >= 0).all() and (out["dev2"][5] == -1).all()  # the other queries still count; a refused job writes nothing
    assert _host(symfind.deviation(ms, table, **bad))["info"].tolist() == [0, -1, -1, -1, 0, -1]


def test_a_replayed_graph_follows_the_table_and_a_reused_workspace_changes_nothing(dev):
    from lc_amd import symfind

    c = cases.named("jobs")
    ms = _set(dev, c.meshes)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    table, other = as_dev(c.table), as_dev(cases.random_rows(len(c.table), 99))
    arrays = [as_dev(a) for a in c.args()[1:]]
    bounds = dict(max_k=int(c.row_k.max()), max_queries=int(c.query_n.max()))
    ws = torch.full((symfind.workspace_bytes(len(c.row_k), bounds["max_k"]) + 64,), 0xA5, device=dev, dtype=torch.uint8)
    eager = _host(symfind.deviation(ms, table, *arrays, **bounds))
    _equal(eager, cases.reference("jobs"), "device arrays")
    for _ in range(2):  # the workspace comes back dirty from the call before
        _equal(_host(symfind.deviation(ms, table, *arrays, workspace=ws, **bounds)), cases.reference("jobs"), "workspace")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = symfind.deviation(ms, table, *arrays, workspace=ws, **bounds)
    g.replay()
    torch.cuda.synchronize()
    _equal(_host(out), cases.reference("jobs"), "replay")
    table.copy_(other)  # in place: the graph reads the same address
    g.replay()
    torch.cuda.synchronize()
    replayed = _host(out)
    fresh = _host(symfind.deviation(ms, other, *arrays, **bounds))
    assert all(cases.same_bits(replayed[f], fresh[f]) for f in cases.FIELDS)
    _equal(replayed, oracle.deviation(c.meshes, other.cpu().numpy(), *c.args()[1:]), "replay after the overwrite")


def _write_models(tmp_path, names):
    from lc_amd import gen_z  # noqa: F401  (the reader of what is written here)

    for k, name in enumerate(names):
        v = cases.tool_mesh(name)
        with open(tmp_path / f"obj_{k + 1:06d}.ply", "w") as f:
            f.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n"
                    "property list uchar int vertex_indices\nend_header\n")
            f.writelines(f"{float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in v)


@pytest.mark.parametrize("name", list(cases.TOOL_SHAPES))
def test_the_tool_proposes_checks_and_rejects_end_to_end(dev, tmp_path, name):
    from lc_amd import prep_models
    from lc_amd.symmetry import SymmetrySet

    _, kind, eps, n_disc, n_cont, closed, truncated = cases.TOOL_SHAPES[name]
    _write_models(tmp_path, [name])
    common = [str(tmp_path), "--fps", "0", "--sym-eps-abs", str(eps), "--sym-eps-rel", "0", "--sym-queries", "0"]
    assert prep_models.main(common + ["--symmetries", "--sym-frame", kind]) == 0
    info = json.load(open(tmp_path / "models_info.json"))["1"]
    side = json.load(open(tmp_path / "symmetry_proposal.json"))["objects"]["1"]
    assert len(info.get("symmetries_discrete", ())) == n_disc and len(info.get("symmetries_continuous", ())) == n_cont
    assert (side["closed"], side["truncated"]) == (closed, truncated) and side["frame"]["kind"] == kind
    sym = SymmetrySet.from_models_info(str(tmp_path / "models_info.json"), device=dev)
    assert sym.max_k == (1 + n_disc) * (384 if n_cont else 1)
    assert prep_models.main(common + ["--check-symmetries"]) == 0
    report = json.load(open(tmp_path / "symmetry_check.json"))
    assert report["ok"] and all(e["ok"] for e in report["objects"]["1"]["symmetries_discrete"] + report["objects"]["1"]["symmetries_continuous"])
    if not (n_disc or n_cont):
        return
    spoilt = dict(json.load(open(tmp_path / "models_info.json")))
    spoilt["1"] = cases.spoil_turn(info) if n_disc else cases.spoil_axis(info)
    with open(tmp_path / "spoilt.json", "w") as f:
        json.dump(spoilt, f)
    assert prep_models.main(common + ["--check-symmetries", str(tmp_path / "spoilt.json")]) != 0
    report = json.load(open(tmp_path / "symmetry_check.json"))
    from lc_amd import symfind

    assert symfind.failed_entries(report) == ["obj 1 symmetries_discrete[0]" if n_disc else "obj 1 symmetries_continuous[0]"]
    assert os.path.exists(tmp_path / "symmetry_proposal.json")


def test_the_farthest_points_are_the_queries_of_meshes_of_unequal_size(dev, tmp_path):
    """`--sym-queries N` with N between the sizes of two meshes: the smaller is queried at every vertex (its farthest points are all of
    them), the larger at its first N farthest points; the sidecar and the check report say so, the decisions are those of every vertex."""
    from lc_amd import models, prep_models
    from lc_amd.render import MeshSet

    names = ("cuboid", "scalene")
    sizes = [len(cases.tool_mesh(n)) for n in names]
    N = (sizes[0] + sizes[1]) // 2
    assert sizes[0] < N < sizes[1]
    _write_models(tmp_path, names)
    common = [str(tmp_path), "--fps", "0", "--sym-eps-abs", "0.5", "--sym-eps-rel", "0", "--sym-queries", str(N)]
    assert prep_models.main(common + ["--symmetries", "--sym-frame", "model"]) == 0
    info = json.load(open(tmp_path / "models_info.json"))
    side = json.load(open(tmp_path / "symmetry_proposal.json"))["objects"]
    assert [side[k]["n_queries"] for k in ("1", "2")] == [sizes[0], N]
    assert len(info["1"]["symmetries_discrete"]) == 3 and "symmetries_discrete" not in info["2"] and "symmetries_continuous" not in info["2"]
    ms = MeshSet([(cases.tool_mesh(n), FACES0) for n in names], dev)
    got = prep_models._queries(ms, ms_meshes(names), N)
    for k, n in enumerate(names):  # each mesh's own selection, cut to its count
        want = models.prepare(_set(dev, [cases.tool_mesh(n)]), min(N, sizes[k]), want_diameter=False).fps_index.cpu().numpy()[0]
        assert np.array_equal(got[k], want), n
    assert sorted(got[0].tolist()) == list(range(sizes[0]))
    assert prep_models.main(common + ["--check-symmetries"]) == 0
    report = json.load(open(tmp_path / "symmetry_check.json"))["objects"]
    assert [report[k]["n_queries"] for k in ("1", "2")] == [sizes[0], N] and report["1"]["ok"]


def ms_meshes(names):
    return [(cases.tool_mesh(n), FACES0) for n in names]
