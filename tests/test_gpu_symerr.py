"""GPU tests of the symmetry-aware pose errors (lc_amd.metrics.compute_sym_pose_errors, lc_sym_metrics.hip): mssd, mspd and proj against the
fp64 oracle (tests/symerr_oracle.py) on the same fp32 inputs within the project's metric tolerance (tests/symerr_cases.tol =
metrics_cases.tol, 2e-5 max(1, |ref|)), the winning symmetries exactly, and the same bits in every launch shape.  The inputs and the
conditions that make them able to see a skipped vertex or symmetry are tests/symerr_cases.py (shown on the CPU by
tests/test_symerr_oracle.py).  Every figure is printed as a fraction of the tolerance before it is asserted."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import symerr_cases as C
from tests import symerr_oracle as orc
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("mssd", "mspd", "proj")


def _symset(case):
    from lc_amd import symmetry

    return symmetry.SymmetrySet(case["transforms"], list(range(len(case["transforms"]))), DEV)


def _shifted(t):
    """A copy of `t` one element further into its own allocation: 4-byte aligned floats and ints, 8-byte aligned doubles, nothing more."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def _shifted_symset(ss):
    out = copy.copy(ss)
    out.table, out.obj_off, out.obj_k = _shifted(ss.table), _shifted(ss.obj_off), _shifted(ss.obj_k)
    assert out.table.data_ptr() % 8 == 0 and out.table.data_ptr() % 16 != ss.table.data_ptr() % 16
    return out


def _tensors(case, shift=False):
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in ("R_est", "t_est", "R_gt", "t_gt", "cam_K", "pts", "pts_off", "pts_cnt", "obj_index")}
    return {k: _shifted(v) for k, v in t.items()} if shift else t


def _call(t, ss, rows=slice(None)):
    from lc_amd import metrics

    out = metrics.compute_sym_pose_errors(t["R_est"][rows], t["t_est"][rows], t["R_gt"][rows], t["t_gt"][rows], t["cam_K"][rows], t["pts"], ss,
                                          t["obj_index"][rows], pts_off=t["pts_off"][rows], pts_cnt=t["pts_cnt"][rows])
    return out


def _np(out):
    err = torch.stack((out["mssd"], out["mspd"], out["proj"]), -1).cpu().numpy()
    arg = torch.stack((out["mssd_sym"], out["mspd_sym"]), -1).cpu().numpy()
    assert err.dtype == np.float32 and arg.dtype == np.int32
    return err, arg


def _run(case, ss=None, shift=False):
    return _np(_call(_tensors(case, shift), _symset(case) if ss is None else ss))


def _same_bits(a, b, what):
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), (what, "err", np.nonzero((a[0].view(np.int32) != b[0].view(np.int32)).any(-1))[0])
    assert np.array_equal(a[1], b[1]), (what, "arg")


def _check(what, got, ref, arg_exact=True):
    """Errors within the tolerance of the fp64 oracle (each figure printed as a fraction of it first), the winning symmetries exactly."""
    (err, arg), (rerr, rarg) = got, ref
    assert err.shape == rerr.shape and arg.shape == rarg.shape
    frac = np.abs(err.astype(np.float64) - rerr) / np.vectorize(C.tol)(rerr)
    for j, name in enumerate(NAMES):
        print(f"{what}: {name} worst {frac[:, j].max():.4f} of the tolerance (pose {int(frac[:, j].argmax())}, ref {rerr[int(frac[:, j].argmax()), j]:.6g})")
    assert np.isfinite(err).all() and (frac <= 1.0).all(), (what, frac.max())
    if arg_exact:
        assert np.array_equal(arg, rarg), (what, np.nonzero((arg != rarg).any(-1))[0])


@functools.lru_cache(maxsize=None)
def _vertex():
    case = C.vertex_edge_case()
    return case, orc.batch(case)


@functools.lru_cache(maxsize=None)
def _symmetry():
    case = C.symmetry_edge_case()
    return case, orc.batch(case)


def test_reference_golden():
    z = np.load(f"{GOLDEN}/sym_err_b12_m700.npz")
    case = C.golden_case(z)
    ref = (np.stack((z["mssd"], z["mspd"], z["proj"]), -1), np.stack((z["mssd_sym"], z["mspd_sym"]), -1))
    _check("golden", _run(case), ref)
    # the route with one cloud for every pose (no offsets) and a single (3,3) camera: the same bits
    from lc_amd import metrics

    t = _tensors(case)
    out = metrics.compute_sym_pose_errors(t["R_est"], t["t_est"][..., None], t["R_gt"], t["t_gt"], t["cam_K"][0], t["pts"], _symset(case), t["obj_index"].long())
    _same_bits(_np(out), _run(case), "no offsets")


def test_every_vertex_counts():
    case, ref = _vertex()
    rows = C.vertex_conditions(case)  # on the CPU, before any GPU result is read
    assert all(r["mssd"] >= C.SENSITIVITY and r["mspd"] >= C.SENSITIVITY for r in rows)
    assert len({int(o) % 2 for o in case["pts_off"]}) == 2
    _check("vertex edges", _run(case), ref)


def test_every_symmetry_counts():
    case, ref = _symmetry()
    rows = C.symmetry_conditions(case)
    assert all(r["mssd"] >= C.SENSITIVITY and r["mspd"] >= C.SENSITIVITY and r["k3"] == r["win"] and r["k2"] == r["win"] for r in rows)
    got = _run(case)
    _check("symmetry edges", got, ref)
    assert np.array_equal(got[1][:, 0], case["win"]) and np.array_equal(got[1][:, 1], case["win"])


def test_ties_go_to_the_lowest_symmetry():
    case = C.tie_case()
    got = _run(case)
    _check("identical rows", got, orc.batch(case))
    assert (got[1] == 2).all()  # rows 2 and 4 are the same bits: equal errors by construction
    case = C.tie_case(last_bit=True)
    err, arg = _run(case)
    _check("rows one bit apart", (err, arg), orc.batch(case), arg_exact=False)
    for b in range(len(arg)):
        e3, e2 = orc.per_symmetry(*C.pose_args(case, b))
        want = (C.lowest_fp32_winner(e3, err[b, 0]), C.lowest_fp32_winner(e2, err[b, 1]))
        print(f"one bit apart, pose {b}: arg {arg[b].tolist()}, oracle on the returned bits {want}, e[2] - e[4] = {e3[2] - e3[4]:.2e}, {e2[2] - e2[4]:.2e}")
        assert tuple(arg[b]) == want and set(arg[b]) <= {2, 4}


def test_same_bits_in_every_shape():
    (va, _), (sa, _) = _vertex(), _symmetry()
    both = C.merge(va, sa)
    ss = _symset(both)
    first = _run(both, ss)
    _same_bits(_run(both, ss), first, "second launch")
    nv = len(va["obj_index"])
    # each case alone: another B, another table, another vertex buffer
    _same_bits(_run(va), (first[0][:nv], first[1][:nv]), "vertex case alone")
    _same_bits(_run(sa), (first[0][nv:], first[1][nv:]), "symmetry case alone")
    # pose by pose, B = 1, on copies at another alignment
    t, ss1 = _tensors(both, shift=True), _shifted_symset(ss)
    assert t["pts"].data_ptr() % 8 != _tensors(both)["pts"].data_ptr() % 8
    single = [_call(t, ss1, slice(b, b + 1)) for b in range(len(both["obj_index"]))]
    single = (np.concatenate([_np(o)[0] for o in single]), np.concatenate([_np(o)[1] for o in single]))
    _same_bits(single, first, "B = 1")
    # reversed, with the two cases' objects interleaved
    a, b = list(range(nv))[::-1], list(range(nv, len(both["obj_index"])))[::-1]
    perm = [x for pair in zip(a, b) for x in pair] + a[len(b):] + b[len(a):]
    assert sorted(perm) == list(range(len(both["obj_index"])))
    got = _run(C.take(both, perm), ss)
    _same_bits(got, (first[0][perm], first[1][perm]), "reversed and interleaved")


def test_exact_zeros():
    case = C.zero_case()
    err, arg = _run(case)
    assert len(arg) == 270 and set(case["pts_cnt"].tolist()) == {1, 255, 1025}
    assert not err.view(np.int32).any(), np.nonzero(err)[0]  # +0.0, all three
    assert not arg.any()


def test_cameras():
    case, plain = C.camera_case()
    assert (case["cam_K"][:, 0, 0] != case["cam_K"][:, 1, 1]).all() and (case["cam_K"][:, 0, 1] != 0).all() and (case["cam_K"][2::3, 2, :2] != 0).all()
    got = _run(case)
    _check("cameras", got, orc.batch(case))
    other = _run(plain)
    assert np.array_equal(got[0][:, 0].view(np.int32), other[0][:, 0].view(np.int32)) and np.array_equal(got[1][:, 0], other[1][:, 0])
    assert (got[0][:, 1] != other[0][:, 1]).all()


def test_refusals_on_the_device():
    """Rows 1, 4 and 6 are refused: obj_index -1, obj_index = n_obj and pts_cnt 0.  Their other arguments stay those of valid poses, and
    the table the launch is told about (n_obj = 4) is the front of a table of five objects, so a kernel that read a refused row anyway
    would still read inside this test's own buffers.  The test pins the outputs and provokes nothing."""
    case, _ = C.golden_inputs()
    five = _symset(dict(transforms=case["transforms"] + [case["transforms"][1]]))
    ss = copy.copy(five)
    ss.n_obj = 4
    assert five.n_obj == 5 and ss.obj_k.numel() == 5 and ss.max_k == 36
    bad = {1: ("obj_index", -1), 4: ("obj_index", 4), 6: ("pts_cnt", 0)}
    mixed = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    for b, (key, val) in bad.items():
        mixed[key][b] = val
    err, arg = _run(mixed, ss)
    keep = [b for b in range(12) if b not in bad]
    for b in bad:
        assert np.isnan(err[b]).all() and (arg[b] == -1).all(), b
    _same_bits((err[keep], arg[keep]), _run(C.take(case, keep)), "valid rows")
    _check("valid rows", (err[keep], arg[keep]), tuple(a[keep] for a in orc.batch(case)))
    from lc_amd import metrics

    t = _tensors(case)
    out = metrics.compute_sym_pose_errors(t["R_est"][:0], t["t_est"][:0], t["R_gt"][:0], t["t_gt"][:0], t["cam_K"][:0], t["pts"], _symset(case), t["obj_index"][:0])
    assert out["mssd"].shape == (0,) and out["mssd_sym"].shape == (0,)


def test_graph_capture():
    case, _ = C.golden_inputs()
    ss, t = _symset(case), _tensors(case)
    _call(t, ss)  # sizes the cached workspace outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(t, ss)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _call(t, ss)
    perm = [5, 0, 11, 3, 8, 1, 9, 2, 10, 4, 7, 6]  # new pose values (and objects) written into the same tensors
    new = _tensors(C.take(case, perm))
    for k in ("R_est", "t_est", "R_gt", "t_gt", "obj_index"):
        t[k].copy_(new[k])
    g.replay()
    torch.cuda.synchronize()
    replayed = _np(out)
    eager = _run(C.take(case, perm), ss)
    _same_bits(replayed, eager, "replay")
    _check("replay", replayed, tuple(a[perm] for a in orc.batch(case)))


def test_meshes_and_states_routes():
    from lc_amd import metrics, render
    from lc_amd.transforms import quaternion_rep_to_RT

    rng = np.random.default_rng(77)
    _, transforms = C.bop_objects(36)
    counts = (130, 64, 257, 33)
    clouds = [((rng.random((m, 3)) * 2 - 1) * C.BOX).astype(np.float32) for m in counts]
    meshes = render.MeshSet([(v, np.zeros((1, 3), np.int32)) for v in clouds], DEV)
    B = 9
    obj = np.array([0, 1, 2, 3, 3, 2, 1, 0, 2], np.int32)
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    tg = np.stack((rng.uniform(-60, 60, B), rng.uniform(-60, 60, B), rng.uniform(700, 900, B)), -1)
    sg = torch.from_numpy(np.concatenate((q, tg), 1).astype(np.float32)).to(DEV)
    se = sg + torch.from_numpy(np.concatenate((rng.normal(size=(B, 4)) * 0.01, rng.normal(size=(B, 3))), 1).astype(np.float32)).to(DEV)
    K = torch.from_numpy(C.lm_camera(1)[0].astype(np.float32)).to(DEV)
    case = dict(transforms=transforms)
    ss = _symset(case)
    idx = torch.from_numpy(obj).to(DEV)
    mesh_idx = idx.clone()
    mesh_idx[4] = -1  # a mesh the set lacks: refused
    (Re, te), (Rg, tg_) = quaternion_rep_to_RT(se), quaternion_rep_to_RT(sg)
    off = torch.from_numpy(meshes.table_host[obj, 0].copy()).to(DEV)
    cnt = torch.from_numpy(meshes.table_host[obj, 1].copy()).to(DEV)
    cnt[4] = 0
    explicit = _np(metrics.compute_sym_pose_errors(Re, te, Rg, tg_, K, meshes.verts, ss, idx, pts_off=off, pts_cnt=cnt))
    routed = _np(metrics.sym_pose_errors_from_states(se, sg, K, syms=ss, obj_index=idx, meshes=meshes, mesh_index=mesh_idx))
    _same_bits(routed, explicit, "meshes + states")
    assert np.isnan(routed[0][4]).all() and (routed[1][4] == -1).all() and np.isfinite(np.delete(routed[0], 4, 0)).all()
    ref_case = C._case(Re.cpu().numpy(), te.cpu().numpy().reshape(B, 3), Rg.cpu().numpy(), tg_.cpu().numpy().reshape(B, 3), np.tile(K.cpu().numpy(), (B, 1, 1)),
                       meshes.verts.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy(), obj, transforms)
    keep = [b for b in range(B) if b != 4]
    _check("meshes + states", (routed[0][keep], routed[1][keep]), orc.batch(C.take(ref_case, keep)))
    # default mesh index: the object index itself
    same = _np(metrics.compute_sym_pose_errors(Re, te, Rg, tg_, K, syms=ss, obj_index=idx, meshes=meshes))
    _same_bits((np.delete(same[0], 4, 0), np.delete(same[1], 4, 0)), (np.delete(explicit[0], 4, 0), np.delete(explicit[1], 4, 0)), "default mesh index")
    # a SymmetrySet on another device than the poses
    far = copy.copy(ss)
    far.device = torch.device("cuda", 1)
    with pytest.raises(RuntimeError, match="SymmetrySet is on cuda:1"):
        metrics.compute_sym_pose_errors(Re, te, Rg, tg_, K, meshes.verts, far, idx)
