"""The symmetry deviation of a model on the device (lc_amd/csrc/symfind/lc_symfind.hip, lc_amd/_C/liblc_amd_symfind.so; C ABI and the exact
definitions in include/lc_amd_symfind.h, `lc_symfind_deviation_f32`), and the two uses `python -m lc_amd.prep_models` makes of it.

    deviation(meshes: MeshSet, table, mesh_index, row_off, row_k, query_idx=None, query_off=None, query_n=None, *, max_k=None, max_queries=None,
              workspace=None) -> Deviation(dev2, arg_query, arg_target, dev, info)
    workspace_bytes(n_jobs, max_k)
    device_scorer(meshes) -> score(jobs)        the device call behind check_symmetries / propose_symmetries
    check_symmetries(score, ids, models_info, diameters, ...)  -> the dict of symmetry_check.json
    propose_symmetries(score, ids, frames, diameters, ...)     -> ({id: the two models_info keys}, the dict of symmetry_proposal.json)

BOP's rule (the BOP 2020 challenge paper, section 2.3): a transform S is a potential symmetry of a model when the Hausdorff deviation
between its vertices and its transformed vertices is below eps = max(15 mm, 0.1 diameter).  `deviation` evaluates the directed deviation
max_i min_j |S x_i - v_j| for every row of a transform table in the layout of `lc_amd.symmetry.SymmetrySet` (row-major 3 x 4 [R | t],
float64) against the vertices of the job's mesh: the query is transformed in fp64 and rounded once to fp32, d2 is fp32 without FMA, the
min goes to the lowest target and the max to the lowest query position at ties, a NaN d2 never wins a min.  Outputs are (n_jobs, max_k),
-1 where a job has no such row, no vertex or no query; `dev = sqrt(dev2)` in float64; `info` -1 for a job refused on the device, 1 if a
query index was out of range and skipped.  With a query list the result is a LOWER bound of the deviation over all vertices.  Runs on the
current stream, never waits for the device, reads nothing back, can be captured into a graph (with the job arrays on the device already).
There is no CPU fallback (tests/symfind_oracle.py is the numpy restatement).

`check_symmetries` and `propose_symmetries` are host logic around a `score(jobs)` callable -- jobs = [(mesh position, transforms (K,12)
float64, query indices or None)], answer = [dev (K,) float64] -- so that they run against the numpy oracle without a device.  The proposal is a
STATED SEARCH in the manner of lc_amd.obox: rotations about the three axes of one frame through its centre, judged by the rule above.  It
is no proof of a symmetry, sees no texture or colour, knows no axis outside its frame (a cube's diagonal three-fold axes appear only
through the closure), and does not reproduce BOP's hand-made annotations.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_int, c_size_t, c_void_p
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import build as _build
from . import symmetry as _symmetry
from .render import MeshSet  # (importing it does not load the render library)

TILE = 256     # LC_SYMFIND_TILE: target vertices of one LDS tile
QUERIES = 256  # LC_SYMFIND_QUERIES: queries of one workgroup
STEPS = 384    # the reference's discretisation of a continuous symmetry (SymmetrySet's default)
MAX_DISCRETE = 47  # the closure stops here (the 48 elements of the cube's full group without the identity)
SAME = 1e-9    # two transforms are equal when their 3 x 4 differ by less

_SO = _lib.SideLibrary(_build.SYMFIND, {
    "lc_symfind_workspace_bytes": (c_size_t, [c_int, c_int]),
    # the mesh table is passed twice: on the device, and as a HOST int array the argument rules are checked from
    "lc_symfind_deviation_f32": (c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(c_int), c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
})
_SIGNATURES, load = _SO.signatures, _SO.load


class Deviation(NamedTuple):
    dev2: Tensor        # (n_jobs,max_k) float32: the score, -1 where there is none
    arg_query: Tensor   # (n_jobs,max_k) int32: the vertex index of the witness query
    arg_target: Tensor  # (n_jobs,max_k) int32: the witness target of that query
    dev: Tensor         # (n_jobs,max_k) float64: sqrt(dev2) (NaN where dev2 is -1)
    info: Tensor        # (n_jobs,) int32: 0, -1 refused on the device, 1 a query index out of range


def workspace_bytes(n_jobs: int, max_k: int) -> int:
    """The formula of include/lc_amd_symfind.h, restated: the library's own answer is `lc_symfind_workspace_bytes`."""
    if n_jobs <= 0 or max_k <= 0:
        return 0
    return -(-8 * n_jobs * max_k // 16) * 16


def _ints(name, a, dev):
    """(device int32 tensor, host maximum or None) of a job array given on the host (uploaded) or on the device (taken as it is)."""
    if isinstance(a, Tensor):
        if not a.is_cuda or a.dtype != torch.int32 or a.dim() != 1:
            raise TypeError(f"lc_amd.symfind: {name} as a tensor must be a 1-d int32 tensor on the device, got {a.dtype} {tuple(a.shape)} on {a.device}")
        return a.contiguous(), None
    h = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
    return torch.from_numpy(h).to(dev), (int(h.max()) if h.size else 0)


@torch.no_grad()
def deviation(meshes: MeshSet, table, mesh_index, row_off, row_k, query_idx=None, query_off=None, query_n=None, *, max_k=None, max_queries=None,
              workspace=None) -> Deviation:
    """`table`: (Ktot,12) float64, a device tensor or a host array.  The job arrays (and the query arrays, all three or none) are host
    sequences -- uploaded, their maxima taken here -- or int32 device tensors, for which `max_k` (and `max_queries` with a query list) must
    be given: the bounds the grid is sized from; a job beyond them is refused on the device (info -1)."""
    if not isinstance(meshes, MeshSet):
        raise TypeError(f"lc_amd.symfind: meshes must be a MeshSet, got {type(meshes)}")
    dev = meshes.device
    if not isinstance(table, Tensor):
        table = torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.float64))).to(dev)
    if not table.is_cuda or table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 12 or table.shape[0] < 1:
        raise TypeError(f"lc_amd.symfind: table must be (Ktot,12) float64 on the device, got {table.dtype} {tuple(table.shape)} on {table.device}")
    table = table.contiguous()
    (mesh_index, _), (row_off, _), (row_k, host_k) = _ints("mesh_index", mesh_index, dev), _ints("row_off", row_off, dev), _ints("row_k", row_k, dev)
    G = mesh_index.numel()
    if G < 1 or row_off.numel() != G or row_k.numel() != G:
        raise ValueError(f"lc_amd.symfind: mesh_index, row_off and row_k must have one entry per job, got {G}, {row_off.numel()}, {row_k.numel()}")
    max_k = host_k if max_k is None else int(max_k)
    if max_k is None:
        raise ValueError("lc_amd.symfind: row_k on the device needs max_k")
    max_k = max(min(max_k, int(table.shape[0])), 1)  # (a job with more rows than the table has is refused on the device)
    total_q = 0
    if query_idx is not None:
        if query_off is None or query_n is None:
            raise ValueError("lc_amd.symfind: a query list needs query_idx, query_off and query_n")
        (query_idx, _), (query_off, _), (query_n, host_q) = _ints("query_idx", query_idx, dev), _ints("query_off", query_off, dev), _ints("query_n", query_n, dev)
        total_q = query_idx.numel()
        if total_q < 1:
            raise ValueError("lc_amd.symfind: query_idx is empty (a job without queries has query_n 0 in a list that others fill)")
        if query_off.numel() != G or query_n.numel() != G:
            raise ValueError("lc_amd.symfind: query_off and query_n must have one entry per job")
        max_queries = host_q if max_queries is None else int(max_queries)
        if max_queries is None:
            raise ValueError("lc_amd.symfind: query_n on the device needs max_queries")
        max_queries = max(min(max_queries, total_q), 1)
    elif query_off is not None or query_n is not None:
        raise ValueError("lc_amd.symfind: query_off / query_n without query_idx")
    lib = load()
    dev2 = torch.empty(G, max_k, device=dev, dtype=torch.float32)
    arg_query = torch.empty(G, max_k, device=dev, dtype=torch.int32)
    arg_target = torch.empty(G, max_k, device=dev, dtype=torch.int32)
    info = torch.empty(G, device=dev, dtype=torch.int32)
    nbytes = int(lib.lc_symfind_workspace_bytes(G, max_k))
    if workspace is None:
        workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    elif not isinstance(workspace, Tensor) or not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < nbytes or not workspace.is_contiguous():
        raise ValueError(f"lc_amd.symfind: workspace must be a contiguous uint8 device tensor of at least {nbytes} bytes")
    table_host = np.ascontiguousarray(meshes.table_host, dtype=np.int32)
    max_verts = max(int(table_host[:, 1].max()), 1)
    with _lib.on_device(dev):
        rc = lib.lc_symfind_deviation_f32(_lib.ptr(meshes.verts), meshes.total_verts, _lib.ptr(meshes.table), table_host.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                          meshes.n_meshes, max_verts, _lib.ptr(table), int(table.shape[0]), _lib.ptr(mesh_index), _lib.ptr(row_off),
                                          _lib.ptr(row_k), G, max_k, _lib.ptr(query_idx), _lib.ptr(query_off), _lib.ptr(query_n), total_q,
                                          max_queries or 0, _lib.ptr(dev2), _lib.ptr(arg_query), _lib.ptr(arg_target), _lib.ptr(info), _lib.ptr(workspace),
                                          workspace.numel(), _lib.stream_ptr(dev))
    if rc != 0:
        _SO.fail("symfind.deviation", rc)
    return Deviation(dev2, arg_query, arg_target, torch.sqrt(dev2.double()), info)


# ---- the two tools' host logic: everything below is numpy around a `score(jobs)` callable ----

def device_scorer(meshes: MeshSet):
    """score(jobs) on the device: jobs = [(mesh position, transforms (K,12) float64, query vertex indices or None)] -> [dev (K,) float64], all
    jobs in ONE call of `deviation`, read back once (an offline tool's read).  Jobs with and without a query list do not mix in a call: a
    job without one is given the list of all its vertices."""
    def score(jobs):
        jobs = [(int(m), np.asarray(t, np.float64).reshape(-1, 12), q) for m, t, q in jobs]
        if not jobs:
            return []
        ks = [len(t) for _, t, _ in jobs]
        offs = np.concatenate(([0], np.cumsum(ks)[:-1]))
        q = {}
        if any(j[2] is not None for j in jobs):
            lists = [np.arange(int(meshes.table_host[m, 1]), dtype=np.int32) if ql is None else np.asarray(ql, np.int32).reshape(-1) for m, _, ql in jobs]
            q = dict(query_idx=np.concatenate(lists), query_off=np.concatenate(([0], np.cumsum([len(l) for l in lists])[:-1])), query_n=[len(l) for l in lists])
        out = deviation(meshes, np.concatenate([t for _, t, _ in jobs]), [m for m, _, _ in jobs], offs, ks, **q)
        dev, info = out.dev.cpu().numpy(), out.info.cpu().numpy()
        if info.any():
            raise RuntimeError(f"lc_amd.symfind: the device refused jobs {np.flatnonzero(info).tolist()} (info {info[info != 0].tolist()})")
        return [dev[g, :k].copy() for g, k in enumerate(ks)]

    return score


def epsilon(diameter, eps_abs=15.0, eps_rel=0.1):
    """BOP's bound: max(eps_abs, eps_rel * diameter), in the unit of the vertices."""
    return max(float(eps_abs), float(eps_rel) * float(diameter))


def inverse_rows(rows):
    """S^-1 = [R^T | -R^T t] of every row-major 3 x 4 row, in float64."""
    m = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    Rt = m[:, :, :3].transpose(0, 2, 1)
    return np.concatenate((Rt, -(Rt @ m[:, :, 3:])), -1).reshape(-1, 12)


def compose(a, b):
    """a after b of two row-major 3 x 4 transforms, float64: [Ra Rb | Ra tb + ta]."""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    return np.concatenate((a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]), 1).reshape(12)


_IDENTITY = np.eye(3, 4).reshape(12)


def same(a, b):
    return bool(np.abs(np.asarray(a) - np.asarray(b)).max() < SAME)


def _both_ways(score, jobs):
    """max(dev of S, dev of S^-1) per row: S^-1 formed on the host in fp64, its rows appended to the job's."""
    got = score([(m, np.concatenate((t, inverse_rows(t))), q) for m, t, q in jobs])
    return [np.maximum(d[:len(t)], d[len(t):]) for d, (_, t, _) in zip(got, jobs)]


def check_symmetries(score, ids, models_info, diameters, *, queries=None, eps_abs=15.0, eps_rel=0.1, steps=STEPS):
    """The dict of symmetry_check.json: per object the diameter, eps and, per entry of `symmetries_discrete` / `symmetries_continuous` of
    `models_info` (a dict or a path), the larger of the deviations of S and S^-1 (`dev`, in the unit of the vertices: mm for BOP;
    `dev_rel` = dev / diameter) and `ok` = dev <= eps; for the continuous entry the maximum over its `steps` - 1 turns and the `step` it
    occurs at.  The rows are those of `SymmetrySet.from_models_info` (symmetry.models_info_transforms: row d * C of an object is discrete
    entry d, rows 1..C-1 the continuous entry); the products of a discrete with a continuous entry (d >= 1 and c >= 1) are not judged.
    `queries`: per object the query vertex indices, or None for every vertex (then dev is the Hausdorff deviation over the vertices;
    with a list, a lower bound of it).  `ok` at the top is the conjunction."""
    ids = [int(i) for i in ids]
    models_info = _load(models_info)
    _, transforms = _symmetry.models_info_transforms(models_info, ids, steps)
    jobs = [(k, np.concatenate((R, t[..., None]), -1).reshape(-1, 12), None if queries is None else queries[k]) for k, (R, t) in enumerate(transforms)]
    devs = _both_ways(score, jobs)
    by_id = {int(k): v for k, v in models_info.items()}
    report, all_ok = {}, True
    for k, oid in enumerate(ids):
        entry = by_id[oid]
        n_disc = len(entry.get("symmetries_discrete", ()) or ())
        has_cont = bool(entry.get("symmetries_continuous", ()) or ())
        C = int(steps) if has_cont else 1
        dia = float(diameters[k])
        eps = epsilon(dia, eps_abs, eps_rel)
        dev = devs[k]
        assert len(dev) == (1 + n_disc) * C
        one = lambda d: {"dev": float(d), "dev_rel": float(d) / dia if dia > 0 else None, "ok": bool(d <= eps)}
        disc = [dict(index=d - 1, **one(dev[d * C])) for d in range(1, n_disc + 1)]
        cont = []
        if has_cont and C > 1:
            c = 1 + int(np.argmax(dev[1:C]))  # the first of equal maxima
            cont = [dict(index=0, step=c, steps=C, **one(dev[c]))]
        ok = all(e["ok"] for e in disc + cont)
        all_ok &= ok
        report[str(oid)] = {"diameter": dia, "eps": eps, "n_queries": None if queries is None else int(len(queries[k])),
                            "symmetries_discrete": disc, "symmetries_continuous": cont, "ok": ok}
    return {"eps_abs": float(eps_abs), "eps_rel": float(eps_rel), "continuous_steps": int(steps), "ok": bool(all_ok), "objects": report}


def _load(info):
    import json
    import os

    if isinstance(info, (str, os.PathLike)):
        with open(info) as f:
            return json.load(f)
    return info


def failed_entries(report):
    """["obj <id> symmetries_discrete[<n>]", ...] of a check_symmetries report: the entries that are not ok."""
    return [f"obj {oid} {kind}[{e['index']}]" for oid, o in report["objects"].items() for kind in ("symmetries_discrete", "symmetries_continuous")
            for e in o[kind] if not e["ok"]]


def frame_of_xform(xform):
    """(centre (3,), axes (3,3) rows) of an `lc_amd.obox` transform [R | t]: p' = R v + t, so the box axes are the rows of R and its centre,
    in model coordinates, -R^T t.  R is fp32 there, orthonormal to 1e-7 only; the axes returned are its nearest rotation in float64 (the
    polar factor, by an SVD), so that turns about them compose to the group they generate within the 1e-9 of `same`."""
    X = np.asarray(xform, np.float64).reshape(4, 4)
    U, _, Vt = np.linalg.svd(X[:3, :3])
    R = U @ Vt
    return -(R.T @ X[:3, 3]), R


def axis_turns(max_fold=12, steps=STEPS):
    """The turns tried about every axis as (label, angle): (i) ("s", s) for the `steps` - 1 turns 2 pi s / steps, then (ii) ("f", n, k) for
    2 pi k / n, n = 2..max_fold, k = 1..n-1, where k / n is no multiple of 1 / steps (those are in (i) at s = steps k / n)."""
    turns = [(("s", s), 2.0 * math.pi * s / steps) for s in range(1, steps)]
    for n in range(2, int(max_fold) + 1):
        turns += [(("f", n, k), 2.0 * math.pi * k / n) for k in range(1, n) if (steps * k) % n]
    return turns


def turn_row(axis, centre, angle):
    """Row-major 3 x 4 of the rotation by `angle` about the unit `axis` through `centre`: R = rodrigues, t = c - R c, float64."""
    R = _symmetry.rodrigues(axis, angle)
    return np.concatenate((R, (centre - R @ centre)[:, None]), 1).reshape(12)


def _fold_positions(turns, n, steps):
    """Where the n - 1 turns 2 pi k / n stand in `turns`."""
    at = {label: i for i, (label, _) in enumerate(turns)}
    return [at[("f", n, k)] if (steps * k) % n else at[("s", steps * k // n)] for k in range(1, n)]


def close_group(generators, cap=MAX_DISCRETE):
    """(elements, truncated): the closure under composition of the row-major 3 x 4 `generators` (float64), the identity left out, equal
    elements (`same`) kept once, in the order they are met -- generators first, then a o b for a, b in list order, until nothing new
    appears.  Stops at `cap` elements and says so."""
    elems = []
    for g in generators:
        if not same(g, _IDENTITY) and not any(same(g, e) for e in elems):
            elems.append(np.asarray(g, np.float64).reshape(12))
    done = 0
    while done < len(elems):
        n = len(elems)
        for i in range(n):
            for j in range(n):
                if i < done and j < done:
                    continue
                c = compose(elems[i], elems[j])
                if same(c, _IDENTITY) or any(same(c, e) for e in elems):
                    continue
                if len(elems) >= cap:
                    return elems, True
                elems.append(c)
        done = n
    return elems, False


def propose_symmetries(score, ids, frames, diameters, *, queries=None, eps_abs=15.0, eps_rel=0.1, max_fold=12, steps=STEPS, frame_kind="obox"):
    """A stated search, not a proof: ({id: {"symmetries_discrete": [...], "symmetries_continuous": [...]}} with empty keys left out, the dict
    of symmetry_proposal.json).  `frames[k]` = (centre c (3,), axes (3,3) rows) of object k.  Candidates are the rotations `axis_turns`
    about each axis through c, all objects in one `score` call (one direction: a rotation group holds the inverse of every member).  With
    dev the score and eps = max(eps_abs, eps_rel diameter):
      * an axis is continuous when its steps - 1 turns of (i) all have dev <= eps; of several the one with the smallest maximum, lowest
        index at ties (the reference supports one);
      * any other axis has an n-fold symmetry for the largest n <= max_fold whose n - 1 turns all have dev <= eps;
      * with a continuous axis the discrete set is the accepted half turns about the other two axes, as they are (their product is a
        turn about the continuous axis, which the continuous entry holds already);
      * otherwise it is `close_group` of the accepted turns; elements that were no candidates are scored in a second call, one above eps
        is dropped and the object reported `closed: false`; `truncated` says the closure met its cap."""
    ids = [int(i) for i in ids]
    turns = axis_turns(max_fold, steps)
    T = len(turns)
    cand, jobs = [], []
    for k in range(len(ids)):
        c, axes = np.asarray(frames[k][0], np.float64), np.asarray(frames[k][1], np.float64)
        rows = np.stack([turn_row(axes[a] / np.linalg.norm(axes[a]), c, ang) for a in range(3) for _, ang in turns])
        cand.append(rows)
        jobs.append((k, rows, None if queries is None else queries[k]))
    devs = score(jobs)
    proposal, sidecar, work = {}, {}, []  # work[k] = (the object's elements, their scores or None, the places of the unscored)
    for k, oid in enumerate(ids):
        c, axes = np.asarray(frames[k][0], np.float64), np.asarray(frames[k][1], np.float64)
        dia = float(diameters[k])
        eps = epsilon(dia, eps_abs, eps_rel)
        dev = np.asarray(devs[k], np.float64).reshape(3, T)
        okay = dev <= eps
        cont_axes = [a for a in range(3) if okay[a, :steps - 1].all()]
        cont = min(cont_axes, key=lambda a: (dev[a, :steps - 1].max(), a)) if cont_axes else None
        folds = [0, 0, 0]
        for a in range(3):
            if a == cont:
                continue
            for n in range(int(max_fold), 1, -1):
                if okay[a, _fold_positions(turns, n, steps)].all():
                    folds[a] = n
                    break
        half = _fold_positions(turns, 2, steps)[0]
        if cont is not None:
            elems, truncated = [cand[k][a * T + half] for a in range(3) if a != cont and okay[a, half]], False
        else:
            elems, truncated = close_group([cand[k][a * T + i] for a in range(3) if folds[a] for i in _fold_positions(turns, folds[a], steps)])
        known = []
        for e in elems:
            hit = np.flatnonzero(np.abs(cand[k] - e).max(1) < SAME)
            known.append(float(dev.reshape(-1)[hit[0]]) if len(hit) else None)
        work.append((elems, known, [i for i, d in enumerate(known) if d is None]))
        sidecar[str(oid)] = {"diameter": dia, "eps": eps, "frame": {"kind": frame_kind, "centre": c.tolist(), "axes": axes.tolist()},
                             "n_queries": None if queries is None else int(len(queries[k])), "continuous_axis": cont, "folds": folds,
                             "candidates": [{"turns": dev[a, :steps - 1].tolist(),
                                             "extra": [{"n": l[1], "k": l[2], "dev": float(dev[a, i])} for i, (l, _) in enumerate(turns) if l[0] == "f"]} for a in range(3)],
                             "truncated": bool(truncated), "closed": True}
    asked = [k for k, (_, _, new) in enumerate(work) if new]  # the second call: the closure elements that were no candidates
    extra = dict(zip(asked, score([(k, np.stack([work[k][0][i] for i in work[k][2]]), None if queries is None else queries[k]) for k in asked])))
    for k, (elems, known, new) in enumerate(work):
        side = sidecar[str(ids[k])]
        for i, d in zip(new, extra.get(k, ())):
            known[i] = float(d)
        eps = side["eps"]
        side["closed"] = all(d <= eps for d in known)
        side["elements"] = [{"dev": d, "candidate": i not in new, "kept": bool(d <= eps)} for i, d in enumerate(known)]
        kept = [e for e, d in zip(elems, known) if d <= eps]
        out = {}
        if kept:
            out["symmetries_discrete"] = [np.concatenate((e.reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]])).reshape(16).tolist() for e in kept]
        if side["continuous_axis"] is not None:
            a = np.asarray(side["frame"]["axes"][side["continuous_axis"]], np.float64)
            out["symmetries_continuous"] = [{"axis": (a / np.linalg.norm(a)).tolist(), "offset": side["frame"]["centre"]}]
        proposal[ids[k]] = out
    return proposal, {"eps_abs": float(eps_abs), "eps_rel": float(eps_rel), "max_fold": int(max_fold), "steps": int(steps), "objects": sidecar}
