"""The sampler library and the resident training set without a GPU (lc_amd/csrc/sampler/, include/lc_amd_sampler.h, lc_amd/sampler.py,
lc_amd/trainset.py): the library's place in the registry, header = exports = ctypes table, what the compiler made of the three kernels, the
refusals of the three entry points reached with host pointers (nothing launches), the host restatements -- the epoch's order is a
bijection, an epoch's primaries are every annotation once, the selection's hand-written cases -- and every refusal of the wrappers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sampler_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_is_the_fifth_of_the_third_tuple_and_of_no_other():
    import __graft_entry__ as entry
    from lc_amd import build, sampler

    T = build.SAMPLER
    assert build.EXTRA_TARGETS[:5] == (build.SHADE, build.OBOX, build.SYMFIND, build.TEXTURE, T) and T not in build.TARGETS + build.LATER_TARGETS
    assert T == build._side("sampler", (build.KEYED_HASH_H, build.WAVE_INT_H))
    assert T.src_dir == os.path.join(build.CSRC, "sampler") and T.header == "lc_amd_sampler.h" and T.hash_marker == b"LC_AMD_SAMPLER_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_sampler.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_sampler.so " in doc and "lc_amd/csrc/sampler/ " in doc and "include/lc_amd_sampler.h " in doc
    entry.build()
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = sampler.load()
    assert lib.lc_amd_sampler_version() == 1
    assert lib.lc_amd_sampler_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    every = build.TARGETS + build.LATER_TARGETS + build.EXTRA_TARGETS
    assert every.count(T) == 1 and len({t.so_path for t in every}) == len({t.hash_marker for t in every}) == len({build.source_hash(t) for t in every}) == len(every)
    for other in every:  # no other library sees this one's files or carries its marker, and the reverse
        if other is T:
            continue
        assert not any("sampler" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    own = {os.path.join(T.src_dir, "lc_sampler.hip"), os.path.join(ROOT, "include", T.header)}
    assert {os.path.normpath(d) for d in build._deps(T)} == own | {build.KEYED_HASH_H, build.WAVE_INT_H}
    assert not any("shade" in os.path.basename(d) for d in own)
    source = open(build.sources(T)[0]).read()
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_sampler.h", "../shared/lc_keyed_hash.h", "../shared/lc_wave_int.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_SAMPLER_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomic" not in code and "hipMalloc" not in code and "hipMemset" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert code.count("hipLaunchKernelGGL") == 3 and "fmix32(unsigned" not in code and "wave_sum(int" not in code  # the shared pieces are used, not restated
    assert build.build_later.__doc__ and "EXTRA_TARGETS" in build.build_later.__doc__


def test_header_exports_and_the_ctypes_table_agree():
    from lc_amd import augment, build, sampler

    T = build.SAMPLER
    sampler.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    entries = ("lc_sampler_rows", "lc_sampler_select_i32", "lc_sampler_take_rows")
    assert declared == set(sampler._SIGNATURES) and set(entries) <= declared and len(declared) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared

    def define(name):
        return int(re.search(rf"#define {name} (\w+)", header).group(1).rstrip("u"), 0)

    assert define("LC_AMD_SAMPLER_VERSION") == 1
    assert (sampler.MAX_ROWS, sampler.MAX_N, sampler.MAX_STEP_BITS, sampler.MAX_TENSORS, sampler.MAX_ROW_BYTES) == tuple(
        define("LC_SAMPLER_" + n) for n in ("MAX_ROWS", "MAX_N", "MAX_STEP_BITS", "MAX_TENSORS", "MAX_ROW_BYTES")) == (65536, 2 ** 31 - 1, 40, 16, 2 ** 30)
    assert sampler.OP_SPARE == define("LC_SAMPLER_OP_SPARE") == augment.OP_ZOOM + 1 and sampler.OP_PERM == define("LC_SAMPLER_OP_PERM") == augment.OP_ZOOM + 2
    assert sampler.ROUNDS == tuple(define(f"LC_SAMPLER_ROUND_{r}") for r in range(4)) and len(set(sampler.ROUNDS)) == 4
    assert define("LC_SAMPLER_TABLE_POINTERS") == len(sampler.FIELDS) == 10 and define("LC_SAMPLER_ROWS_POINTERS") == len(sampler.Rows._fields) == 12
    assert sampler.Rows._fields == ("index",) + sampler.FIELDS + ("info",)
    pp = ctypes.POINTER(ctypes.c_void_p)
    kinds_of = {ctypes.c_void_p: "p", pp: "p", ctypes.POINTER(ctypes.c_uint64): "p", ctypes.c_int: "i", ctypes.c_uint64: "u"}
    for name in entries:
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "uint64_t": "u"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = sampler._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)


def test_three_kernels_without_scratch_or_spills(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, sampler

    sampler.load()
    res = kernel_resources(build.SAMPLER.so_path)
    assert len(res) == 3, sorted(res)
    for short, threads, lds in (("lc_sampler_rows_kernel", 64, 0), ("lc_sampler_select_kernel", 1024, 1024 * 24 + 64), ("lc_sampler_take_kernel", 256, 0)):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs, {d.get('group_segment_fixed_size', 0)} B of LDS", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == threads and d.get("group_segment_fixed_size", 0) == lds, short


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import sampler

    lib = sampler.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_sampler_last_error

    def ptrs(n, **change):
        a = (ctypes.c_void_p * n)(*([p] * n))
        for i, v in change.items():
            a[int(i[1:])] = v
        return a

    def rows(seed=p, N=5, B=2, S=1, table=ptrs(10), out=ptrs(12)):
        return lib.lc_sampler_rows(seed, 0, N, B, S, table, out, None)

    for kw in (dict(B=0), dict(S=-1), dict(B=65536, S=1)):
        assert rows(**kw) == 1 and b"lc_sampler_rows: 1 <= B" in msg(), kw
    assert rows(seed=None) == 2 and b"seed must not be NULL" in msg()
    assert rows(out=None) == 2 and rows(table=None) == 2 and b"table must not be NULL" in msg()
    assert rows(seed=p + 4) == 7 and b"aligned to 8" in msg()
    assert rows(out=ptrs(12, _11=None)) == 2 and b"out[11]" in msg()
    assert rows(out=ptrs(12, _3=p + 2)) == 7 and b"out[3]" in msg()
    assert rows(table=ptrs(10, _9=None)) == 2 and b"table[9]" in msg()
    assert rows(table=ptrs(10, _0=p + 1)) == 7 and b"table[0]" in msg()

    def select(cnt=p, info=p, B=2, R=4, take=p, short=p):
        return lib.lc_sampler_select_i32(cnt, info, 100, B, R, take, short, None)

    for kw in (dict(R=0), dict(R=65537), dict(B=0), dict(B=5)):
        assert select(**kw) == 1 and b"lc_sampler_select_i32: 1 <= B <= rows" in msg(), kw
    for name in ("cnt", "info", "take", "short"):
        assert select(**{name: None}) == 2 and select(**{name: p + 2}) == 7, name

    def take(t=p, B=2, R=4, n=1, src=ptrs(1), dst=ptrs(1), nbytes=(16,)):
        return lib.lc_sampler_take_rows(t, B, R, n, src, dst, (ctypes.c_uint64 * len(nbytes))(*nbytes), None)

    for kw in (dict(B=0), dict(R=0), dict(B=65537), dict(R=65537)):
        assert take(**kw) == 1, kw
    assert take(n=0) == 3 and take(n=17) == 3 and b"1 <= n <= 16" in msg()
    assert take(t=None) == 2 and take(src=None) == 2 and take(dst=None) == 2 and take(t=p + 2) == 7
    assert take(src=ptrs(1, _0=None)) == 2 and take(dst=ptrs(1, _0=None)) == 2 and b"src[0] and dst[0]" in msg()
    assert take(nbytes=(0,)) == 4 and take(nbytes=(2 ** 30 + 1,)) == 4 and b"row_bytes" in msg()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 65537])
def test_the_epoch_order_is_a_bijection(n):
    from lc_amd.sampler import permute_host

    a = permute_host(12345, 0, n)
    assert a.dtype == np.int64 and np.array_equal(np.sort(a), np.arange(n))
    if n >= 16:
        assert not np.array_equal(a, permute_host(12345, 1, n)) and not np.array_equal(a, permute_host(12346, 0, n))
        assert not np.array_equal(a, permute_host(12345, 2 ** 32, n)) and not np.array_equal(a, permute_host(12345 + 2 ** 32, 0, n))  # the upper halves count
        assert not np.array_equal(a, np.arange(n))
    assert np.array_equal(permute_host(12345, 0, n, [n - 1, 0]), a[[n - 1, 0]])


@pytest.mark.parametrize("n,batch", [(257, 32), (5, 7)])
def test_an_epoch_s_primaries_are_every_annotation_once(n, batch):
    from lc_amd.sampler import draw_rows_host, permute_host

    seed0, spare, drawn = 2 ** 63 + 11, 5, []
    for step in range(-(-n // batch)):
        rows = draw_rows_host(n, seed=(seed0 + step) % 2 ** 64, seed0=seed0, batch=batch, spare=spare)
        assert rows.index.dtype == np.int32 and rows.index.shape == (batch + spare,) and not rows.info.any()
        assert ((rows.index[batch:] >= 0) & (rows.index[batch:] < n)).all()
        drawn += rows.index[:batch].tolist()
    assert sorted(drawn[:n]) == list(range(n)) and drawn[:n] == permute_host(seed0, 0, n).tolist()
    assert drawn[n:] == permute_host(seed0, 1, n).tolist()[:len(drawn) - n]  # an epoch changes inside a batch


def test_draw_rows_host_copies_the_records_and_refuses_rows():
    from lc_amd.sampler import FIELDS, AnnotationTable, draw_rows_host

    cols = AnnotationTable.validate(**cases.table_columns(17))
    rows = draw_rows_host(cols, seed=9, seed0=7, batch=7, spare=3)
    for name in FIELDS:
        assert np.array_equal(getattr(rows, name), cols[name][rows.index]), name
    assert rows.cam_K.shape == (10, 3, 3) and rows.t.shape == (10, 3) and rows.bbox_xyxy.dtype == np.float32
    for kw in (dict(seed=2 ** 40, seed0=0), dict(seed=0, seed0=1)):  # step = 2^40, and step = 2^64 - 1
        r = draw_rows_host(cols, batch=2, spare=1, **kw)
        assert (r.index == -1).all() and (r.info == -1).all() and (r.obj_id == -1).all() and np.isnan(r.R).all() and np.isnan(r.bbox_xyxy).all()
    assert not draw_rows_host(cols, seed=2 ** 40 - 1, seed0=0, batch=2, spare=1).info.any()
    r = draw_rows_host(0, seed=0, seed0=0, batch=2, spare=1)
    assert (r.index == -1).all() and (r.info == -1).all()
    hurt = dict(cols, mesh_index=np.where(np.arange(17) == rows.index[1], -1, cols["mesh_index"]).astype(np.int32))
    r = draw_rows_host(hurt, seed=9, seed0=7, batch=7, spare=3)
    bad = rows.index == rows.index[1]
    assert (r.info[bad] == -1).all() and (r.index[bad] == -1).all() and np.isnan(r.t[bad]).all() and not r.info[~bad].any() and np.array_equal(r.index[~bad], rows.index[~bad])


@pytest.mark.parametrize("case", cases.SELECT_CASES, ids=[c[0] for c in cases.SELECT_CASES])
def test_select_rows_host_on_hand_written_cases(case):
    from lc_amd.sampler import select_rows_host

    _, cnt, info, batch, want, shortfall = case
    take, short = select_rows_host(np.array(cnt, np.int32), np.array(info, np.int32), batch=batch, valid_th=cases.TH)
    assert take.dtype == np.int32 and take.tolist() == want and short == shortfall == want.count(-1)


def test_annotation_table_refusals():
    from lc_amd.sampler import AnnotationTable

    good = cases.table_columns(6)
    AnnotationTable.validate(**good, n_frames=3, n_masks=6, n_meshes=2)
    AnnotationTable.validate(**dict(good, cam_K=good["cam_K"][0], t=good["t"][:, :, None]))

    def bad(error, match, **change):
        with pytest.raises(error, match=match):
            AnnotationTable.validate(**{**good, **{k: v for k, v in change.items() if not k.startswith("n_")}}, **{k: v for k, v in change.items() if k.startswith("n_")})

    bad(TypeError, "frame_index must hold whole numbers", frame_index=good["frame_index"].astype(np.float32))
    bad(TypeError, "obj_id is a host array", obj_id=torch.zeros(6, dtype=torch.int32))
    bad(TypeError, "R is a host array", R=torch.zeros(6, 3, 3))
    bad(TypeError, "t must hold numbers", t=np.zeros((6, 3), dtype=complex))
    bad(ValueError, r"im_id has shape \(6, 1\)", im_id=good["im_id"][:, None])
    bad(ValueError, "mask_index has 5 rows", mask_index=good["mask_index"][:5])
    bad(ValueError, "scene_id must fit int32", scene_id=np.full(6, 2 ** 31, np.int64))
    bad(ValueError, "1 to 2147483647 annotations", **{k: v[:0] for k, v in good.items()})
    bad(ValueError, r"mesh_index must lie in \[0, 2\^31\), got -1", mesh_index=np.array([0, 1, 0, -1, 0, 1]))
    bad(ValueError, r"frame_index must lie in \[0, 2\), got 0 to 2", n_frames=2)
    bad(ValueError, r"mask_index must lie in \[0, 5\)", n_masks=5)
    bad(ValueError, r"mesh_index must lie in \[0, 1\)", n_meshes=1)
    bad(TypeError, "n_frames must be a whole number", n_frames=3.0)
    bad(ValueError, r"bbox_xyxy has shape \(6, 5\)", bbox_xyxy=np.zeros((6, 5), np.float32))
    bad(ValueError, r"cam_K has shape \(5, 3, 3\)", cam_K=good["cam_K"][:5])
    bad(ValueError, "R must be finite", R=np.where(np.arange(54).reshape(6, 3, 3) == 7, np.nan, good["R"]))
    bad(ValueError, "t must be finite", t=np.full((6, 3), 1e39))  # infinite as float32
    with pytest.raises(RuntimeError, match="the table lives on a HIP device, got cpu"):
        AnnotationTable(**good, device="cpu")


def test_wrapper_refusals():
    from lc_amd import sampler

    class FakeTable(sampler.AnnotationTable):
        def __init__(self):
            self.N, self.device = 6, torch.device("cpu")

    with pytest.raises(TypeError, match="table must be an AnnotationTable"):
        sampler.draw_rows(cases.table_columns(6), seed=0, seed0=0, batch=2, spare=1)
    tb = FakeTable()
    for error, match, kw in ((TypeError, "seed must be a whole number", dict(seed=1.5)), (ValueError, "seed of 0 to", dict(seed=2 ** 64)),
                             (TypeError, "a seed tensor holds one uint64 or int64 element", dict(seed=torch.zeros(2, dtype=torch.int64))),
                             (TypeError, "a seed tensor holds one", dict(seed=torch.zeros(1, dtype=torch.int32))),
                             (TypeError, "seed0 must be a whole number", dict(seed0=torch.zeros(1, dtype=torch.int64))), (ValueError, "seed0 of 0 to", dict(seed0=-1)),
                             (ValueError, "batch of 1 to 65536, got 0", dict(batch=0)), (TypeError, "batch must be a whole number", dict(batch=True)),
                             (ValueError, "spare of 0 to 65536, got -1", dict(spare=-1)), (ValueError, "batch \\+ spare of at most 65536", dict(batch=65536, spare=1))):
        with pytest.raises(error, match=match):
            sampler.draw_rows(tb, **{**dict(seed=0, seed0=0, batch=2, spare=1), **kw})

    cnt, info = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for error, match, a, kw in ((TypeError, "valid_cnt must be a torch.Tensor", (cnt.numpy(), info), {}), (TypeError, "valid_cnt must be int32", (cnt.long(), info), {}),
                                (ValueError, r"valid_cnt has shape \(4, 1\)", (cnt[:, None], info), {}), (ValueError, r"info has shape \(3,\)", (cnt, info[:3]), {}),
                                (TypeError, "info must be int32", (cnt, info.float()), {}), (ValueError, "1 to 65536 rows, got 0", (cnt[:0], info[:0]), {}),
                                (ValueError, "batch of 1 to 4, got 5", (cnt, info), dict(batch=5)), (ValueError, "batch of 1 to 4, got 0", (cnt, info), dict(batch=0)),
                                (TypeError, "valid_th must be a whole number", (cnt, info), dict(valid_th=1.0)), (ValueError, "valid_th of", (cnt, info), dict(valid_th=2 ** 31)),
                                (RuntimeError, "valid_cnt is on cpu", (cnt, info), {})):
        with pytest.raises(error, match=match):
            sampler.select_rows(*a, **{**dict(batch=2, valid_th=100), **kw})

    take, x = torch.zeros(2, dtype=torch.int32), torch.zeros(4, 3)
    for error, match, a, kw in ((TypeError, "take must be int32", (take.long(), x), {}), (ValueError, r"take has shape \(2, 1\)", (take[:, None], x), {}),
                                (ValueError, "take holds 1 to 65536 rows, got 0", (take[:0], x), {}), (ValueError, "needs at least one tensor", (take,), {}),
                                (TypeError, r"tensors\[1\] must be a torch.Tensor", (take, x, x.numpy()), {}), (ValueError, r"tensors\[0\] has no rows", (take, x.sum()), {}),
                                (ValueError, r"tensors\[1\] has 3 rows, tensors\[0\] has 4", (take, x, x[:3]), {}), (ValueError, "rows of 0 bytes", (take, x[:, :0]), {}),
                                (ValueError, "out holds one tensor per source", (take, x), dict(out=())), (TypeError, r"out\[0\] must be torch.float32", (take, x), dict(out=(x[:2].double(),))),
                                (ValueError, r"out\[0\] has shape \(4, 3\), expected \(2, 3\)", (take, x), dict(out=(x,))),
                                (ValueError, r"out\[0\] must be contiguous", (take, x), dict(out=(torch.zeros(3, 2).t(),))), (RuntimeError, "take is on cpu", (take, x), {})):
        with pytest.raises(error, match=match):
            sampler.take_rows(*a, **kw)


def test_trainset_refusals():
    from lc_amd import sampler
    from lc_amd.augment import AugmentConfig
    from lc_amd.trainset import TrainSet

    class FakeTable(sampler.AnnotationTable):
        def __init__(self):
            self.N, self.device, self.columns = 6, torch.device("cpu"), {"frame_index": torch.zeros(6, dtype=torch.int32)}

    frames, masks = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(6, 48, 64, dtype=torch.uint8)
    good = dict(masks=masks, cfg=AugmentConfig(), seed0=5, batch=4, spare=4, in_hw=(32, 32), out_hw=(16, 16))

    def bad(error, match, frames=frames, table=FakeTable(), **change):
        with pytest.raises(error, match=match):
            TrainSet(frames, table, **{**good, **change})

    bad(ValueError, "one of the two", masks=None)
    bad(ValueError, "one of the two", rle_store=object())
    bad(TypeError, "rle_store must be an RleStore", masks=None, rle_store=object())
    bad(ValueError, "at most one of the two", backgrounds=torch.zeros(1, 3, 32, 32, dtype=torch.uint8), background_store=object())
    bad(TypeError, "background_store must be a BackgroundStore", background_store=object())
    bad(TypeError, "table must be an AnnotationTable", table=cases.table_columns(6))
    bad(TypeError, "cfg must be an AugmentConfig", cfg=None)
    bad(TypeError, "meshes must be a MeshSet", meshes=object(), near=0.1, far=10.0)
    bad(ValueError, "near given without meshes", near=0.1)
    bad(TypeError, "frames must be uint8", frames=frames.float())
    bad(ValueError, r"frames has shape \(2, 48, 64\)", frames=frames[..., 0])
    bad(ValueError, "in_hw is a pair", in_hw=32)
    bad(ValueError, "out_hw of 1 to 16384, got 0", out_hw=(0, 16))
    bad(TypeError, "seed0 must be a whole number", seed0=1.0)
    bad(ValueError, "seed0 of 0 to", seed0=2 ** 64)
    bad(ValueError, "batch of 1 to 65536, got 0", batch=0)
    bad(ValueError, "spare of 0 to 65536, got -1", spare=-1)
    bad(ValueError, r"batch \+ spare of at most 65536", batch=40000, spare=40000)
    bad(TypeError, "valid_th must be a whole number", valid_th=1.5)
    bad(ValueError, "n_check of 0 to 256, got 257", n_check=257)
    bad(ValueError, "vis_interp must be one of", vis_interp="cubic")
    bad(TypeError, "dtype must be one of", dtype=torch.float64)
    bad(ValueError, r"masks has shape \(6, 48, 60\)", masks=masks[:, :, :60])
    bad(RuntimeError, "frames is on cpu")
