"""The training mask crops without a GPU: the numpy restatement (tests/maskcrop_oracle.py) against OpenCV's float path restated in
float32 and against the existing 8-bit oracle, the round rule and the hash's uniformity, and the library and its wrapper
(lc_amd.maskcrop) as far as they go without a device: build group, header, exports, source hash, every refusal."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import crops_oracle, maskcrop_cases as cases, maskcrop_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", cases.WARPS, ids=lambda c: c.name)
def test_linear_msk_vis_is_opencvs_float_path_bit_for_bit(case):
    window = cases.mask(case.mask_hw, case.seed)
    k = oracle.linear_count(window, case.origin, case.M, case.out_hw)
    assert k.min() >= 0 and k.max() <= 1024
    vis, _ = oracle.warp_row(window, case.origin, case.M, case.out_hw, oracle.LINEAR)
    emu = oracle.opencv_float_linear(window, case.origin, case.M, case.out_hw)
    assert vis.dtype == emu.dtype == np.float32
    assert np.array_equal(vis.view(np.uint32), emu.view(np.uint32))
    assert np.array_equal(vis.astype(np.float64) * 1024.0, k.astype(np.float64))  # k / 1024 exactly


def test_the_case_list_reaches_partial_weights_and_the_window_edges():
    seen_partial = seen_outside = seen_inside = False
    for case in cases.WARPS:
        window = cases.mask(case.mask_hw, case.seed)
        k = oracle.linear_count(window, case.origin, case.M, case.out_hw)
        t, _, _ = oracle.linear_parts(np.ones_like(window), case.origin, case.M, case.out_hw)
        inside = sum(t)
        seen_partial |= bool(((k > 0) & (k < 1024)).any())
        seen_outside |= bool(((inside > 0) & (inside < 4)).any())  # a pixel whose four taps straddle the window's edge
        seen_inside |= bool((inside == 4).any())
    assert seen_partial and seen_outside and seen_inside


@pytest.mark.parametrize("case", cases.WARPS, ids=lambda c: c.name)
def test_msk_noc_is_the_8_bit_oracles_nearest_warp(case):
    """Tied to the existing yardstick: the window embedded at its origin in a frame that holds it, 255 where set."""
    window = cases.mask(case.mask_hw, case.seed)
    _, noc = oracle.warp_row(window, case.origin, case.M, case.out_hw)
    frame, shift = cases.embed(window, case.origin)
    M = np.asarray(case.M, dtype=np.float32)
    if shift == (0, 0):
        ref = crops_oracle.warp_one((255 * frame)[..., None], M, case.out_hw, crops_oracle.NEAREST)[..., 0] > 127
        assert np.array_equal(noc.astype(bool), ref)
    # with a negative origin the frame would need negative pixels: there the same taps are read from the oracle's own coordinates
    X, Y = crops_oracle.coordinates(M, case.out_hw, crops_oracle.NEAREST)
    sx, sy = (X >> 10) + shift[0], (Y >> 10) + shift[1]
    H, W = frame.shape
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    ref = np.where(inside, frame[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)] != 0, False)
    assert np.array_equal(noc.astype(bool), ref)


def test_the_case_list_notices_a_contracted_row_term():
    """The fma row: forming m01 * y + b1 with one rounding (crops_oracle's planted mistake "fma") moves at least one pixel of msk_noc or
    msk_vis there, so a device copy of the coordinates that lets the compiler contract that expression cannot pass test_gpu_maskcrop."""
    by_name = {c.name: c for c in cases.WARPS}
    case = by_name["fma-row"]
    assert case.out_hw == (16, 16) and case.mask_hw[0] <= 48 and case.mask_hw[1] <= 40 and by_name["ties"].out_hw == (16, 16)
    window = cases.mask(case.mask_hw, case.seed)
    vis, noc = cases.moved_by(window, case.origin, case.M, case.out_hw, "fma")
    print("pixels moved by the contraction: msk_vis", vis, "msk_noc", noc)
    assert vis + noc >= 1
    assert crops_oracle.coordinates is cases.crops_oracle.coordinates and cases.moved_by(window, case.origin, case.M, case.out_hw, None) == (0, 0)
    from tests import crops_cases

    assert np.array_equal(np.asarray(by_name["ties"].M, dtype=np.float32), dict(crops_cases.CASES)["ties"])


@pytest.mark.parametrize("valid,n_check", [(1, 256), (2, 255), (100, 256), (255, 256), (256, 256), (257, 256), (300, 1), (4096, 256), (7, 20)])
def test_every_round_is_a_permutation(valid, n_check):
    noc = cases.noc_with(valid, (64, 64), seed=valid)
    assert int(noc.sum()) == valid
    rs = oracle.rounds(noc, n_check, seed=11, sample_id=5)
    set_p = set(np.flatnonzero(noc.reshape(-1)).tolist())
    assert sum(len(r) for r in rs) == n_check
    for i, r in enumerate(rs):
        assert len(set(r.tolist())) == len(r) and set(r.tolist()) <= set_p
        assert len(r) == (valid if i < len(rs) - 1 else n_check - valid * (len(rs) - 1))
    if len(rs) > 2 and valid >= 100:
        assert not np.array_equal(rs[0], rs[1])  # another round, another order (100! orders: equal ones would be a defect of the key)
    pts = oracle.check_points(noc, valid, n_check, 11, 5)
    assert pts.shape == (n_check, 2) and noc[pts[:, 1], pts[:, 0]].all()
    assert (oracle.check_points(noc, valid + 1, n_check, 11, 5) == -1).all()  # valid_cnt < valid_th
    assert (oracle.check_points(np.zeros_like(noc), 0, n_check, 11, 5) == -1).all()  # nothing valid


def test_rounds_of_100_100_56():
    noc = cases.noc_with(100, (64, 64), seed=3)
    assert [len(r) for r in oracle.rounds(noc, 256, 0, 0)] == [100, 100, 56]


def test_the_hash_is_murmur3s_finaliser():
    # the finaliser's published test values (MurmurHash3 fmix32) and its fixed point
    assert int(oracle.fmix32(0)) == 0
    assert int(oracle.fmix32(1)) == 0x514E28B7
    assert int(oracle.fmix32(0xFFFFFFFF)) == 0x81F16F39
    # the header's chain, written out once more in Python integers
    def f(v):
        v ^= v >> 16
        v = (v * 0x85EBCA6B) & 0xFFFFFFFF
        v ^= v >> 13
        v = (v * 0xC2B2AE35) & 0xFFFFFFFF
        return v ^ (v >> 16)

    seed, sid, r, p = 0x123456789ABCDEF0, 77, 3, 4095
    assert int(oracle.key(seed, sid, r, p)) == f(f(f(f(f(seed & 0xFFFFFFFF) ^ (seed >> 32)) ^ sid) ^ r) ^ p)


@pytest.mark.parametrize("sweep", ["seed", "sample_id"])
def test_the_draw_is_uniform(sweep):
    """16 valid pixels, 4 drawn, 4 096 draws: every pixel's count within five binomial standard deviations of 1 024."""
    noc = np.zeros((8, 8), dtype=np.uint8)
    noc[2:6, 2:6] = 1
    counts = np.zeros(64, dtype=np.int64)
    for s in range(4096):
        pts = oracle.check_points(noc, 1, 4, s if sweep == "seed" else 7, 3 if sweep == "seed" else s)
        np.add.at(counts, pts[:, 1] * 8 + pts[:, 0], 1)
    assert counts[noc.reshape(-1) == 0].sum() == 0 and counts.sum() == 4 * 4096
    sd = (4096 * 0.25 * 0.75) ** 0.5
    dev = np.abs(counts[noc.reshape(-1) > 0] - 1024)
    print("largest deviation in standard deviations:", dev.max() / sd)
    assert dev.max() <= 5 * sd


def test_batch_contract_of_the_oracle():
    masks = np.stack([cases.mask((12, 10), s) for s in range(3)])
    M = np.tile(np.array([[1.0, 0.0, 0.5], [0.0, 1.0, -0.25]], dtype=np.float32), (5, 1, 1))
    M[3, 0, 1] = np.nan
    got = oracle.mask_crops(masks, M, (9, 11), mask_index=[2, 0, 3, 1, 0], origin=[[0, 0], [1, -2], [0, 0], [0, 0], [(1 << 24) + 1, 0]],
                            valid_th=1, n_check=8, seed=2)
    assert got["info"].tolist() == [0, 0, -1, -1, -1]
    for b in (2, 3, 4):
        assert not got["msk_vis"][b].any() and not got["msk_noc"][b].any() and got["valid_cnt"][b] == 0 and (got["sym_ck_pts2d"][b] == -1).all()
    assert got["valid_cnt"][0] > 0 and got["msk_noc"].dtype == bool and got["msk_vis"].dtype == np.float32


# ---- the library and its wrapper, without a device


def test_build_group_header_exports_and_source_hash():
    from lc_amd import build, maskcrop

    T = build.MASKCROP  # (its place among the libraries, its files and includes: tests/test_libraries_host.py)
    lib = maskcrop.load()
    assert not build.is_stale(T)
    assert lib.lc_amd_maskcrop_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert build.sources(T) == [os.path.join(build.CSRC, "maskcrop", "lc_maskcrop.hip")]

    header = open(os.path.join(ROOT, "include", "lc_amd_maskcrop.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(maskcrop._SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_maskcrop_version() == int(re.search(r"#define LC_AMD_MASKCROP_VERSION (\d+)", header).group(1)) == 1
    for name, have in (("MAX_SIZE", maskcrop.MAX_SIZE), ("MAX_ORIGIN", maskcrop.MAX_ORIGIN), ("MAX_CHECK", maskcrop.MAX_CHECK),
                       ("MAX_CHECK_PIXELS", maskcrop.MAX_CHECK_PIXELS), ("NEAREST", maskcrop.INTERP["nearest"]), ("LINEAR", maskcrop.INTERP["linear"]),
                       ("I32", maskcrop.CK_DTYPES[torch.int32]), ("I64", maskcrop.CK_DTYPES[torch.int64])):
        assert have == int(re.search(rf"#define LC_MASKCROP_{name} (\d+)", header).group(1)), name
    assert maskcrop.MAX_CHECK_PIXELS >= 65536 and maskcrop.MAX_ORIGIN == oracle.MAX_ORIGIN
    from lc_amd import gtinfo

    assert maskcrop.MAX_ORIGIN == gtinfo.MAX_ORIGIN  # "the bound gtinfo uses"
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_size_t: "8", ctypes.c_uint64: "8"}  # (one ctypes type where size_t has 64 bits)
    for name in ("lc_mask_crops_u8", "lc_mask_crops_workspace_bytes"):
        m = re.search(rf"(int|size_t) {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "size_t": "8", "uint64_t": "8"}[a.split()[0]] for a in m.group(2).split(",")]
        res, args = maskcrop._SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)], name
        assert kinds == [kinds_of[a] for a in args], (name, kinds)
    wb = lib.lc_mask_crops_workspace_bytes
    assert wb(3, 5, 7, 256, 1, 1) == 0 and wb(3, 5, 7, 0, 0, 0) == 0 and wb(3, 5, 7, 4, 1, 0) == 12 and wb(3, 5, 7, 4, 0, 0) == 12 + 108 and wb(0, 5, 7, 4, 0, 0) == 0


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, maskcrop

    maskcrop.load()
    res = kernel_resources(build.MASKCROP.so_path)
    assert len(res) == 4 and all("lc_mask_" in n for n in res), sorted(res)
    for d in res.values():
        assert d.get("private_segment_fixed_size", 0) == 0, (d["name"], "scratch")
        assert d["vgpr_count"] <= 128, d["name"]
        assert d.get("group_segment_fixed_size", 0) <= 4096, d["name"]


def _good(B=3):
    return dict(masks=torch.zeros(2, 6, 7, dtype=torch.uint8), M=torch.zeros(B, 2, 3), out_hw=(4, 5))


def test_wrapper_refusals():
    from lc_amd import maskcrop

    f = maskcrop.mask_crops
    with pytest.raises(TypeError, match="masks must be a torch.Tensor"):
        f(**dict(_good(), masks=np.zeros((2, 6, 7), np.uint8)))
    with pytest.raises(TypeError, match="masks must be uint8 or bool"):
        f(**dict(_good(), masks=torch.zeros(2, 6, 7)))
    with pytest.raises(ValueError, match=r"masks has shape \(6, 7\)"):
        f(**dict(_good(), masks=torch.zeros(6, 7, dtype=torch.uint8)))
    with pytest.raises(TypeError, match="M must be float32"):
        f(**dict(_good(), M=torch.zeros(3, 2, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"M has shape \(3, 3, 3\)"):
        f(**dict(_good(), M=torch.zeros(3, 3, 3)))
    with pytest.raises(ValueError, match="out_hw is a pair"):
        f(**dict(_good(), out_hw=4))
    with pytest.raises(TypeError, match="out_hw must be a whole number"):
        f(**dict(_good(), out_hw=(4.0, 5)))
    with pytest.raises(ValueError, match="out_hw of 1 to 16384"):
        f(**dict(_good(), out_hw=(0, 5)))
    with pytest.raises(ValueError, match="mask sizes of 1 to 16384"):
        f(**dict(_good(), masks=torch.zeros(1, 1, 16385, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="vis_interp must be one of"):
        f(**_good(), vis_interp="cubic")
    with pytest.raises(TypeError, match="valid_th must be a whole number"):
        f(**_good(), valid_th=1.5)
    with pytest.raises(ValueError, match="n_check of 0 to 256"):
        f(**_good(), n_check=257)
    with pytest.raises(ValueError, match="seed of 0 to"):
        f(**_good(), seed=-1)
    with pytest.raises(TypeError, match="seed must be a whole number"):
        f(**_good(), seed=torch.tensor(1))
    with pytest.raises(TypeError, match="ck_dtype"):
        f(**_good(), ck_dtype=torch.int16)
    with pytest.raises(ValueError, match="want holds names"):
        f(**_good(), want=("msk_in",))
    with pytest.raises(ValueError, match="want holds names"):
        f(**_good(), want="msk_vis")
    with pytest.raises(ValueError, match="at most 65536 pixels"):
        f(**dict(_good(), out_hw=(256, 257)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the same crop without check points is in order
        f(**dict(_good(), out_hw=(256, 257)), n_check=0)
    with pytest.raises(TypeError, match="mask_index must be int32"):
        f(**_good(), mask_index=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"mask_index has shape \(2,\)"):
        f(**_good(), mask_index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="origin must be int32 or int64"):
        f(**_good(), origin=torch.zeros(3, 2))
    with pytest.raises(ValueError, match=r"origin has shape \(3,\)"):
        f(**_good(), origin=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="sample_id must be int32"):
        f(**_good(), sample_id=torch.zeros(3))
    with pytest.raises(ValueError, match="out holds tensors under names"):
        f(**_good(), out=dict(msk_in=torch.zeros(3, 4, 5)))
    with pytest.raises(ValueError, match="want does not name"):
        f(**_good(), want=("msk_noc",), out=dict(msk_vis=torch.zeros(3, 4, 5)))
    with pytest.raises(TypeError, match=r"out\['msk_vis'\] must be float32"):
        f(**_good(), out=dict(msk_vis=torch.zeros(3, 4, 5, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"out\['sym_ck_pts2d'\] has shape"):
        f(**_good(), out=dict(sym_ck_pts2d=torch.zeros(3, 255, 2, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order: the masks are not on the HIP device
        f(**_good())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**dict(_good(), masks=torch.zeros(2, 6, 7, dtype=torch.bool)), origin=torch.full((3, 2), -4, dtype=torch.int64), sample_id=torch.zeros(3, dtype=torch.int32))


def test_entry_point_checks_its_arguments_before_launching():
    from lc_amd import maskcrop

    lib = maskcrop.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(masks=p, F=2, Hm=6, Wm=7, idx=None, org=None, M=p, B=3, h=4, w=5, interp=1, th=100, n=256, sid=None, ckd=1, vis=p, noc=p, cnt=p, ck=p, info=p,
             ws=None, nbytes=0):
        return lib.lc_mask_crops_u8(masks, F, Hm, Wm, idx, org, M, B, h, w, interp, th, n, 0, sid, ckd, vis, noc, cnt, ck, info, ws, nbytes, None)

    msg = lib.lc_amd_maskcrop_last_error
    assert call(B=-1) != 0 and b"lc_mask_crops_u8: B < 0" in msg()
    assert call(B=0) == 0 and call(B=0, masks=None, M=None) == 0  # an empty batch is a no-op
    assert call(F=-1) != 0 and b"F < 0" in msg()
    assert call(Hm=0) != 0 and b"16384" in msg()
    assert call(w=16385) != 0 and b"16384" in msg()
    assert call(interp=2) != 0 and b"vis_interp" in msg()
    assert call(n=257) != 0 and b"n_check" in msg()
    assert call(n=-1) != 0 and b"n_check" in msg()
    assert call(ckd=2) != 0 and b"ck_dtype" in msg()
    assert call(h=256, w=257) != 0 and b"65536 pixels" in msg()
    assert call(M=None) != 0 and b"NULL" in msg()
    assert call(masks=None) != 0 and b"NULL" in msg()
    assert call(M=p + 2) != 0 and b"aligned" in msg()
    assert call(ck=p + 4) != 0 and b"aligned" in msg()
    assert call(org=p + 1) != 0 and b"aligned" in msg()
    assert call(noc=None) != 0 and b"workspace is smaller" in msg()
    assert call(cnt=None, ws=p, nbytes=11) != 0 and b"workspace is smaller" in msg()


def test_wide_warps_reach_the_layouts_the_small_crops_stop_short_of():
    """tests/crops_cases.warp_grid restates the launch geometry both libraries share: the crops of WARPS end at 32 threads along x, the
    wide ones use 64, 128 and 256 and a second trip of the quad loop."""
    from tests import crops_cases

    assert max(crops_cases.warp_grid(*c.out_hw)[2] for c in cases.WARPS) == 5 and max(c.out_hw[1] for c in cases.WARPS) == 65
    assert {crops_cases.warp_grid(*c.out_hw)[2] for c in cases.WIDE_WARPS} == {6, 7, 8}
    assert {c.out_hw for c in cases.WIDE_WARPS} == set(crops_cases.WIDE_SIZES) and len(cases.WIDE_WARPS) == 2 * len(crops_cases.WIDE_SIZES)
    assert sum((c.out_hw[1] + 3) // 4 > 256 for c in cases.WIDE_WARPS) == 4
    assert all(c.out_hw[0] * c.out_hw[1] <= oracle.MAX_CHECK_PIXELS for c in cases.WIDE_WARPS)  # check points may be asked for


@pytest.mark.parametrize("case", cases.WIDE_WARPS, ids=lambda c: c.name)
def test_wide_warps_cross_the_windows_edges_and_notice_a_wrong_layout(case):
    """Every wide case reads inside and outside its window, over at least two of the window's sides, and both of its masks part from
    the oracle's under a row loop that steps by 8; under x terms formed from x mod 1024 they part exactly where there is a second trip."""
    window = cases.mask(case.mask_hw, case.seed)
    X, Y = crops_oracle.coordinates(case.M, case.out_hw, oracle.NEAREST)
    u, v = (X >> 10) - case.origin[0], (Y >> 10) - case.origin[1]
    sides = [bool(s.any()) for s in (u < 0, u >= case.mask_hw[1], v < 0, v >= case.mask_hw[0])]
    assert sum(sides) >= 2, sides
    for vis_interp in (oracle.LINEAR, oracle.NEAREST):
        vis, noc = oracle.warp_row(window, case.origin, case.M, case.out_hw, vis_interp)
        assert 0 < np.count_nonzero(noc) < noc.size
        if vis_interp == oracle.LINEAR:
            assert ((vis > 0) & (vis < 1)).any()
        bad_vis, bad_noc = cases.wide_planted(case, vis_interp, "row_stride_8")
        assert (bad_vis != vis).any() and (bad_noc != noc).any() and bad_noc.sum() != noc.sum()
        bad_vis, bad_noc = cases.wide_planted(case, vis_interp, "x_mod_1024")
        second_trip = case.out_hw[1] > 1024
        assert (bad_vis != vis).any() == second_trip and (bad_noc != noc).any() == second_trip
        assert np.array_equal(bad_vis[:, :1024], vis[:, :1024]) and np.array_equal(bad_noc[:, :1024], noc[:, :1024])


def test_depth_rows_have_the_depths_they_are_named_for():
    """The searched sample ids give a selection of every depth 0..3 on both crops; the search is deterministic, and the literal ids of the
    64 x 64 crop are what it returns (depths 0..2 are searched again here; depth 3 is re-derived, its search takes seconds)."""
    small, big = cases.depth_crop(64), cases.depth_crop(256)
    assert small.shape == (64, 64) and 0.55 < small.mean() < 0.65 and big.shape == (256, 256) and big.all()
    assert cases.find_depth_ids(small, depths=(0, 1, 2), tries=200) == {d: cases.DEPTH_IDS_64[d] for d in (0, 1, 2)}
    for size, crop in ((64, small), (256, big)):
        ids = cases.depth_ids(size)
        assert sorted(ids) == [0, 1, 2, 3] and len(set(ids.values())) == 4
        for d, sid in ids.items():
            assert oracle.selection_depth(crop, cases.DEPTH_N, cases.DEPTH_SEED, sid) == d, (size, d, sid)
            assert cases.boundary_pair(crop, cases.DEPTH_N, cases.DEPTH_SEED, sid)[0] == d
    assert cases.depth_ids(256) == cases.find_depth_ids(big)
    assert oracle.selection_depth(cases.noc_with(256, (64, 64), 1), 256, 0, 0) is None and oracle.selection_depth(cases.noc_with(257, (64, 64), 1), 256, 0, 0) in range(4)
    # the depth is what it says: the two keys share exactly that many leading bytes
    k = np.sort(oracle.key(cases.DEPTH_SEED, cases.depth_ids(256)[3], 0, np.arange(256 * 256)))
    assert k[255] >> np.uint64(8) == k[256] >> np.uint64(8) and k[255] != k[256]
    k = np.sort(oracle.key(cases.DEPTH_SEED, cases.depth_ids(256)[0], 0, np.arange(256 * 256)))
    assert k[255] >> np.uint64(24) != k[256] >> np.uint64(24)


@pytest.mark.parametrize("size", [64, 256])
def test_depth_3_rows_notice_a_selection_that_skips_the_last_key_byte(size):
    crop, sid = cases.depth_crop(size), cases.depth_ids(size)[3]
    good = oracle.check_points(crop, 1, cases.DEPTH_N, cases.DEPTH_SEED, sid)
    assert np.array_equal(good, cases.planted_points(crop, cases.DEPTH_N, cases.DEPTH_SEED, sid, None))  # the restatement itself
    bad = cases.planted_points(crop, cases.DEPTH_N, cases.DEPTH_SEED, sid, "top_24_bits")
    assert not np.array_equal(good, bad)
    assert {tuple(q) for q in good.tolist()} != {tuple(q) for q in bad.tolist()}  # another pixel is taken, not only another order
    for d in (0, 1, 2):  # and only there: on the shallower rows the last byte never decides which pixels are taken
        sid = cases.depth_ids(size)[d]
        good = oracle.check_points(crop, 1, cases.DEPTH_N, cases.DEPTH_SEED, sid)
        bad = cases.planted_points(crop, cases.DEPTH_N, cases.DEPTH_SEED, sid, "top_24_bits")
        assert {tuple(q) for q in good.tolist()} == {tuple(q) for q in bad.tolist()}


def test_large_p_masks_hold_the_pixel_index_at_its_full_width():
    masks = {name: (m, sid) for name, m, sid in cases.large_p_masks()}
    assert list(masks) == ["last-300", "last-rows-200", "exactly-256"]
    m, sid = masks["last-300"]
    p = np.flatnonzero(m.reshape(-1))
    assert p.tolist() == list(range(65236, 65536)) and (p >> 15).all()
    good = oracle.check_points(m, 100, cases.DEPTH_N, cases.DEPTH_SEED, sid)
    assert ((good[:, 1] * 256 + good[:, 0]) >= 65236).all() and len({tuple(q) for q in good.tolist()}) == 256
    bad = cases.planted_points(m, cases.DEPTH_N, cases.DEPTH_SEED, sid, "p_12_bits")
    assert not np.array_equal(good, bad) and (good != bad).any(axis=1).all()  # every point moves: each p has bits above the twelfth
    m, sid = masks["last-rows-200"]
    p = np.flatnonzero(m.reshape(-1))
    assert len(p) == 200 and p.min() >= 254 * 256 and oracle.selection_depth(m, cases.DEPTH_N, cases.DEPTH_SEED, sid) is None
    pts = oracle.check_points(m, 100, cases.DEPTH_N, cases.DEPTH_SEED, sid)
    assert (pts[:, 1] >= 254).all() and len(oracle.rounds(m, cases.DEPTH_N, cases.DEPTH_SEED, sid)) == 2
    m, sid = masks["exactly-256"]
    p = np.flatnonzero(m.reshape(-1))
    assert len(p) == 256 and p[0] == 0 and p[-1] == 65535 and oracle.selection_depth(m, cases.DEPTH_N, cases.DEPTH_SEED, sid) is None
    pts = oracle.check_points(m, 100, cases.DEPTH_N, cases.DEPTH_SEED, sid).tolist()
    assert [0, 0] in pts and [255, 255] in pts
