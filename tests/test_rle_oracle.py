"""The run-length mask store without a GPU: COCO's compressed string (hand-checked vectors, round trips), the numpy oracle against itself
(decode and encode are inverse up to the canonical form; windows; the index), the library of its own (group, header, exports, signatures,
source hash, kernel resources), every refusal of the three C entry points before any launch, and every refusal of the wrapper."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import rle_cases as cases, rle_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counts -> string, each checked by hand with the rule of include/lc_amd_rle.h's companion, lc_amd/rle.py
VECTORS = [([5], "5"), ([15], "?"), ([16], "`0"), ([31], "o0"), ([3, 2, 2], "32O"),
           ([0], "0"), ([32], "P1"),            # 32 = 0 + 1 * 32: group 0 with more -> 0x20 + 48 = 'P', then 1
           ([1024], "PP1"),                     # 0, 0, 1
           ([3, 2, 5], "322"),                  # 5 - 3 = 2
           ([10, 4, 10, 4], ":400"),            # both differences 0
           ([100, 7, 20], "T37`M"),             # 100 = 4 + 3 * 32: 'T' '3'; 7; 20 - 100 = -80: -80 & 31 = 16, more -> '`'; -3 & 31 = 29, bit 4, x = -1 -> 'M'
           ([], "")]


@pytest.mark.parametrize("counts,string", VECTORS, ids=[v[1] or "empty" for v in VECTORS])
def test_string_vectors(counts, string):
    from lc_amd import rle

    assert oracle.to_string(counts) == string and oracle.from_string(string) == counts
    assert rle.counts_to_string(counts) == string.encode() and rle.string_to_counts(string).tolist() == counts
    assert rle.string_to_counts(string.encode()).dtype == np.uint32


def test_string_round_trips_with_negative_and_wide_differences():
    from lc_amd import rle

    rng = np.random.default_rng(7)
    seen_negative = seen_wide = 0
    for trial in range(200):
        n = int(rng.integers(0, 60))
        hi = (8, 40, 70000, 2 ** 32)[trial % 4]
        c = rng.integers(0, hi, n).tolist()
        d = [c[i] - c[i - 2] for i in range(2, n)]
        seen_negative += any(v < 0 for v in d)
        seen_wide += any(abs(v) >= 2 ** 15 for v in d)
        s = oracle.to_string(c)
        assert all(48 <= ord(ch) <= 111 for ch in s)
        assert rle.counts_to_string(c) == s.encode() and rle.counts_to_string(np.asarray(c, dtype=np.uint32)) == s.encode()
        assert oracle.from_string(s) == c and rle.string_to_counts(s).tolist() == c
    assert seen_negative > 50 and seen_wide > 50
    ends = [2 ** 32 - 1, 0, 0, 2 ** 32 - 1, 2 ** 32 - 1, 0]  # the widest differences both ways
    assert rle.string_to_counts(rle.counts_to_string(ends)).tolist() == ends == oracle.from_string(oracle.to_string(ends))
    with pytest.raises(ValueError, match="48"):
        rle.string_to_counts("5 5")
    with pytest.raises(ValueError, match="ends inside a count"):
        rle.string_to_counts("5P")
    with pytest.raises(ValueError, match=r"outside \[0, 2\^32\)"):
        rle.string_to_counts("N")  # 30: bit 4 set, the last group: -2
    with pytest.raises(ValueError, match="more than 8 groups"):
        rle.string_to_counts("P" * 8 + "1")
    with pytest.raises(TypeError, match="bytes or str"):
        rle.string_to_counts([5])


@pytest.mark.parametrize("hw", cases.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_and_encode_are_inverse_up_to_the_canonical_form(hw):
    H, W = hw
    for name, c in cases.valid_lists(H, W):
        m = oracle.decode(c, H, W)
        assert m.shape == (H, W) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}, name
        canon = oracle.encode(m).tolist()
        assert sum(canon) == H * W and all(v > 0 for v in canon[1:]), name
        assert np.array_equal(oracle.decode(canon, H, W), m), name
        assert canon == [v for v in _merged(c)], name
        assert oracle.from_string(oracle.to_string(canon)) == canon, name
    assert oracle.encode(np.zeros((H, W))).tolist() == [H * W] and oracle.encode(np.full((H, W), 7)).tolist() == [0, H * W]
    for name, c in cases.invalid_lists(H, W):
        assert not oracle.is_valid(c, H, W), name
    assert sum(cases.invalid_lists(H, W)[2][1]) & 0xFFFFFFFF == H * W  # what 32 bits would have accepted


def _merged(counts):
    """The canonical list by list surgery alone: zero counts dropped with their neighbours joined."""
    out = [counts[0]]
    for k, c in enumerate(counts[1:], 1):
        if (len(out) - 1) % 2 == k % 2:
            out[-1] += c
        elif c > 0:
            out.append(c)
        # a zero count of the other value: nothing to add, and the next count joins the run before it
    return out


def test_oracle_closed_forms():
    H, W = 37, 53
    named = dict(cases.valid_lists(H, W))
    for name, xy in (("corner-tl", (0, 0)), ("corner-bl", (0, H - 1)), ("corner-tr", (W - 1, 0)), ("corner-br", (W - 1, H - 1))):
        m = oracle.decode(named[name], H, W)
        assert m.sum() == 1 and m[xy[1], xy[0]] == 1 and oracle.area_box(m) == (1, [xy[0], xy[1], xy[0], xy[1]]), name
    m = oracle.decode(named["column-cross"], H, W)  # a run over a column boundary: rows 0 and H - 1, two columns
    assert oracle.area_box(m) == (4, [1, 0, 2, H - 1]) and m[H - 2:, 1].all() and m[:2, 2].all()
    m = oracle.decode(named["long-run"], H, W)
    assert oracle.area_box(m) == (3 * H + 7, [1, 0, 4, H - 1])
    assert oracle.area_box(np.zeros((H, W))) == (0, [-1, -1, -1, -1])
    # the index over a flat store with one bad offset pair and one bad size
    lists = [named["blob"], [5, 9, H * W - 13], named["full"], named["empty"]]
    flat = np.concatenate([np.asarray(c, dtype=np.uint32) for c in lists])
    n = [len(c) for c in lists]
    offsets = np.concatenate(([0], np.cumsum(n)))
    sizes = [[H, W]] * 4
    ends, area, box, valid = oracle.index(flat, offsets, sizes)
    assert valid.tolist() == [0, -1, 0, 0] and area.tolist() == [int(oracle.decode(lists[0], H, W).sum()), 0, H * W, 0]
    assert box[2].tolist() == [0, 0, W - 1, H - 1] and box[1].tolist() == [-1] * 4 == box[3].tolist()
    assert ends[offsets[1]:offsets[2]].tolist() == [5, 14, H * W + 1] and ends[-1] == H * W
    bad = offsets.copy()
    bad[3] = len(flat) + 1
    _, _, _, v2 = oracle.index(flat, bad, [[H, W], [H, W], [0, W], [H, W]])
    assert v2.tolist() == [0, -1, -1, -1]
    # windows: decode then encode of the same window is the frame with everything outside the window cleared
    full = oracle.decode(named["blob"], H, W)
    for name, origin, hw in cases.windows(H, W):
        win = oracle.window_of(full, origin, hw)
        back = oracle.frame_of(win, origin, (H, W))
        inside = oracle.frame_of(np.ones(hw, np.uint8), origin, (H, W))
        assert np.array_equal(back, full * inside), name
        out, n_runs, info = oracle.encode_rows([win * 9], [[H, W]], [origin], 64)
        assert info[0] == 0 and np.array_equal(oracle.decode(out[0, :n_runs[0]], H, W), back) and not out[0, n_runs[0]:].any(), name
    out, n_runs, info = oracle.encode_rows([full], None, None, 3)
    assert info[0] == -2 and n_runs[0] == len(named["blob"]) > 3 and not out.any()


# ---- the library


def test_build_group_header_exports_and_source_hash():
    import __graft_entry__ as entry
    from lc_amd import build, rle

    T = build.RLE  # (its place among the libraries, its files and includes: tests/test_libraries_host.py)
    entry.build()
    lib = rle.load()
    assert not build.is_stale(T)
    assert lib.lc_amd_rle_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert build.sources(T) == [os.path.join(build.CSRC, "rle", "lc_rle.hip")]

    header = open(os.path.join(ROOT, "include", "lc_amd_rle.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(rle._SIGNATURES) and {"lc_rle_index_u32", "lc_rle_decode_u8", "lc_rle_encode_u8"} <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_rle_version() == int(re.search(r"#define LC_AMD_RLE_VERSION (\d+)", header).group(1)) == 1
    for name, have in (("MAX_SIZE", rle.MAX_SIZE), ("MAX_ORIGIN", rle.MAX_ORIGIN), ("MAX_COUNTS", rle.MAX_COUNTS)):
        assert have == int(re.search(rf"#define LC_RLE_{name} (\d+)", header).group(1)), name
    from lc_amd import gtinfo, maskcrop

    assert rle.MAX_ORIGIN == maskcrop.MAX_ORIGIN == gtinfo.MAX_ORIGIN == oracle.MAX_ORIGIN and rle.MAX_SIZE == maskcrop.MAX_SIZE == oracle.MAX_SIZE
    # every prototype's argument list against the ctypes signature: pointers, 32-bit and 64-bit whole numbers in the same places
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "8"}
    for name in ("lc_rle_index_u32", "lc_rle_decode_u8", "lc_rle_encode_u8"):
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "int64_t": "8"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = rle._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)


LDS_STATED = {"lc_rle_index_kernel": 144, "lc_rle_decode_kernel": 4, "lc_rle_encode_kernel": 256}


def test_three_kernels_without_scratch_within_the_stated_lds(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import build, rle

    rle.load()
    res = kernel_resources(build.RLE.so_path)
    assert len(res) == 3, sorted(res)
    header = open(os.path.join(ROOT, "include", "lc_amd_rle.h")).read()
    for short, lds in LDS_STATED.items():
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d.get('group_segment_fixed_size', 0)} B of LDS, {d['vgpr_count']} VGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d.get("group_segment_fixed_size", 0) <= lds, short
        assert f"{lds} bytes of LDS" in header, short  # the bound is the one the header states


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import rle

    lib = rle.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_rle_last_error

    def index(counts=p, offsets=p, sizes=p, T=8, F=2, ends=p, area=p, box=p, valid=p):
        return lib.lc_rle_index_u32(counts, offsets, sizes, T, F, ends, area, box, valid, None)

    assert index(F=-1) != 0 and b"lc_rle_index_u32: F < 0" in msg()
    assert index(F=0) == 0 and index(F=0, counts=None, offsets=None, sizes=None, ends=None, area=None, box=None, valid=None) == 0  # an empty store is a no-op
    assert index(T=-1) != 0 and b"T must be in [0, 4294967296]" in msg() and index(T=2 ** 32 + 1) != 0 and b"got 4294967297" in msg()
    for name in ("counts", "offsets", "sizes", "ends", "area", "box", "valid"):
        assert index(**{name: None}) != 0 and b"NULL" in msg(), name
    for name in ("counts", "sizes", "ends", "area", "box", "valid"):
        assert index(**{name: p + 2}) != 0 and b"aligned" in msg(), name
    assert index(offsets=p + 4) != 0 and b"aligned" in msg()

    def decode(ends=p, offsets=p, sizes=p, valid=p, T=8, F=2, idx=p, org=p, B=2, Hm=8, Wm=8, out=p, info=p):
        return lib.lc_rle_decode_u8(ends, offsets, sizes, valid, T, F, idx, org, B, Hm, Wm, out, info, None)

    assert decode(B=-1) != 0 and b"lc_rle_decode_u8: B < 0" in msg()
    assert decode(B=0) == 0 and decode(B=0, ends=None, offsets=None, sizes=None, valid=None, out=None) == 0  # an empty batch is a no-op
    assert decode(F=-1) != 0 and b"F < 0" in msg()
    assert decode(T=-1) != 0 and b"T must be" in msg() and decode(T=2 ** 32 + 1) != 0
    assert decode(Hm=0) != 0 and b"[1, 16384], got 0 x 8" in msg() and decode(Wm=16385) != 0 and b"got 8 x 16385" in msg()
    for name in ("ends", "offsets", "sizes", "valid", "out"):
        assert decode(**{name: None}) != 0 and b"NULL" in msg(), name
    for name in ("ends", "sizes", "valid", "idx", "org", "info"):
        assert decode(**{name: p + 2}) != 0 and b"aligned" in msg(), name
    assert decode(offsets=p + 4) != 0 and b"aligned" in msg()
    assert decode(B=2 ** 31 - 1, Hm=16384, Wm=16384) != 0 and b"too many" in msg()

    def encode(masks=p, F=2, Hm=8, Wm=8, sizes=p, org=p, cap=4, counts=p, n=p, info=p):
        return lib.lc_rle_encode_u8(masks, F, Hm, Wm, sizes, org, cap, counts, n, info, None)

    assert encode(F=-1) != 0 and b"lc_rle_encode_u8: F < 0" in msg()
    assert encode(F=0) == 0 and encode(F=0, masks=None, counts=None, n=None) == 0
    assert encode(Hm=0) != 0 and b"[1, 16384]" in msg() and encode(Wm=16385) != 0
    assert encode(cap=0) != 0 and b"cap must be at least 1, got 0" in msg()
    for name in ("masks", "counts", "n"):
        assert encode(**{name: None}) != 0 and b"NULL" in msg(), name
    for name in ("sizes", "org", "counts", "n", "info"):
        assert encode(**{name: p + 2}) != 0 and b"aligned" in msg(), name


def test_wrapper_refusals():
    from lc_amd import rle

    H, W = 6, 5
    with pytest.raises(TypeError, match="a list of arrays, one per mask"):
        rle.RleStore.from_counts(np.zeros((2, 3), np.uint32), (H, W))
    with pytest.raises(TypeError, match="the counts of mask 1 must be a list of whole numbers"):
        rle.RleStore.from_counts([[30], [29.0, 1.0]], (H, W))
    with pytest.raises(ValueError, match=r"the counts of mask 0 must lie in \[0, 2\^32\)"):
        rle.RleStore.from_counts([[31, -1]], (H, W))
    with pytest.raises(ValueError, match=r"must lie in \[0, 2\^32\)"):
        rle.RleStore.from_counts([[2 ** 32]], (H, W))
    with pytest.raises(ValueError, match=r"sizes has shape \(3, 2\), expected \(2,\) or \(2, 2\)"):
        rle.RleStore.from_counts([[30], [30]], np.ones((3, 2), np.int64))
    with pytest.raises(ValueError, match="frame sizes of 1 to 16384, got 0 to 5"):
        rle.RleStore.from_counts([[30]], (0, 5))
    with pytest.raises(TypeError, match="sizes must hold whole numbers"):
        rle.RleStore.from_counts([[30]], (6.0, 5.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order, but for the device
        rle.RleStore.from_counts([[30], [0, 30]], (H, W), device="cpu")
    with pytest.raises(TypeError, match="from_coco takes a list of records"):
        rle.RleStore.from_coco({"size": [H, W], "counts": b"n0"})
    with pytest.raises(ValueError, match="record 1 must be a dict with 'size' and 'counts'"):
        rle.RleStore.from_coco([{"size": [H, W], "counts": [30]}, {"size": [H, W]}])
    with pytest.raises(ValueError, match="ends inside a count"):
        rle.RleStore.from_coco([{"size": [H, W], "counts": "P"}])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rle.RleStore.from_coco([{"size": [H, W], "counts": "n0"}, {"size": [H, W], "counts": [0, 30]}], device="cpu")
    with pytest.raises(TypeError, match="counts must be int32"):
        rle.RleStore(torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.ones(1, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match="offsets must be int64"):
        rle.RleStore(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.ones(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"sizes has shape \(2, 2\), expected \(1, 2\)"):
        rle.RleStore(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.ones(2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="offsets holds F \\+ 1 entries"):
        rle.RleStore(torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), torch.ones(0, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rle.RleStore(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.ones(1, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match="decode takes an RleStore"):
        rle.decode([[30]])

    e = rle.encode
    m = torch.zeros(2, H, W, dtype=torch.uint8)
    with pytest.raises(TypeError, match="masks must be a torch.Tensor"):
        e(np.zeros((2, H, W), np.uint8))
    with pytest.raises(TypeError, match="masks must be uint8 or bool"):
        e(m.float())
    with pytest.raises(ValueError, match=r"masks has shape \(6, 5\)"):
        e(m[0])
    with pytest.raises(ValueError, match="mask sizes of 1 to 16384, got 0 x 5"):
        e(torch.zeros(2, 0, W, dtype=torch.uint8))
    with pytest.raises(ValueError, match="cap of 1 to"):
        e(m, cap=0)
    with pytest.raises(TypeError, match="cap must be a whole number"):
        e(m, cap=4.0)
    with pytest.raises(ValueError, match="sizes is a pair"):
        e(m, sizes=(1, 2, 3))
    with pytest.raises(ValueError, match="sizes of 1 to 16384, got 16385"):
        e(m, sizes=(16385, 4))
    with pytest.raises(TypeError, match="sizes must be int32"):
        e(m, sizes=torch.ones(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"sizes has shape \(3, 2\)"):
        e(m, sizes=torch.ones(3, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match="origin_xy must be int32 or int64"):
        e(m, origin_xy=torch.zeros(2, 2))
    with pytest.raises(ValueError, match=r"origin_xy has shape \(2, 3\)"):
        e(m, origin_xy=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="out is the triple"):
        e(m, out=(m, m))
    with pytest.raises(ValueError, match=r"out\[0\] has shape \(2, 8\), expected \(2, 4\)"):
        e(m, cap=4, out=(torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e(m, sizes=(H + 3, W + 3), origin_xy=torch.zeros(2, 2, dtype=torch.int64), cap=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rle.RleStore.from_masks(m)


@pytest.mark.parametrize("HW", cases.WIDE_FRAMES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_wide_frames_notice_an_encoder_that_forgets_the_chunk_before(HW):
    """The encoder takes 1024 frame columns at a time.  On the wide frames every mask but the empty one has a list that an encoder which
    restarts its boundary count and its last boundary with each chunk gets wrong, and the masks and windows put a boundary, none at all,
    and the closing column alone into a later chunk."""
    H, W = HW
    assert max(w for _, w in cases.FRAMES) < cases.ENC_CHUNK < W  # the old frames: one chunk, always
    masks = dict(cases.wide_masks(H, W))
    assert list(masks)[:6] == ["empty", "full", "blob", "checkerboard", "edge-run", "last-of-1023"] and ("empty-middle" in masks) == (W > 2048)
    for name, m in masks.items():
        assert m.shape == (H, W) and m.dtype == np.uint8
        good = oracle.encode(m).tolist()
        assert cases.encode_restarting(m, chunk=W + 1) == good  # one chunk: the restatement is the oracle
        assert (cases.encode_restarting(m) != good) == (name != "empty"), name
        assert np.array_equal(oracle.decode(good, H, W), m)
    b = cases.boundaries(masks["edge-run"]) // H
    assert b.tolist() == [1023, 1024] and oracle.encode(masks["edge-run"]).tolist() == [1024 * H - 1, 2, H * W - 1024 * H - 1]
    b = cases.boundaries(masks["last-of-1023"]) // H
    assert b.max() == 1024 and masks["last-of-1023"][H - 1, 1023] and not masks["last-of-1023"][:, 1024:].any()
    if W > 2048:
        b = cases.boundaries(masks["empty-middle"]) // H
        assert ((b < 1024) | (b >= 2048)).all() and (b < 1024).any() and (b >= 2048).sum() >= 2 and masks["empty-middle"][:, 1024:2048].all()
    # the windows: columns walked, chunks, and where the closing column falls
    wins = {name: (org, hw) for name, org, hw in cases.wide_windows(H, W)}
    assert cases.walked_columns(*wins["frame"], HW) == (0, W)
    assert cases.walked_columns(*wins["closing-alone"], HW) == (0, 1025)  # column 1024 is the only one of chunk two
    assert cases.walked_columns(*wins["from-6"], HW) == (6, W - 6) and cases.walked_columns(*wins["over-right-bottom"], HW) == (9, W - 9)
    for wname, (org, hw) in wins.items():
        xa, ncols = cases.walked_columns(org, hw, HW)
        differ = []
        for name, m in masks.items():
            frame = oracle.frame_of(oracle.window_of(m, org, hw), org, HW)
            good = oracle.encode(frame).tolist()
            assert cases.encode_restarting(frame, xa, ncols, chunk=W + 1) == good
            if cases.encode_restarting(frame, xa, ncols) != good:
                differ.append(name)
        assert (len(differ) > 0) == (ncols > cases.ENC_CHUNK), (wname, differ)
        if wname == "closing-alone":  # the masks with a set pixel at the foot of column 1023 are closed by the lone column
            assert {"full", "edge-run", "last-of-1023"} <= set(differ)


def test_chunked_index_lists_notice_a_32_bit_sum_and_a_dropped_carry():
    H, W = 64, 64
    assert all(len(c) <= 4 for _, c in cases.invalid_lists(H, W))  # the old invalid lists: one chunk of 256 counts, always
    (n1, good, v1), (n2, over, v2) = cases.chunked_index_lists(H, W)
    assert (n1, v1, n2, v2) == ("carried-sum", True, "carried-overflow", False)
    assert oracle.is_valid(good, H, W) and not oracle.is_valid(over, H, W)
    assert len(good) > 2 * cases.IDX_CHUNK and len(over) > 2 * cases.IDX_CHUNK
    assert cases.valid_with(over, H, W, "sum_32_bits") and cases.valid_with(good, H, W, "sum_32_bits")  # 32 bits take the overflow for valid
    assert not cases.valid_with(good, H, W, "no_carry") and not cases.valid_with(over, H, W, "no_carry")  # without carries the good list fails
    assert sum(over[:600]) < 2 ** 32 <= sum(over[:601]) and 600 // cases.IDX_CHUNK == 2  # the sum passes 2^32 in the third chunk
    flat = np.asarray(good + over, dtype=np.uint32)
    ends, area, box, valid = oracle.index(flat, [0, len(good), len(good) + len(over)], [(H, W), (H, W)])
    assert valid.tolist() == [0, -1] and area[0] == sum(good[1::2]) and area[1] == 0 and box[1].tolist() == [-1] * 4
    assert ends[len(good) - 1] == H * W and ends[-1] == H * W  # the low 32 bits of both sums
