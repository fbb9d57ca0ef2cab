"""The background-store library without a GPU (lc_amd/csrc/bgstore/, include/lc_amd_bgstore.h, lc_amd/backgrounds.py): its place beside
the registry's thirteen rows, header = exports = ctypes table, its source hash, what the compiler made of the two kernels, every refusal of
the two entry points reached with host pointers (nothing launches), the wrappers' refusals, the store's layout, the host contract the
pick rests on, and the oracle's planted mistakes on the case list."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIRTEEN = ["main", "optim", "posecov", "render", "crop", "models", "symerr", "vsd", "gtinfo", "maskcrop", "augment", "rle", "geometry"]


def test_the_library_stands_behind_the_thirteen_and_the_entry_point_builds_it():
    import __graft_entry__ as entry
    from lc_amd import backgrounds, build

    T = build.BGSTORE
    assert build.LATER_TARGETS == (T,) and [t.name for t in build.TARGETS] == THIRTEEN and T not in build.TARGETS
    assert T == build._side("bgstore", (build.KEYED_HASH_H, build.WARP_GRID_H))
    assert T.src_dir == os.path.join(build.CSRC, "bgstore") and T.header == "lc_amd_bgstore.h" and T.hash_marker == b"LC_AMD_BGSTORE_SRC_HASH:"
    assert T.so_path == os.path.join(ROOT, "lc_amd", "_C", "liblc_amd_bgstore.so")
    doc = build.__doc__
    assert "lc_amd/_C/liblc_amd_bgstore.so " in doc and "lc_amd/csrc/bgstore/ " in doc and "include/lc_amd_bgstore.h " in doc
    entry.build()
    assert os.path.exists(T.so_path) and not build.is_stale(T)
    lib = backgrounds.load()
    assert lib.lc_amd_bgstore_version() == 1
    assert lib.lc_amd_bgstore_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    every = build.TARGETS + build.LATER_TARGETS
    assert len({build.source_hash(t) for t in every}) == len({t.so_path for t in every}) == len({t.hash_marker for t in every}) == 14
    for other in build.TARGETS:  # no library of the thirteen sees this one's directory or header, or carries its marker, and the reverse
        assert not any("bgstore" in os.path.basename(d) or os.path.dirname(d) == T.src_dir for d in build._deps(other)), other.name
        assert build.embedded_hash(other.so_path, T.hash_marker) is None and build.embedded_hash(T.so_path, other.hash_marker) is None, other.name
    # the hash covers the library's own files and exactly the two shared headers it declares and includes
    deps = [os.path.normpath(d) for d in build._deps(T)]
    own = {os.path.join(T.src_dir, "lc_bgstore.hip"), os.path.join(ROOT, "include", T.header)}
    assert set(deps) - own == {build.KEYED_HASH_H, build.WARP_GRID_H} and own <= set(deps)
    source = open(build.sources(T)[0]).read()
    assert build.sources(T) == [os.path.join(T.src_dir, "lc_bgstore.hip")]
    assert set(re.findall(r'#include "([^"]+)"', source)) == {"../../../include/lc_amd_bgstore.h", "../shared/lc_keyed_hash.h", "../shared/lc_warp_grid.h"}
    assert set(re.findall(r"^\s*#\s*ifn?def\s+(\w+)", source, re.M)) == {"LC_AMD_BGSTORE_SRC_HASH"}  # no build switch
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomic" not in code
    # the two scripts that walk "all libraries" walk this one too
    assert "build.TARGETS + build.LATER_TARGETS" in open(os.path.join(ROOT, "scripts", "isa_identity.py")).read()


def test_header_exports_and_the_ctypes_table_agree():
    from lc_amd import augment, backgrounds, build, crops

    T = build.BGSTORE
    backgrounds.load()
    header = open(os.path.join(ROOT, "include", T.header)).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(backgrounds._SIGNATURES) and {"lc_bgstore_pick", "lc_bgstore_switch_u8"} <= declared and len(declared) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert int(re.search(r"#define LC_AMD_BGSTORE_VERSION (\d+)", header).group(1)) == 1
    assert backgrounds.MAX_SIZE == crops.MAX_SIZE == int(re.search(r"#define LC_BGSTORE_MAX_SIZE (\d+)", header).group(1))
    assert augment.OP_SWITCH == int(re.search(r"#define LC_BGSTORE_OP_SWITCH (\d+)", header).group(1))
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_double: "d"}
    for name in ("lc_bgstore_pick", "lc_bgstore_switch_u8"):
        m = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        kinds = ["p" if "*" in a else {"int": "i", "double": "d"}[a.split()[0]] for a in m.group(1).split(",")]
        res, args = backgrounds._SIGNATURES[name]
        assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], (name, kinds)


def test_two_kernels_without_scratch_or_spills(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import backgrounds, build

    backgrounds.load()
    res = kernel_resources(build.BGSTORE.so_path)
    assert len(res) == 2, sorted(res)
    for short, threads in (("lc_bgstore_pick_kernel", 64), ("lc_bgstore_switch_kernel", 256)):
        (d,) = [d for n, d in res.items() if short in n]
        with capsys.disabled():
            print(f"\n{short}: {d['vgpr_count']} VGPRs, {d['sgpr_count']} SGPRs, {d.get('group_segment_fixed_size', 0)} B of LDS", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (short, "scratch")
        assert d["max_flat_workgroup_size"] == threads, short
    assert [d for n, d in res.items() if "pick" in n][0].get("group_segment_fixed_size", 0) == 0


def test_entry_points_check_their_arguments_before_launching():
    from lc_amd import backgrounds

    lib = backgrounds.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    msg = lib.lc_amd_bgstore_last_error

    def pick(prob=0.5, G=3, seed=p, sid=p, hw=p, B=2, gate=p, which=p, bg_hw=p):
        return lib.lc_bgstore_pick(prob, G, seed, sid, hw, B, gate, which, bg_hw, None)

    assert pick(B=-1) != 0 and b"lc_bgstore_pick: B < 0" in msg()
    assert pick(B=0) == 0 and pick(B=0, seed=None, sid=None, hw=None, gate=None, which=None, bg_hw=None) == 0
    assert pick(G=-1) != 0 and b"G < 0" in msg()
    for name in ("seed", "sid", "hw", "gate", "which", "bg_hw"):
        assert pick(**{name: None}) != 0 and b"NULL" in msg(), name
    for bad in (-1e-9, 1.0000001, math.nan, math.inf):
        assert pick(prob=bad) != 0 and b"switch_bg_prob must lie in [0, 1]" in msg(), bad
    assert pick(seed=p + 4) != 0 and b"seed must be aligned to 8 bytes" in msg()
    for name in ("sid", "hw", "gate", "which", "bg_hw"):
        assert pick(**{name: p + 2}) != 0 and b"aligned to 4 bytes" in msg(), name

    def switch(crops=p, msk=p, pixels=p, offsets=p, hw=p, G=3, which=p, M=p, h=32, w=40, B=2, info=p):
        return lib.lc_bgstore_switch_u8(crops, msk, pixels, offsets, hw, G, which, M, h, w, B, info, None)

    assert switch(B=-1) != 0 and b"lc_bgstore_switch_u8: B < 0" in msg()
    assert switch(B=0) == 0 and switch(B=0, crops=None, msk=None, pixels=None, offsets=None, hw=None, which=None, M=None, info=None) == 0
    assert switch(G=-1) != 0 and b"G < 0" in msg()
    for name in ("crops", "msk", "pixels", "offsets", "hw", "which", "M", "info"):
        assert switch(**{name: None}) != 0 and b"NULL" in msg(), name
    for bad in ((0, 40), (32, 0), (16385, 40), (32, 16385), (-1, 40)):
        assert switch(h=bad[0], w=bad[1]) != 0 and b"h and w must be in [1, 16384], got" in msg(), bad
    assert switch(offsets=p + 4) != 0 and b"offsets must be aligned to 8 bytes" in msg()
    for name in ("msk", "hw", "which", "M", "info"):
        assert switch(**{name: p + 2}) != 0 and b"aligned to 4 bytes" in msg(), name


def test_wrapper_and_store_refusals():
    from lc_amd import backgrounds as bg
    from lc_amd.augment import AugmentConfig
    from lc_amd.train_inputs import train_inputs

    im = np.zeros((5, 7, 3), np.uint8)
    with pytest.raises(TypeError, match="images is a sequence"):
        bg.BackgroundStore.from_images(im, "cuda:0")
    with pytest.raises(ValueError, match="at least one image"):
        bg.BackgroundStore.from_images([], "cuda:0")
    with pytest.raises(TypeError, match="image 1 must be a uint8 array or tensor, got float32"):
        bg.BackgroundStore.from_images([im, im.astype(np.float32)], "cuda:0")
    with pytest.raises(ValueError, match=r"image 0 has shape \(5, 7\), expected \(Hb,Wb,3\)"):
        bg.BackgroundStore.from_images([im[:, :, 0]], "cuda:0")
    with pytest.raises(ValueError, match="image sizes of 1 to 16384, got 0 x 7 for image 1"):
        bg.BackgroundStore.from_images([torch.from_numpy(im), im[:0]], "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bg.BackgroundStore.from_images([im], "cpu")

    z = torch.zeros(0, dtype=torch.uint8)
    store = bg.BackgroundStore(z, torch.zeros(1, dtype=torch.int64), torch.ones(1, 2, dtype=torch.int32), [(1, 1)])  # a host stand-in: refusals only
    cfg, sid = AugmentConfig(), torch.zeros(3, dtype=torch.int32)
    crops, msk = torch.zeros(3, 3, 8, 12, dtype=torch.uint8), torch.ones(3, 8, 12)

    def switch(crops=crops, store=store, cfg=cfg, seed=1, sample_id=sid, msk_in=msk):
        return bg.switch_backgrounds(crops, store, cfg, seed=seed, sample_id=sample_id, msk_in=msk_in)

    with pytest.raises(TypeError, match="lc_amd.backgrounds: crops must be uint8"):
        switch(crops=crops.float())
    with pytest.raises(ValueError, match=r"crops has shape \(3, 1, 8, 12\)"):
        switch(crops=crops[:, :1])
    with pytest.raises(TypeError, match="store must be a BackgroundStore"):
        switch(store=crops)
    with pytest.raises(TypeError, match="cfg must be an AugmentConfig"):
        switch(cfg=None)
    with pytest.raises(ValueError, match=r"switch_bg_prob must lie in \[0, 1\], got 1.5"):
        switch(cfg=AugmentConfig(switch_bg_prob=1.5))
    with pytest.raises(TypeError, match="sample_id must be int32, got torch.int64"):
        switch(sample_id=sid.long())
    with pytest.raises(ValueError, match=r"sample_id has shape \(2,\), expected \(3,\)"):
        switch(sample_id=sid[:2])
    with pytest.raises(TypeError, match="msk_in must be a torch.Tensor"):
        switch(msk_in=None)
    with pytest.raises(ValueError, match=r"msk_in has shape \(3, 8, 11\)"):
        switch(msk_in=msk[:, :, :11])
    with pytest.raises(ValueError, match="seed of 0 to 18446744073709551615, got -1"):
        switch(seed=-1)
    with pytest.raises(TypeError, match="a seed tensor holds one uint64 or int64 element"):
        switch(seed=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="crops must be contiguous"):
        switch(crops=torch.zeros(3, 3, 12, 8, dtype=torch.uint8).transpose(2, 3))
    with pytest.raises(RuntimeError, match="lc_amd.backgrounds: crops is on cpu.*no CPU fallback"):
        switch()
    with pytest.raises(TypeError, match="sample_id must be int32"):
        bg.pick_backgrounds(store, cfg, seed=1, sample_id=sid.float())

    frames, masks = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint8)
    base = dict(masks=masks, bbox_xyxy=torch.zeros(3, 4), cam_K=torch.eye(3), sample_id=sid, cfg=cfg, seed=3, in_hw=(32, 32), out_hw=(16, 16))
    with pytest.raises(ValueError, match="at most one of the two"):
        train_inputs(frames, sid, backgrounds=torch.zeros(1, 3, 32, 32, dtype=torch.uint8), background_store=store, **base)
    with pytest.raises(TypeError, match="background_store must be a BackgroundStore"):
        train_inputs(frames, sid, background_store=[im], **base)


def test_the_layout_packs_rows_and_rounds_every_start_up_to_four():
    from lc_amd import backgrounds as bg
    from tests import bgstore_cases as cases

    assert bg.layout([(5, 7), (48, 64), (37, 101)]) == ([0, 108, 9324], 9324 + 3 * 37 * 101)  # 105 -> 108; 108 + 9216 is a multiple already
    assert bg.layout([(1, 1), (1, 1), (1, 3)]) == ([0, 4, 8], 17)
    assert bg.layout([(37, 101)]) == ([0], 11211)
    for sizes in cases.STORES.values():
        offsets, total = bg.layout(sizes)
        ends = [o + 3 * h * w for o, (h, w) in zip(offsets, sizes)]
        assert all(o % bg.ALIGN == 0 for o in offsets) and total == ends[-1]
        assert all(0 <= nxt - end < bg.ALIGN for end, nxt in zip(ends, offsets[1:]))


def test_the_case_list_switches_the_rows_it_says_and_draw_s_other_words_ignore_the_backgrounds():
    from lc_amd import augment
    from tests import bgstore_cases as cases
    from tests import bgstore_oracle as oracle

    cfg = augment.AugmentConfig()
    gate, which, bg_hw = oracle.pick(cfg, cases.SEED, cases.IDS, cases.STORES["three"])
    assert {int(b): int(which[b]) for b in np.flatnonzero(gate)} == cases.SWITCHED and int((gate == 0).sum()) == 5
    assert (which[gate == 0] == -1).all() and (bg_hw[gate == 0] == 1).all()
    assert all(tuple(bg_hw[b]) == cases.STORES["three"][g] for b, g in cases.SWITCHED.items())
    g1, w1, _ = oracle.pick(cfg, cases.SEED, cases.IDS, cases.STORES["one"])
    assert np.array_equal(g1, gate) and set(w1[g1 == 1]) == {0}
    # the colour chain's draws do not depend on the number of backgrounds: rows for G = 0 and G differ in bit 0 and P[1] alone
    for use in (dict(), dict(use_peper_salt=True, use_motion_blur=True, use_invert=True)):
        c = augment.AugmentConfig(**use)
        P0, lut0 = augment.draw(c, cases.SEED, cases.IDS, 0, (31, 40))
        for G in (1, 3):
            P, lut = augment.draw(c, cases.SEED, cases.IDS, G, (31, 40))
            assert np.array_equal(lut, lut0) and np.array_equal(P[:, 2:], P0[:, 2:]) and np.array_equal(P[:, 0] & ~1, P0[:, 0])
            assert not (P0[:, 0] & 1).any() and not P0[:, 1].any() and (P[:, 0] & 1).sum() == 7


def test_every_planted_mistake_changes_the_oracle_s_bytes():
    from lc_amd import augment
    from tests import bgstore_cases as cases
    from tests import bgstore_oracle as oracle

    cfg = augment.AugmentConfig()
    assert oracle.MISTAKES == ("hw_of_wrong_image", "row_stride_padded", "tie_half_up", "closed_rows_written")
    for mistake in oracle.MISTAKES:
        changed = []
        for store, hw in cases.CASES:
            ref = cases.reference(store, hw)
            got = oracle.switch(ref["crops"], ref["images"], cfg, cases.SEED, cases.IDS, ref["msk"], mistake=mistake)[0]
            changed.append(not np.array_equal(got, ref["out"]))
        if mistake == "hw_of_wrong_image":  # (a store of one image has no other size)
            assert changed == [store == "three" for store, _ in cases.CASES], (mistake, changed)
        else:
            assert all(changed), (mistake, changed)
    # and the reference itself: closed rows and k = 1024 pixels keep the sentinel, the rest of an open row changes somewhere
    for store, hw in cases.CASES:
        ref = cases.reference(store, hw)
        closed = ref["info"] == 0
        assert np.array_equal(ref["out"][closed], ref["crops"][closed])
        keep = np.broadcast_to((ref["msk"] >= 1.0)[:, None], ref["out"].shape)
        assert np.array_equal(ref["out"][keep], ref["crops"][keep])
        assert all(not np.array_equal(ref["out"][b], ref["crops"][b]) for b in np.flatnonzero(~closed))
