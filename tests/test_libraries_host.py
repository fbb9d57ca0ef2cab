"""The registry of the native libraries (lc_amd/build.py: `TARGETS`), stated ONCE, without a GPU: one row per library, and what follows
from the rows -- the build order and what `__graft_entry__.build()` asks for, each library's files, marker and source hash, which files
a hash covers and which it must not, the quoted includes, and the users of every header of lc_amd/csrc/shared/.  A new library is one
more row; a library that includes one more shared header is one changed row.  What is a library's own business (header = exports = ctypes
table, constants, refusals, kernel resources) is in that library's test file."""
import glob
import os
import re
import shutil
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Row(NamedTuple):
    name: str
    src_dir: str      # under lc_amd/csrc ("" is that directory itself)
    header: str       # under include/
    so: str           # under lc_amd/_C
    marker: bytes
    shared: tuple     # the declared shared headers, under lc_amd/csrc, in the order of `Target.shared`
    includes: object  # the quoted #includes of its .hip files; None for main, whose many files reach lc_shared.h through lc_common.h


ROWS = (
    Row("main", "", "lc_amd.h", "liblc_amd.so", b"LC_AMD_SRC_HASH:", ("shared/lc_shared.h",), None),
    Row("optim", "optim", "lc_amd_optim.h", "liblc_amd_optim.so", b"LC_AMD_OPTIM_SRC_HASH:", (), {"../../../include/lc_amd_optim.h"}),
    Row("posecov", "posecov", "lc_amd_posecov.h", "liblc_amd_posecov.so", b"LC_AMD_POSECOV_SRC_HASH:", ("shared/lc_shared.h",),
        {"../../../include/lc_amd_posecov.h", "../shared/lc_shared.h"}),
    Row("render", "render", "lc_amd_render.h", "liblc_amd_render.so", b"LC_AMD_RENDER_SRC_HASH:", (), {"../../../include/lc_amd_render.h"}),
    Row("crop", "crop", "lc_amd_crop.h", "liblc_amd_crop.so", b"LC_AMD_CROP_SRC_HASH:", ("shared/lc_byte_finish.h", "shared/lc_warp_grid.h"),
        {"../../../include/lc_amd_crop.h", "../shared/lc_byte_finish.h", "../shared/lc_warp_grid.h"}),
    Row("models", "models", "lc_amd_models.h", "liblc_amd_models.so", b"LC_AMD_MODELS_SRC_HASH:", ("shared/lc_shared.h",),
        {"../../../include/lc_amd_models.h", "../shared/lc_shared.h"}),
    Row("symerr", "symerr", "lc_amd_symerr.h", "liblc_amd_symerr.so", b"LC_AMD_SYMERR_SRC_HASH:", ("shared/lc_shared.h", "lc_sym_args.h"),
        {"../../../include/lc_amd_symerr.h", "../lc_sym_args.h", "../shared/lc_shared.h", "lc_sym_metrics_args.h"}),
    Row("vsd", "vsd", "lc_amd_vsd.h", "liblc_amd_vsd.so", b"LC_AMD_VSD_SRC_HASH:", ("shared/lc_ray_length.h", "shared/lc_wave_int.h"),
        {"../../../include/lc_amd_vsd.h", "../shared/lc_ray_length.h", "../shared/lc_wave_int.h"}),
    Row("gtinfo", "gtinfo", "lc_amd_gtinfo.h", "liblc_amd_gtinfo.so", b"LC_AMD_GTINFO_SRC_HASH:", ("shared/lc_ray_length.h", "shared/lc_wave_int.h"),
        {"../../../include/lc_amd_gtinfo.h", "../shared/lc_ray_length.h", "../shared/lc_wave_int.h"}),
    Row("maskcrop", "maskcrop", "lc_amd_maskcrop.h", "liblc_amd_maskcrop.so", b"LC_AMD_MASKCROP_SRC_HASH:",
        ("shared/lc_keyed_hash.h", "shared/lc_warp_grid.h", "shared/lc_wave_int.h"),
        {"../../../include/lc_amd_maskcrop.h", "../shared/lc_keyed_hash.h", "../shared/lc_warp_grid.h", "../shared/lc_wave_int.h"}),
    Row("augment", "augment", "lc_amd_augment.h", "liblc_amd_augment.so", b"LC_AMD_AUGMENT_SRC_HASH:", ("shared/lc_byte_finish.h", "shared/lc_keyed_hash.h"),
        {"../../../include/lc_amd_augment.h", "../shared/lc_byte_finish.h", "../shared/lc_keyed_hash.h"}),
    Row("rle", "rle", "lc_amd_rle.h", "liblc_amd_rle.so", b"LC_AMD_RLE_SRC_HASH:", (), {"../../../include/lc_amd_rle.h"}),
    Row("geometry", "geometry", "lc_amd_geometry.h", "liblc_amd_geometry.so", b"LC_AMD_GEOMETRY_SRC_HASH:", ("shared/lc_keyed_hash.h",),
        {"../../../include/lc_amd_geometry.h", "../shared/lc_keyed_hash.h"}),
)
# the one file of one library's directory that another library hashes: the table rules symerr has in common with the label kernels
LENT = {("main", "symerr"): {"lc_sym_args.h"}}


def _csrc(rel):
    from lc_amd import build

    return os.path.normpath(os.path.join(build.CSRC, rel))


def _quoted(path):
    return re.findall(r'#include "([^"]+)"', open(path).read())


def _resolved(path):
    return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in _quoted(path)]


def _pairs():
    from lc_amd import build

    assert len(build.TARGETS) == len(ROWS)
    return list(zip(build.TARGETS, ROWS))


def _includes(target, header):
    """Does a file of the library's own directory include the header?"""
    from lc_amd import build

    return any(header in _resolved(f) for f in build.sources(target) + glob.glob(os.path.join(target.src_dir, "*.h")))


def test_the_targets_are_the_rows_in_build_order():
    from lc_amd import build

    names = [r.name for r in ROWS]
    assert [t.name for t in build.TARGETS] == names and len(set(names)) == len(names) == 13
    for t, r in _pairs():
        assert t.src_dir == _csrc(r.src_dir) and os.path.isdir(t.src_dir), r.name
        assert t.so_path == os.path.join(build.OUT_DIR, r.so) and build.OUT_DIR == os.path.join(ROOT, "lc_amd", "_C"), r.name
        assert t.header == r.header and os.path.exists(os.path.join(ROOT, "include", r.header)), r.name
        assert t.hash_marker == r.marker, r.name
        assert t.shared == tuple(_csrc(s) for s in r.shared) and all(os.path.exists(s) for s in t.shared), r.name
    for distinct in ([t.so_path for t in build.TARGETS], [t.hash_marker for t in build.TARGETS], [build.source_hash(t) for t in build.TARGETS]):
        assert len(set(distinct)) == 13, distinct
    doc = build.__doc__
    for r in ROWS:
        assert f"lc_amd/_C/{r.so} " in doc and "lc_amd/csrc/" + (r.src_dir + "/ " if r.src_dir else "*.hip ") in doc and f"include/{r.header} " in doc, r.name


def test_the_entry_point_builds_every_library_once_in_that_order(monkeypatch):
    import __graft_entry__ as entry
    from lc_amd import build

    asked, real = [], build.build
    monkeypatch.setattr(build, "build", lambda force=False, verbose=False, target=build.MAIN: (asked.append(target), real(force, verbose, target))[1])
    entry.build()
    assert tuple(asked) == build.TARGETS
    assert all(os.path.exists(t.so_path) and not build.is_stale(t) for t in build.TARGETS)


def test_a_hash_covers_the_library_s_own_files_and_exactly_the_shared_headers_it_declares():
    from lc_amd import build

    def own(t, d):
        return os.path.dirname(d) == t.src_dir or d == os.path.join(ROOT, "include", t.header)

    for t, r in _pairs():
        deps = [os.path.normpath(d) for d in build._deps(t)]
        assert all(os.path.exists(d) for d in deps), r.name
        assert {d for d in deps if not own(t, d)} == set(t.shared), r.name
        build.build(target=t)  # (nothing to do where the library is current)
        for other, ro in _pairs():
            if other is t:
                continue
            # no other library sees this one's directory or header, or carries its marker
            seen = {os.path.basename(d) for d in build._deps(other) if own(t, os.path.normpath(d))}
            assert seen == LENT.get((r.name, ro.name), set()), (r.name, ro.name)
            assert build.embedded_hash(t.so_path, other.hash_marker) is None, (r.name, ro.name)
        assert build.embedded_hash(t.so_path, t.hash_marker) == build.source_hash(t), r.name


def test_the_quoted_includes_are_the_rows():
    from lc_amd import build

    for t, r in _pairs():
        if r.includes is None:
            assert t is build.MAIN and build.SHARED_H in _resolved(os.path.join(build.CSRC, "lc_common.h"))
        else:
            assert {inc for src in build.sources(t) for inc in _quoted(src)} == r.includes, r.name


def test_a_shared_header_belongs_to_exactly_the_libraries_that_declare_it(tmp_path, monkeypatch):
    """For every header of lc_amd/csrc/shared/: the libraries that hash it, that declare it, that include it and whose row names it are
    the same; and one more byte in it, in a COPY of the sources, changes the source hashes of exactly those."""
    from lc_amd import build

    every = build.TARGETS
    headers = sorted(glob.glob(os.path.join(build.SHARED, "*")))
    named = {_csrc(s) for r in ROWS for s in r.shared if s.startswith("shared/")}
    assert set(headers) == named and len(headers) == 6
    assert {build.SHARED_H, build.WARP_GRID_H, build.RAY_LENGTH_H, build.WAVE_INT_H, build.KEYED_HASH_H, build.BYTE_FINISH_H} == named

    pkg = tmp_path / "lc_amd"
    shutil.copytree(build.CSRC, pkg / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    monkeypatch.setattr(build, "PKG", str(pkg))  # where _deps looks for include/

    def moved(path):
        return str(pkg / os.path.relpath(path, os.path.dirname(build.CSRC)))

    copies = [t._replace(src_dir=moved(t.src_dir), shared=tuple(moved(s) for s in t.shared)) for t in every]
    assert [build.source_hash(t) for t in copies] == [build.source_hash(t) for t in every]  # (names and contents: the copy hashes like the tree)
    for header in headers:
        users = [r.name for r in ROWS if os.path.relpath(header, build.CSRC) in r.shared]
        assert len(users) >= 2, header  # a header with one user belongs into that user's directory
        assert [t.name for t in every if header in build._deps(t)] == users, header
        assert [t.name for t in every if header in t.shared] == users, header
        assert [t.name for t in every if _includes(t, header)] == users, header
        before = [build.source_hash(t) for t in copies]
        with open(moved(header), "ab") as f:
            f.write(b"\n")
        after = [build.source_hash(t) for t in copies]
        assert [t.name for t, x, y in zip(copies, before, after) if x != y] == users, header
