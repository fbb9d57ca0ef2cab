"""Builds the native libraries with hipcc for gfx950 (cross-compiles without a GPU), each from the .hip files of one directory:

    name     library                         sources                  C ABI
    main     lc_amd/_C/liblc_amd.so          lc_amd/csrc/*.hip        include/lc_amd.h          the hot path
    optim    lc_amd/_C/liblc_amd_optim.so    lc_amd/csrc/optim/       include/lc_amd_optim.h    the fused optimizer step
    posecov  lc_amd/_C/liblc_amd_posecov.so  lc_amd/csrc/posecov/     include/lc_amd_posecov.h  the test-time pose covariance
    render   lc_amd/_C/liblc_amd_render.so   lc_amd/csrc/render/      include/lc_amd_render.h   the depth rasteriser
    crop     lc_amd/_C/liblc_amd_crop.so     lc_amd/csrc/crop/        include/lc_amd_crop.h     the zoom-in crops
    models   lc_amd/_C/liblc_amd_models.so   lc_amd/csrc/models/      include/lc_amd_models.h   model preparation (an offline tool's kernels)
    symerr   lc_amd/_C/liblc_amd_symerr.so   lc_amd/csrc/symerr/      include/lc_amd_symerr.h   symmetry-aware pose errors (evaluation)
    vsd      lc_amd/_C/liblc_amd_vsd.so      lc_amd/csrc/vsd/         include/lc_amd_vsd.h      BOP's VSD from rendered and scene depth (evaluation)
    gtinfo   lc_amd/_C/liblc_amd_gtinfo.so   lc_amd/csrc/gtinfo/      include/lc_amd_gtinfo.h   BOP's ground-truth visibility annotations (an offline tool's kernels)
    maskcrop lc_amd/_C/liblc_amd_maskcrop.so lc_amd/csrc/maskcrop/    include/lc_amd_maskcrop.h the training mask crops: warps, valid count, check points
    augment  lc_amd/_C/liblc_amd_augment.so  lc_amd/csrc/augment/     include/lc_amd_augment.h  the training crops' background switch and colour augmentation
    rle      lc_amd/_C/liblc_amd_rle.so      lc_amd/csrc/rle/         include/lc_amd_rle.h      the store of COCO run-length masks: index, decode, encode
    geometry lc_amd/_C/liblc_amd_geometry.so lc_amd/csrc/geometry/    include/lc_amd_geometry.h the training crops' geometry drawn from the seed word
    bgstore  lc_amd/_C/liblc_amd_bgstore.so  lc_amd/csrc/bgstore/     include/lc_amd_bgstore.h  the resident background store: each row's pick, cut and blend
    shade    lc_amd/_C/liblc_amd_shade.so    lc_amd/csrc/shade/       include/lc_amd_shade.h    the shading pass behind the rasteriser: uint8 frames of posed, vertex-coloured meshes
    obox     lc_amd/_C/liblc_amd_obox.so     lc_amd/csrc/obox/        include/lc_amd_obox.h     the oriented model box behind models_xform.json (an offline tool's kernels)
    symfind  lc_amd/_C/liblc_amd_symfind.so  lc_amd/csrc/symfind/     include/lc_amd_symfind.h  the symmetry deviation of a model: BOP's geometric rule, checked and searched (an offline tool's kernels)
    texture  lc_amd/_C/liblc_amd_texture.so  lc_amd/csrc/texture/     include/lc_amd_texture.h  the textured shading pass: per-corner texture coordinates, a resident store of mip-mapped textures
    sampler  lc_amd/_C/liblc_amd_sampler.so  lc_amd/csrc/sampler/     include/lc_amd_sampler.h  the resident training set: a step's rows drawn from the seed word, the retry on valid_cnt, the gather
    posedraw lc_amd/_C/liblc_amd_posedraw.so lc_amd/csrc/posedraw/    include/lc_amd_posedraw.h the synthetic scenes' object poses drawn from the seed word: uniform rotations, sphere-separated positions

A library's source hash covers its directory, its header and the headers of lc_amd/csrc/shared/ it declares (`Target.shared`): code that
two libraries need exists once there (lc_shared.h: main, posecov, models, symerr; lc_warp_grid.h: crop, maskcrop; lc_ray_length.h: vsd,
gtinfo; lc_wave_int.h: vsd, gtinfo, maskcrop; lc_keyed_hash.h: maskcrop, augment, geometry; lc_byte_finish.h: crop, augment), and no side
library restates another's arithmetic -- but for the wave scans that rle writes out for itself.  `TARGETS` is every library in build
order: whoever builds, packages, hashes or compares "all of them" iterates it, and tests/test_libraries_host.py states it row by row
(each library's files, marker, shared headers and includes, and each shared header's users).  `LATER_TARGETS` holds the libraries added
since that statement was written (bgstore, which includes lc_keyed_hash.h and lc_warp_grid.h and restates crop's tap combination and
augment's blend, pinned by tests/test_gpu_bgstore.py): "all of them" is `TARGETS + LATER_TARGETS`, in that order, and `build_later`
builds the second tuple as `build` builds a member of the first.  `EXTRA_TARGETS` is where every library after that goes (shade, which
includes no shared header and restates the rasteriser's snapped projection, pinned by tests/test_gpu_shade.py; obox, which includes no
shared header either and whose fp32 rule is the one of models, pinned by tests/test_gpu_obox.py; symfind, which includes none either and
restates models' d2, pinned by tests/test_gpu_symfind.py; texture, which includes none either and restates shade's pixel around a sampled
albedo, pinned by tests/test_gpu_texshade.py; sampler, which includes lc_keyed_hash.h and lc_wave_int.h and restates nothing, pinned by
tests/test_gpu_sampler.py; posedraw, which includes lc_keyed_hash.h and restates geometry's cosine and sine polynomial, pinned by
tests/test_gpu_posedraw.py): "all of them" is
`TARGETS + LATER_TARGETS + EXTRA_TARGETS`, `build_later` builds the third tuple behind the second, and the next library joins the third
tuple.  Every function takes the library it works on as a `Target`
(default: the hot-path library)."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
from typing import NamedTuple

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
OUT_DIR = os.path.join(PKG, "_C")
SO_PATH = os.path.join(OUT_DIR, "liblc_amd.so")
ARCH = "gfx950"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


class Target(NamedTuple):
    """One library: its short name, the directory of its sources (non-recursive globs), its public header, where it goes, the marker
    in front of the source hash it carries (compiled in as the macro named by the marker without its colon), and the headers it
    includes from lc_amd/csrc/shared/ (hashed along with its own directory)."""
    name: str
    src_dir: str
    header: str
    so_path: str
    hash_marker: bytes
    shared: tuple = ()


SHARED = os.path.join(CSRC, "shared")
SHARED_H = os.path.join(SHARED, "lc_shared.h")  # the fp64 cross-lane layer: the order-defining reductions of MAIN and POSECOV
WARP_GRID_H = os.path.join(SHARED, "lc_warp_grid.h")  # the fixed-point warp coordinates and launch geometry of CROP and MASKCROP
RAY_LENGTH_H = os.path.join(SHARED, "lc_ray_length.h")  # the ray length through a pixel and the phase-aligned group loads of VSD and GTINFO
WAVE_INT_H = os.path.join(SHARED, "lc_wave_int.h")  # the integer wave butterflies of VSD, GTINFO, MASKCROP and SAMPLER
KEYED_HASH_H = os.path.join(SHARED, "lc_keyed_hash.h")  # the keyed integer hash of the device's random numbers of MASKCROP, AUGMENT, GEOMETRY, BGSTORE, SAMPLER and POSEDRAW
BYTE_FINISH_H = os.path.join(SHARED, "lc_byte_finish.h")  # the finished output value of an image byte of CROP and AUGMENT


def _side(name: str, shared: tuple = ()) -> Target:
    """A side library, everything following from its name: csrc/<name>, include/lc_amd_<name>.h, _C/liblc_amd_<name>.so."""
    return Target(name, os.path.join(CSRC, name), f"lc_amd_{name}.h", os.path.join(OUT_DIR, f"liblc_amd_{name}.so"),
                  f"LC_AMD_{name.upper()}_SRC_HASH:".encode(), shared)


MAIN = Target("main", CSRC, "lc_amd.h", SO_PATH, b"LC_AMD_SRC_HASH:", (SHARED_H,))  # the hot path of training and test time; carries the hash of its own sources (lc_capi.hip: lc_amd_source_hash)
OPTIM = _side("optim")  # the fused optimizer step (lc_amd.optim)
POSECOV = _side("posecov", (SHARED_H,))  # the test-time pose covariance (lc_amd.posecov)
RENDER = _side("render")  # the depth rasteriser (lc_amd.render)
CROP = _side("crop", (BYTE_FINISH_H, WARP_GRID_H))  # the zoom-in crops (lc_amd.crops)
MODELS = _side("models", (SHARED_H,))  # the offline model preparation (lc_amd.models, python -m lc_amd.prep_models); loaded by no training or test-time path
# the symmetry-aware evaluation errors (lc_amd.metrics.compute_sym_pose_errors): its table rules are those of the label kernels, stated once in lc_sym_args.h
SYMERR = _side("symerr", (SHARED_H, os.path.join(CSRC, "lc_sym_args.h")))
VSD = _side("vsd", (RAY_LENGTH_H, WAVE_INT_H))  # the evaluation error that reads the scene's measured depth (lc_amd.vsd)
# the dataset annotations: visibility records, composed scene depth (lc_amd.gtinfo, python -m lc_amd.gen_gt_info); shares the ray length with VSD
GTINFO = _side("gtinfo", (RAY_LENGTH_H, WAVE_INT_H))
# the training loader's per-instance mask crops (lc_amd.maskcrop); shares the coordinates with CROP
MASKCROP = _side("maskcrop", (KEYED_HASH_H, WARP_GRID_H, WAVE_INT_H))
# the training loader's background switch and colour augmentation (lc_amd.augment); finishes a byte as CROP does, hashes as MASKCROP does
AUGMENT = _side("augment", (BYTE_FINISH_H, KEYED_HASH_H))
RLE = _side("rle")  # the training loader's device-resident store of run-length masks (lc_amd.rle); includes no shared header
GEOMETRY = _side("geometry", (KEYED_HASH_H,))  # the training loader's geometry drawn on the device from the seed word (lc_amd.geometry)
# every library, in build order
TARGETS = (MAIN, OPTIM, POSECOV, RENDER, CROP, MODELS, SYMERR, VSD, GTINFO, MASKCROP, AUGMENT, RLE, GEOMETRY)
# the training loader's resident background store (lc_amd.backgrounds); takes its coordinates from CROP's header and its hash from MASKCROP's
BGSTORE = _side("bgstore", (KEYED_HASH_H, WARP_GRID_H))
# the libraries that came after the registry test's rows, in build order behind TARGETS (folding the two tuples: DESIGN.md, section 7)
LATER_TARGETS = (BGSTORE,)
SHADE = _side("shade")  # the shading pass behind the rasteriser (lc_amd.shade); includes no shared header
# every library added since, in build order behind LATER_TARGETS: the tuple the next library joins
OBOX = _side("obox")  # the oriented model box search (lc_amd.obox, python -m lc_amd.prep_models --xform); includes no shared header
# the symmetry deviation of a model (lc_amd.symfind, python -m lc_amd.prep_models --check-symmetries / --symmetries); includes no shared header
SYMFIND = _side("symfind")
# the textured shading pass (lc_amd.texture); includes no shared header.  Not "texshade": tests/test_shade_host.py lets no other library's file carry "shade" in its name
TEXTURE = _side("texture")
# the training loader's resident annotations (lc_amd.sampler, lc_amd.trainset): hashes as MASKCROP does, sums a wavefront as VSD does
SAMPLER = _side("sampler", (KEYED_HASH_H, WAVE_INT_H))
# the synthetic scenes' object poses drawn on the device from the seed word (lc_amd.posedraw, lc_amd.synthscene); hashes as MASKCROP does
POSEDRAW = _side("posedraw", (KEYED_HASH_H,))
EXTRA_TARGETS = (SHADE, OBOX, SYMFIND, TEXTURE, SAMPLER, POSEDRAW)
HASH_MARKER = MAIN.hash_marker


def sources(target: Target = MAIN):
    return sorted(glob.glob(os.path.join(target.src_dir, "*.hip")))


def _deps(target: Target = MAIN):
    return sources(target) + sorted(glob.glob(os.path.join(target.src_dir, "*.h"))) + [os.path.join(os.path.dirname(PKG), "include", target.header)] + list(target.shared)


def source_hash(target: Target = MAIN) -> str:
    """sha256 over the names and contents of every source the library is built from (mtimes do not survive the copy onto a
    GPU box; contents do)."""
    import hashlib

    h = hashlib.sha256()
    for d in _deps(target):
        if os.path.exists(d):
            h.update(os.path.basename(d).encode())
            h.update(open(d, "rb").read())
    h.update(repr(sorted(PER_FILE_FLAGS.items())).encode())  # a change of the compiler flags is a change of the build
    h.update(repr(COMMON_FLAGS).encode())
    return h.hexdigest()


def embedded_hash(path: str = SO_PATH, marker: bytes = HASH_MARKER):
    """The source hash a built library was compiled from, read from its bytes (no dlopen: a stale library must not get loaded
    just to be asked), or None for a file without the marker."""
    try:
        blob = open(path, "rb").read()
    except OSError:
        return None
    i = blob.find(marker)
    if i < 0:
        return None
    j = i + len(marker)
    return blob[j:j + 64].decode("ascii", "replace")


def is_stale(target: Target = MAIN) -> bool:
    """True when the library is missing or was built from other source contents than the ones on disk now.  The hash lives INSIDE
    the library, so a copied library keeps it and there is no window in which library and hash disagree."""
    return embedded_hash(target.so_path, target.hash_marker) != source_hash(target)


def hipcc_available() -> bool:
    try:
        _hipcc()
        return True
    except RuntimeError:
        return False


def _locked(fn, target: Target = MAIN):
    import fcntl

    os.makedirs(OUT_DIR, exist_ok=True)
    with open(target.so_path + ".lock", "w") as lock:  # one builder at a time (pytest-xdist workers, torchrun ranks, A/B scripts)
        fcntl.flock(lock, fcntl.LOCK_EX)
        return fn()


def _build_one(force: bool, verbose: bool, target: Target) -> str:
    if not force and not is_stale(target):
        return target.so_path
    return _locked(lambda: target.so_path if (not force and not is_stale(target)) else _compile(target.so_path, [], verbose, target), target)


def build(force: bool = False, verbose: bool = False, target: Target = MAIN) -> str:
    return _build_one(force, verbose, target)


def build_later(force: bool = False, verbose: bool = False) -> list:
    """Every library of `LATER_TARGETS` and then of `EXTRA_TARGETS`, in order, each as `build` builds one."""
    return [_build_one(force, verbose, t) for t in LATER_TARGETS + EXTRA_TARGETS]


# Extra compiler flags of single translation units.  The latency builds of the one-wave pose kernels are scheduled for the shortest
# dependent chains (a lone wave per SIMD has nobody to hide its latencies behind): -2.8 % on the metric's launch, same bits; every
# other kernel is faster (or equal) with the default strategy (lc_amd/csrc/lc_pnp_latency.hip has the measurements).
_LATENCY = ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-amdgpu-use-amdgpu-trackers=1"]  # (the register-pressure trackers: -1.3 % more on the fused launch)
_MAX_ILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
PER_FILE_FLAGS = {
    "lc_pnp_latency.hip": _LATENCY,
    "lc_fused_latency.hip": _LATENCY,
    # few-waves-per-unit latency chains as well: head forward -2.6 % (fp32) / -2.8 % (bf16), wide solve -1 %, the test-time pipeline
    # 81.1 -> 79.8 us (scripts/ubench: bench_head.py, pnp_wide_ab.py, graph_inference.py; outputs unchanged)
    "lc_head.hip": _MAX_ILP,
    "lc_pnp.hip": _MAX_ILP,
    "lc_pnp_init.hip": _MAX_ILP,
    "lc_select.hip": _MAX_ILP,
    "lc_dense.hip": _MAX_ILP,
    # NOT lc_loss.hip (the loss kernel alone: +4 %) and NOT lc_fused.hip (the large-grid pose unit: +1.4 %)
}
# -ffp-contract=on: a multiply and an add are fused where the SOURCE writes them in one expression, and nowhere else.  hipcc's default
# (fast) also fuses across statements, and decides that per inlined copy of a function: the LC loss's walk body exists in a one-tile
# and a many-tiles copy, and under `fast` the two contracted differently -- two slicings of the same sample then differed in the last
# bit of an fp32 gradient for about 4 outputs in 10^8 (scripts/ubench/forms_ulp.py).  With `on` every form, slicing and translation
# unit evaluates the same expressions the same way: "bit for bit" is a property of the build, not of the inputs tried.  Cost on the
# headline launch: within the run-to-run noise (13.13 vs 13.07 us).
COMMON_FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-ffp-contract=on"]


def _compile(out: str, flags, verbose: bool, target: Target = MAIN) -> str:
    """One object per .hip source (in parallel; per-file flags from PER_FILE_FLAGS), then one link."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor

    hipcc, digest = _hipcc(), source_hash(target)
    macro = target.hash_marker.decode().rstrip(":")
    tmp = out + f".tmp{os.getpid()}"
    with tempfile.TemporaryDirectory(prefix="lc_amd_build_") as objdir:
        def one(src):
            obj = os.path.join(objdir, os.path.basename(src) + ".o")
            cmd = [hipcc, *COMMON_FLAGS, f'-D{macro}="{digest}"', *flags, *PER_FILE_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            return obj

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            objs = list(pool.map(one, sources(target)))
        link = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-fvisibility=hidden", *objs, "-o", tmp]
        if verbose:
            print(" ".join(link))
        try:
            subprocess.check_call(link)
            os.replace(tmp, out)  # atomic: a reader sees the old library or the new one, each with its own hash inside
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
    return out


def _variant_dir() -> str:
    """Where experiment builds go: LC_AMD_BUILD_DIR if set; next to a source checkout (build/variants, git-ignored) when the package sits in
    one; a per-user cache otherwise (an installed package's parent directory is site-packages: nothing is written there)."""
    env = os.environ.get("LC_AMD_BUILD_DIR")
    if env:
        return env
    parent = os.path.dirname(PKG)
    if os.path.exists(os.path.join(parent, "include", "lc_amd.h")) and os.access(parent, os.W_OK):
        return os.path.join(parent, "build", "variants")
    return os.path.join(os.environ.get("XDG_CACHE_HOME", os.path.join(os.path.expanduser("~"), ".cache")), "lc_amd", "variants")


VARIANT_DIR = _variant_dir()  # diagnostics stay out of the package


def variant_path(name: str) -> str:
    return os.path.join(VARIANT_DIR, f"liblc_amd_{name}.so")


def build_variant(name: str, flags, verbose: bool = False) -> str:
    """An experiment build of the same sources with extra compiler flags (-D switches), OUTSIDE the package:
    build/variants/liblc_amd_<name>.so; select it with LC_AMD_LIB=<path>.  Used by the A/B scripts under scripts/ and by the tests
    that need a diagnostic build only."""
    os.makedirs(VARIANT_DIR, exist_ok=True)
    return _locked(lambda: _compile(variant_path(name), list(flags), verbose))


if __name__ == "__main__":
    for t in TARGETS:
        print(build(force=True, verbose=True, target=t))
    for path in build_later(force=True, verbose=True):
        print(path)
