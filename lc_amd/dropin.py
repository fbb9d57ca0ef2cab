"""Drop-in installer: run the reference's own `train.py` / `test.py` on the HIP hot path without editing them.

    python -m lc_amd.dropin /path/to/lc/train.py --cfg configs/gsplmo.yaml ...

`install()` must run with the reference checkout on `sys.path`.  It swaps exactly the hot-path entry points
 and leaves everything else of the reference untouched:

    lib.cov_mixed.Loss_cov_mixed   -> lc_amd.cov_mixed.Loss_cov_mixed     (also the name `losses` imported, losses.py:15)
    lib.pnp.cer_solver / pnp_ceres -> lc_amd.pnp.cer_solver / pnp_ceres   (registered BEFORE the reference imports them, so the
                                                                          Ceres cffi extension `lib.pnp._ext` is never needed)
    ptnet.softargmax_2d_std        -> lc_amd.ptnet.softargmax_2d_std      (+ ptnet.ptnet.forward's sparse branch fused)
    lib.pnp.cv2_solver             -> lc_amd.pnp.gpu_solver               (only when OpenCV is absent, or on request)
    lib.utils.grad.NormClipper     -> lc_amd.grad.NormClipper             (same constructor and `max_norm` buffer; also the name in `losses`)
    losses.Loss_fn.sparse_kpt_loss / .dense_pose_loss -> the fused-launch methods of lc_amd.losses.Loss_fn (they only use the
                                                          attributes the reference's own Loss_fn instance has)

Opt-in (`install(native_labels=True)`, or `python -m lc_amd.dropin --native-labels train.py ...`): label preparation on the device --
    losses.annots_on_the_fly / selete_best_pose / xyz_from_homo_z, symmetry.select_pose_2d / select_pose_3d -> lc_amd.labels
(`train.py:58,116` look the names up on the module at call time).  Without it the reference's own label preparation runs.

Opt-in (`install(native_optim=True)`, or `--native-optim`, in either order with `--native-labels`): the fused optimizer step --
    lib.optim.ranger.Ranger (and the name `utils.Ranger`, utils.py:10, when the reference's utils is already imported) -> lc_amd.optim.Ranger
Without it the reference's own Ranger runs.

Opt-in (`install(native_depth=MODELS_DIR)`, or `--native-depth MODELS_DIR`; implies `--native-labels`): the depth maps of the labels --
    the models `obj_*.ply` of MODELS_DIR are uploaded once (lc_amd.gen_z.load_models) and `lc_amd.labels.set_depth_source` makes
    annots_on_the_fly render `homo_z_out` for every batch that comes without it; dataset.BOP_Dataset._get_homo_with_depth no longer opens
    `z_path` and _get_single_item leaves `homo_z_out` out of its blob, so a training run needs no `z_crop` directory.

Opt-in (`install(native_sym=MODELS_INFO_JSON)`, or `--native-sym MODELS_INFO_JSON`; implies `--native-labels`): the symmetric pose candidates --
    the per-object symmetry transforms of `models_info.json` are uploaded once (lc_amd.symmetry.SymmetrySet, 384 steps of a continuous
    symmetry as the reference) and `lc_amd.labels.set_symmetry_source` makes annots_on_the_fly form every row's candidates on the device from
    R_no_aug, t_no_aug and obj_id; `symmetry.symmetry_pose_candidates` as the reference's `dataset` module calls it (dataset.py:405) returns
    the single base pose [R | t][None], so the loader ships 12 floats per sample and `sym_collate` keeps the batch in order (one chunk).
    Objects with a continuous AND discrete symmetries are served too (the reference itself raises for them).

Opt-in (`install(native_crops=True)`, or `--native-crops`): the zoom-in crop of the test-time loader (the reference's `dataset` module must still import,
    which needs a cv2 module, imgaug and pycocotools: lc_amd.crops.test_item makes no OpenCV call, `import dataset` does) --
    dataset.BOP_Dataset._get_single_item of a dataset with `training == False` -> lc_amd.crops.test_item (the frame as uint8 and the
    crop's matrix instead of `rgb_in`); utils.xfer_to (and the name `test.xfer_to`, test.py:9, when that module is already imported)
    -> the same transfer followed by lc_amd.crops.finish_blob, which cuts `rgb_in` on the device.  Training datasets keep the
    reference's method.  The frames of one batch must share a size (default_collate stacks them).
"""
from __future__ import annotations

import importlib
import os
import runpy
import sys
import types


def install(patch_ptnet: bool = True, gpu_initialiser=None, native_labels: bool = False, native_optim: bool = False, native_depth=None,
            native_crops: bool = False, native_sym=None) -> dict:
    """gpu_initialiser: True = also register the RANSAC-P3P kernel as `lib.pnp.cv2_solver` (same `solve` surface,
    `test.py:59,120`); None (default) = only when OpenCV cannot be imported, so that `test.py` runs without it.
    native_labels: also rebind the reference's label-preparation names to lc_amd.labels (done["labels"]).
    native_optim: also rebind the reference's Ranger to lc_amd.optim.Ranger (done["optim"]).
    native_depth: a directory of BOP models (obj_*.ply, in mm): also native_labels, with the labels' depth rendered from them (done["depth"]).
    native_crops: also take the test-time loader's zoom-in crop onto the device (done["crops"]).
    native_sym: a BOP models_info.json: also native_labels, with the symmetric pose candidates formed on the device from it (done["sym"])."""
    from . import cov_mixed as cm
    from . import ptnet as head
    from .pnp import cer_solver, gpu_solver, pnp_ceres

    done = {}
    # PnP: register our modules under the reference's names first (lib/ and lib/pnp/ are namespace packages)
    sys.modules["lib.pnp.pnp_ceres"] = pnp_ceres
    sys.modules["lib.pnp.cer_solver"] = cer_solver
    if gpu_initialiser is None:
        try:
            importlib.import_module("cv2")
            gpu_initialiser = False
        except ImportError:
            gpu_initialiser = True
    if gpu_initialiser:
        sys.modules["lib.pnp.cv2_solver"] = gpu_solver
    try:
        pkg = importlib.import_module("lib.pnp")
        pkg.pnp_ceres, pkg.cer_solver = pnp_ceres, cer_solver
        if gpu_initialiser:
            pkg.cv2_solver = gpu_solver
        done["lib.pnp"] = True
    except ImportError:
        done["lib.pnp"] = False
    # loss: patch the defining module and every module that did `from lib.cov_mixed import Loss_cov_mixed`
    try:
        ref_cm = importlib.import_module("lib.cov_mixed")
        ref_cm.Loss_cov_mixed = cm.Loss_cov_mixed
        done["lib.cov_mixed"] = True
    except ImportError:
        done["lib.cov_mixed"] = False
    for name, mod in list(sys.modules.items()):
        if isinstance(mod, types.ModuleType) and name != "lib.cov_mixed" and getattr(mod, "Loss_cov_mixed", None) is not None \
                and mod is not cm:
            mod.Loss_cov_mixed = cm.Loss_cov_mixed
    try:
        ref_losses = importlib.import_module("losses")
        ref_losses.Loss_cov_mixed = cm.Loss_cov_mixed
        done["losses"] = True
    except Exception:  # the reference's losses.py needs scipy/floatbits etc.; absent pieces are the caller's problem
        done["losses"] = False
    # the launch-bound glue of the reference's own Loss_fn: clipper class and the two methods with fused counterparts
    try:
        from . import grad as our_grad
        from . import losses as our_losses

        ref_grad = importlib.import_module("lib.utils.grad")
        ref_grad.NormClipper = our_grad.NormClipper
        if done.get("losses"):
            ref_losses.NormClipper = our_grad.NormClipper
            ref_losses.Loss_fn.sparse_kpt_loss = our_losses.Loss_fn.sparse_kpt_loss
            ref_losses.Loss_fn.dense_pose_loss = our_losses.Loss_fn.dense_pose_loss
        done["loss_glue"] = bool(done.get("losses"))
    except Exception:
        done["loss_glue"] = False
    if patch_ptnet:
        try:
            ref_ptnet = importlib.import_module("ptnet")
            ref_ptnet.softargmax_2d_std = head.softargmax_2d_std
            orig_forward = ref_ptnet.ptnet.forward

            def forward(self, rgb):
                if "kpt_logits" not in self.channel_slices:
                    return orig_forward(self, rgb)
                out_raw, _ = self.net(rgb)  # ptnet.py:55
                return head.sparse_head(out_raw[:, self.channel_slices["kpt_logits"]])  # ptnet.py:59-66 fused

            ref_ptnet.ptnet.forward = forward
            done["ptnet"] = True
        except Exception:
            done["ptnet"] = False
    if native_labels or native_depth or native_sym:
        done["labels"] = _install_labels()
    if native_sym:
        done["sym"] = _install_sym(native_sym)
    if native_depth:
        done["depth"] = _install_depth(native_depth)
    if native_optim:
        done["optim"] = _install_optim()
    if native_crops:
        done["crops"] = _install_crops()
    return done


_LABEL_NAMES = {"losses": ("annots_on_the_fly", "selete_best_pose", "xyz_from_homo_z"), "symmetry": ("select_pose_2d", "select_pose_3d")}


def _install_labels() -> bool:
    from . import labels

    try:
        mods = {name: importlib.import_module(name) for name in _LABEL_NAMES}
    except Exception:  # the reference's modules need scipy etc.; absent pieces are the caller's problem
        return False
    for name, attrs in _LABEL_NAMES.items():
        for attr in attrs:
            setattr(mods[name], attr, getattr(labels, attr))
    return True


def _install_depth(models_dir) -> bool:
    """The models of `models_dir` on the current device as the labels' depth source (mm, like the poses of a BOP dataset; near and far
    as tools/gen_z.py:75-76), and the reference's loader taken off the stored depth: `BOP_Dataset._get_homo_with_depth` (dataset.py:287-311)
    returns an all-zero `homo_z` and mask without opening `z_path`, and `_get_single_item` delivers its blob without `homo_z_out`
    (dataset.py:444,460) -- the missing key is what makes `annots_on_the_fly` render.  True only when the loader was rebound too."""
    import torch

    from . import gen_z, labels

    meshes = gen_z.load_models(models_dir, torch.device("cuda", torch.cuda.current_device()), scale=1.0)
    labels.set_depth_source(meshes, gen_z.NEAR * 1000.0, gen_z.FAR * 1000.0)
    return _detach_loader_from_z_crop()


def _detach_loader_from_z_crop() -> bool:
    """Rebinds the two loader methods that read and deliver the stored depth (idempotent); False when the reference's `dataset` module
    cannot be imported (then the caller's own loader has to leave `homo_z_out` out)."""
    import numpy as np

    try:
        ref = importlib.import_module("dataset")
        cls = ref.BOP_Dataset
        orig_item = cls._get_single_item
    except Exception:  # the reference's loader needs cv2, imgaug, ...; absent pieces are the caller's problem
        return False
    if getattr(cls, "_lc_amd_native_depth", False):
        return True

    def _get_homo_with_depth(self, annot, size_hw, fill_hole=True):
        size_hw = tuple(size_hw)
        return np.zeros(size_hw + (3,), dtype=np.float32), np.zeros(size_hw, dtype=np.float32)

    def _get_single_item(self, index):
        blob = orig_item(self, index)
        if isinstance(blob, dict):
            blob.pop("homo_z_out", None)
        return blob

    cls._get_homo_with_depth = _get_homo_with_depth
    cls._get_single_item = _get_single_item
    cls._lc_amd_native_depth = True
    return True


def _install_sym(models_info) -> bool:
    """The symmetry transforms of `models_info` (a BOP models_info.json) on the current device as the labels' symmetry source, and the
    reference's loader taken off the candidates: True only when the loader's name was rebound too."""
    import torch

    from . import labels, symmetry

    labels.set_symmetry_source(symmetry.SymmetrySet.from_models_info(models_info, device=torch.device("cuda", torch.cuda.current_device())))
    return _detach_loader_from_candidates()


def _detach_loader_from_candidates() -> bool:
    """Rebinds `symmetry_pose_candidates` of the module the reference's `dataset` calls it on (dataset.py:15,405) to return the base pose
    alone, (1,3,4) (idempotent); False when neither `dataset` nor `symmetry` of the reference can be imported (then the caller's own loader
    ships what it likes: `Rt_candi` is ignored while a symmetry source is set)."""
    import numpy as np

    try:
        mod = importlib.import_module("dataset").symmetry
    except Exception:  # the reference's loader needs cv2, imgaug, ...: the module it would call is the top-level `symmetry`
        try:
            mod = importlib.import_module("symmetry")
        except Exception:
            return False
    if not hasattr(mod, "symmetry_pose_candidates"):
        return False
    if getattr(mod.symmetry_pose_candidates, "_lc_amd_native_sym", False):
        return True

    def symmetry_pose_candidates(base_R, base_t, model_info=None, continuous_steps=384):
        return np.concatenate((np.asarray(base_R), np.asarray(base_t)[..., None]), axis=-1)[None]

    symmetry_pose_candidates._lc_amd_native_sym = True
    mod.symmetry_pose_candidates = symmetry_pose_candidates
    return True


def _install_crops() -> bool:
    """Rebinds the test-time loader and the transfer (idempotent); False when the reference's `dataset` or `utils` cannot be imported.
    `finish_blob` needs the size of the network's input, which no blob carries: the rebound `collate_fn` (called where the loader is
    built, utils.py:37) and the rebound `_get_single_item` note it from the dataset object."""
    from . import crops

    try:
        ref = importlib.import_module("dataset")
        utils = importlib.import_module("utils")
        cls = ref.BOP_Dataset
        orig_item, orig_collate, orig_xfer = cls._get_single_item, cls.collate_fn, utils.xfer_to
    except Exception:  # the reference's loader needs imgaug, pycocotools, ...; absent pieces are the caller's problem
        return False

    def note_size(ds):
        w, h = ds.net_input_wh
        crops.set_net_input_hw((h, w))

    if not getattr(cls, "_lc_amd_native_crops", False):
        def _get_single_item(self, index):
            if self.training:
                return orig_item(self, index)
            note_size(self)
            return crops.test_item(self, index)

        def collate_fn(self):
            if not self.training:
                note_size(self)
            return orig_collate(self)

        cls._get_single_item = _get_single_item
        cls.collate_fn = collate_fn
        cls._lc_amd_native_crops = True
    if not getattr(orig_xfer, "_lc_amd_native_crops", False):
        def xfer_to(pack, device, non_blocking=True):
            return crops.finish_blob(orig_xfer(pack, device, non_blocking=non_blocking))

        xfer_to._lc_amd_native_crops = True
        utils.xfer_to = xfer_to
        test = sys.modules.get("test")
        if test is not None and getattr(test, "xfer_to", None) is orig_xfer:
            test.xfer_to = xfer_to  # `from utils import xfer_to` (test.py:9) ran before the rebinding
    return True


def _install_optim() -> bool:
    from . import optim

    try:
        ref = importlib.import_module("lib.optim.ranger")
    except Exception:
        return False
    ref.Ranger = optim.Ranger
    utils = sys.modules.get("utils")
    if utils is not None and getattr(utils, "Ranger", None) is not None and getattr(utils, "__file__", None) and \
            os.path.dirname(os.path.abspath(utils.__file__)) == os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(ref.__file__)))):
        utils.Ranger = optim.Ranger  # `from lib.optim.ranger import Ranger` (utils.py:10) ran before the rebinding
    return True


_FLAGS = ("--native-labels", "--native-optim", "--native-crops")
_VALUE_FLAGS = ("--native-depth", "--native-sym")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    flags, values = set(), {}
    while argv and (argv[0] in _FLAGS or argv[0] in _VALUE_FLAGS):
        if argv[0] in _VALUE_FLAGS:
            if len(argv) < 2:
                raise SystemExit(f"lc_amd.dropin: {argv[0]} needs a value")
            name = argv.pop(0)
            values[name] = argv.pop(0)
        else:
            flags.add(argv.pop(0))
    native_labels, native_optim = "--native-labels" in flags, "--native-optim" in flags
    if not argv:
        raise SystemExit(__doc__)
    script = argv[0]
    sys.path.insert(0, os.path.dirname(os.path.abspath(script)))
    # native_optim (and native_crops) is passed only when asked for: without the flag install() gets exactly the arguments it got before the flag existed
    kw = dict(native_labels=native_labels, **({"native_optim": True} if native_optim else {}),
              **({"native_depth": values["--native-depth"]} if "--native-depth" in values else {}),
              **({"native_crops": True} if "--native-crops" in flags else {}),
              **({"native_sym": values["--native-sym"]} if "--native-sym" in values else {}))
    print("lc_amd.dropin:", install(**kw), file=sys.stderr)
    sys.argv = argv
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
