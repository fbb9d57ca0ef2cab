"""lc_amd -- MI355X-native hot path of fulliu/lc (linear-covariance pose loss, weighted PnP, keypoint soft-argmax).

Call surface (mirrors the reference):
    lc_amd.cov_mixed.Loss_cov_mixed      <- lib/cov_mixed.py:100
    lc_amd.pnp.cer_solver.solve          <- lib/pnp/cer_solver.py:6
    lc_amd.pnp.pnp_ceres.solve           <- lib/pnp/pnp_ceres.py:6
    lc_amd.ptnet.softargmax_2d_std       <- ptnet.py:100
    lc_amd.losses.Loss_fn                <- losses.py:239
    lc_amd.grad.NormClipper              <- lib/utils/grad.py:5
    lc_amd.kpt.kpt_nll_mean              <- losses.py:318 (sparse_kpt_loss)
    lc_amd.dense.dense_front_end / dense_select   <- losses.py:142-161,355-356 / test.py:39-45,94-113
    lc_amd.floatbits                     <- floatbits.py (ZebraPose codes)
    lc_amd.pnp.gpu_solver.solve          <- lib/pnp/cv2_solver.py:8 (RANSAC initialiser)
    lc_amd.metrics.compute_pose_errors   <- lib/utils/evaluate.py:333
    lc_amd.inference.solve_pnp           <- test.py:47-136
    lc_amd.graphs.GraphedLoss / inference.GraphedSolvePnP   hipGraph replay of the launch-bound steps
    lc_amd.optim.Ranger                  <- lib/optim/ranger.py:29 (fused step, liblc_amd_optim.so; opt-in in the drop-in)
    lc_amd.posecov.pose_covariance       <- lib/nll/pnp_auto.py:86 diff_pnp_perturb(with_cov=True) + lib/cov_mixed.py:52-97 (one launch, liblc_amd_posecov.so)
    lc_amd.inference.solve_pnp_with_cov  solve_pnp + the covariance and predicted error of every weighted pose
    lc_amd.render.render_depth / render_homo_z_out   <- tools/gen_z.py:153 (the EGL renderer) + dataset.py:287-311,444 (depth rasteriser, liblc_amd_render.so)
    lc_amd.gen_z                         <- tools/gen_z.py (python -m lc_amd.gen_z: the z_crop files without OpenGL)
    lc_amd.crops.warp_affine / test_item / finish_blob   <- dataset.py:409-411 cv2.warpAffine + .div(255) + test.py:163 Normalize (zoom-in crops, liblc_amd_crop.so)
    lc_amd.models.prepare / to_models_info / to_fps_dict   the per-object inputs every path reads: extents, exact diameter, FPS keypoints (liblc_amd_models.so)
    lc_amd.prep_models                   python -m lc_amd.prep_models: models_info.json and the `cfg_global.fps` pickle (dataset.py:232-236) of a directory of meshes
    lc_amd.obox.oriented_box / to_models_xform   <- model_transform.py:21-42 reads it, nothing in the reference writes it: `models_xform.json` (the rigid transform and half-extents of each model's minimum-volume oriented box over a stated grid search; liblc_amd_obox.so; python -m lc_amd.prep_models --xform)
    lc_amd.symfind.deviation / check_symmetries / propose_symmetries   BOP's geometric rule for a model symmetry (max over the vertices of the distance from the transformed vertex to the nearest one, below max(15 mm, 0.1 diameter)) evaluated on the device: checks the `symmetries_discrete` / `symmetries_continuous` of a models_info.json against the meshes and proposes them for an object that has none (liblc_amd_symfind.so; python -m lc_amd.prep_models --check-symmetries / --symmetries)
    lc_amd.maskcrop.mask_crops           <- dataset.py:414,425-442 (msk_in / msk_vis / msk_noc warps, valid_cnt, sym_ck_pts2d; liblc_amd_maskcrop.so)
    lc_amd.augment.augment / augment_drawn / draw / background_matrices / draw_zoom   <- dataset.py:137-171,313-327,402,413-419 (background switch, colour augmentation, zoom-in box draw; liblc_amd_augment.so)
    lc_amd.backgrounds.BackgroundStore / switch_backgrounds   <- dataset.py:137-148,413-415 (_switch_bg with np.random.choice(self.bg_list): each row's background picked, cut and blended from a resident store; liblc_amd_bgstore.so)
    lc_amd.shade.shade / shade_scene / render_color / render_scene   <- tools/lib/meshrenderer/meshrenderer_phong.py:125-165 + dataset.py:413 (the `imgn` image: vertex colours under a Phong model behind the rasteriser's face map; liblc_amd_shade.so)
    lc_amd.texture.shade / shade_scene / render_color / render_scene / TextureStore / TexturedAppearance / read_ply_textured   <- tools/lib/pysixd/inout.py:505-617 (models with texture_u / texture_v or a face texcoord list and a texture image: the same frames with the albedo sampled from a resident store of mip-mapped textures at per-corner coordinates; liblc_amd_texture.so)
    lc_amd.sampler.AnnotationTable / draw_rows / select_rows / take_rows   <- dataset.py:332-338 and the DataLoader's sampler and collate (a step's rows drawn from the seed word: every annotation once per epoch, spares at random; rows whose crop is too empty replaced by good spares in order; the batch gathered; liblc_amd_sampler.so)
    lc_amd.trainset.TrainSet.step_inputs   the chain of lc_amd.train_inputs behind a resident annotation table: one seed word decides the step's batch, the cheap stages run on batch + spare rows, the expensive ones on exactly `batch`
    lc_amd.dropin                        run the reference's train.py / test.py on all of the above without editing them
Native code: lc_amd/csrc/*.hip -> lc_amd/_C/liblc_amd.so (C ABI in include/lc_amd.h);
lc_amd/csrc/optim/*.hip -> lc_amd/_C/liblc_amd_optim.so (include/lc_amd_optim.h);
lc_amd/csrc/posecov/*.hip -> lc_amd/_C/liblc_amd_posecov.so (include/lc_amd_posecov.h);
lc_amd/csrc/render/*.hip -> lc_amd/_C/liblc_amd_render.so (include/lc_amd_render.h);
lc_amd/csrc/crop/*.hip -> lc_amd/_C/liblc_amd_crop.so (include/lc_amd_crop.h);
lc_amd/csrc/models/*.hip -> lc_amd/_C/liblc_amd_models.so (include/lc_amd_models.h);
lc_amd/csrc/maskcrop/*.hip -> lc_amd/_C/liblc_amd_maskcrop.so (include/lc_amd_maskcrop.h);
lc_amd/csrc/augment/*.hip -> lc_amd/_C/liblc_amd_augment.so (include/lc_amd_augment.h).
"""
__version__ = "0.1.0"
