"""Which GPU tests launch each compiled kernel form of liblc_amd.so (checked by tests/test_launch_forms.py against the library's symbols).

FORMS: (regex over the mangled kernel name, tests "module::function" that launch every form the regex matches).  A form is a template
instance: its own vector width, per-thread count, LDS layout and tail handling, so each one needs a test whose shape, dtype or alignment
makes the launcher pick it.  Measured with scripts/kernel_coverage.py over rocprofv3 kernel traces of the GPU suite, one per test file
(profiles/coverage/launch_forms_after.txt): every form an entry matches is launched by the files of the tests it names, and each of those
files launches one of them at least; which test of a file does it follows from its shapes (the tests added with this table say so in their
docstrings).

UNREACHABLE: regex -> why no call of the library can launch that form (it is compiled because the launcher's choice is a run-time one).
"""

_T = r"(?:f|DF16_|DF16b)"  # the element types of the maps: float, _Float16, __bf16

FORMS = [
    # ---- lc_bits.hip: binary-code decode -------------------------------------------------------------------------------------
    (r"lc_bits_decode_gt_fwd_kernelILi4E" + _T, ["test_gpu_bits::test_bits_decode_vs_reference", "test_gpu_map_dtypes::test_code_decode_reads_logits_natively"]),
    (r"lc_bits_decode_gt_fwd_kernelILi1E" + _T, ["test_gpu_bits::test_bits_more_than_65535_samples_take_the_generic_forward"]),
    (r"lc_bits_decode_gt_fwd_wide_kernelI" + _T, ["test_gpu_bits::test_bits_strided_subset_and_zlmo_shape", "test_gpu_map_dtypes::test_code_decode_reads_logits_natively"]),
    (r"lc_bits_decode_gt_bwd_kernelILi4E" + _T, ["test_gpu_bits::test_bits_decode_vs_reference", "test_gpu_map_dtypes::test_code_decode_reads_logits_natively"]),
    (r"lc_bits_decode_gt_bwd_kernelILi1E" + _T, ["test_gpu_bits::test_bits_odd_widths_take_the_scalar_path",
                                                  "test_gpu_bits::test_bits_more_than_65535_samples_take_the_generic_forward"]),
    (r"lc_bits_decode_gt_bwd_tile_kernelILi(?:4Ef|8EDF16_|8EDF16b)Li(?:2ELi[124]|3ELi[1234])E", ["test_gpu_bits::test_bits_tile_backward_forms"]),
    (r"lc_bits_decode_kernelILi[14]E" + _T, ["test_gpu_bits::test_bits_decode_vs_reference", "test_gpu_bits::test_bits_odd_widths_take_the_scalar_path",
                                              "test_gpu_map_dtypes::test_test_time_path_on_16bit_network_outputs"]),
    (r"lc_bits_decode_rows_kernelI" + _T, ["test_gpu_test_time::test_decode_of_the_selected_rows_equals_the_whole_map_decode",
                                           "test_gpu_map_dtypes::test_test_time_path_on_16bit_network_outputs"]),
    # ---- lc_capi.hip / lc_clip.hip -------------------------------------------------------------------------------------------
    (r"lc_scale_rows_kernel", ["test_gpu_loss::test_loss_kernel_vs_oracle_shapes"]),  # the autograd backward of the loss
    (r"lc_(?:sqnorm|clip_apply)_kernelIf", ["test_gpu_clip::test_clipper_vs_reference_trajectory", "test_gpu_clip::test_clipper_large_tensor_lists_and_determinism"]),
    (r"lc_(?:sqnorm|clip_apply)_kernelIDF16[_b]", ["test_gpu_dense::test_loss_fn_at_training_shapes_with_half_precision_heads"]),  # hooks on 16-bit maps
    # ---- lc_dense.hip / lc_dense_aux.hip / lc_select.hip: the dense branch ---------------------------------------------------
    (r"lc_dense_frontend_fwd_kernelI(?:ff|DF16_DF16_|DF16bDF16b|DF16_f|DF16bf)E", ["test_gpu_dense::test_dense_front_end_vs_oracle",
                                                                                  "test_gpu_map_dtypes::test_dense_front_end_reads_maps_natively",
                                                                                  "test_gpu_map_dtypes::test_fp32_coordinate_map_next_to_16bit_logits_keeps_an_fp32_gradient"]),
    (r"lc_dense_frontend_bwd_kernelILb[01]E" + _T, ["test_gpu_dense::test_dense_front_end_vs_oracle", "test_gpu_map_dtypes::test_dense_front_end_reads_maps_natively"]),
    (r"lc_dense_frontend_select_kernelI(?:ff|DF16_DF16_|DF16bDF16b)Lb[01]E", ["test_gpu_select::test_front_end_and_selection_in_one_launch",
                                                                              "test_gpu_map_dtypes::test_front_end_and_selection_read_maps_natively"]),
    (r"lc_dense_frontend_select_split_kernelI(?:ff|DF16_DF16_|DF16bDF16b)E", ["test_gpu_select::test_several_workgroups_per_object_select_what_one_workgroup_selects",
                                                                             "test_gpu_select::test_split_selection_soak_over_random_shapes"]),
    (r"lc_dense_frontend_select_split_kernelI(?:DF16_f|DF16bf)E|lc_dense_frontend_select_kernelI(?:DF16_f|DF16bf)Lb[01]E",
     ["test_gpu_select::test_fp32_coordinates_next_to_16bit_logits_select_what_fp32_logits_select"]),
    (r"lc_dense_select_kernel", ["test_gpu_select::test_select_vs_reference_golden", "test_gpu_select::test_select_vs_oracle_sizes"]),
    (r"lc_dense_aux_(?:fwd|bwd)_kernelILi[14]ELi[01]E" + _T, ["test_gpu_dense::test_dense_aux_losses_equal_the_torch_formulas",
                                                               "test_gpu_map_dtypes::test_auxiliary_losses_read_maps_natively"]),
    (r"lc_xyz_bin_loss_(?:fwd|bwd)_kernelI" + _T, ["test_gpu_dense::test_xyz_bin_loss_equals_the_torch_formulas", "test_gpu_map_dtypes::test_auxiliary_losses_read_maps_natively"]),
    (r"lc_xyz_bin_loss_bwd_plane_kernelILi(?:4Ef|8EDF16_|8EDF16b)E", ["test_gpu_dense::test_xyz_bin_loss_equals_the_torch_formulas",
                                                                       "test_gpu_map_dtypes::test_auxiliary_losses_read_maps_natively"]),
    (r"lc_xyz_bin_loss_finish_kernel", ["test_gpu_xyz_bin_sharded::test_one_rank_group_is_the_one_launch_kernel"]),
    # ---- lc_fused*.hip: the pose unit ----------------------------------------------------------------------------------------
    (r"lc_pose_unit_kernelILi[12]E", ["test_gpu_fused::test_pose_unit_equals_separate_kernels"]),
    (r"lc_pose_unit_dense_kernelILi[48]E", ["test_gpu_fused::test_dense_pose_unit_equals_separate_kernels"]),
    # ---- lc_head.hip: the keypoint head ---------------------------------------------------------------------------------------
    (r"lc_head_fwd_kernelI" + _T + r"Li(?:1|2|4|8|16|32)ELi[14]E", ["test_gpu_head::test_head_fwd_forms_fp32_vs_fp64", "test_gpu_head::test_head_fwd_forms_16bit_match_the_fp32_kernel"]),
    (r"lc_head_fwd_kernelI" + _T + r"Li16ELi1E", ["test_gpu_head::test_head_64x64_forms_at_offset_views"]),
    (r"lc_head_fwd_rows_kernelI(?:DF16_|DF16b)Li16ELi4E", ["test_gpu_head::test_head_64x64_forms_at_offset_views"]),
    (r"lc_head_fwd_rows_kernelIfLi16ELi4E", ["test_gpu_head::test_head_rows_kernel_with_misaligned_outputs"]),
    (r"lc_head_fwd_rows_kernelI" + _T + r"Li32ELi16E", ["test_gpu_head::test_head_odd_shapes_vs_torch", "test_gpu_head::test_head_16bit_maps_match_the_fp32_kernel_on_the_same_values"]),
    (r"lc_head_fwd_wave64_kernelI" + _T + r"Lb[01]E", ["test_gpu_head::test_head_vs_golden", "test_gpu_head::test_head_16bit_maps_match_the_fp32_kernel_on_the_same_values"]),
    (r"lc_head_bwd_kernelIfLi(?:4ELb[01]|1ELb0)E", ["test_gpu_head::test_head_fwd_forms_fp32_vs_fp64", "test_gpu_head::test_head_64x64_forms_at_offset_views"]),
    (r"lc_head_bwd_kernelI(?:DF16_|DF16b)Li8ELb1E", ["test_gpu_head::test_head_16bit_maps_match_the_fp32_kernel_on_the_same_values"]),
    (r"lc_head_bwd_kernelI(?:DF16_|DF16b)Li(?:8ELb0|4ELb[01]|1ELb0)E", ["test_gpu_head::test_head_fwd_forms_16bit_match_the_fp32_kernel",
                                                                        "test_gpu_head::test_head_64x64_forms_at_offset_views"]),
    # ---- lc_kpt.hip / lc_metrics.hip ------------------------------------------------------------------------------------------
    (r"lc_kpt_nll_kernel", ["test_gpu_kpt::test_kpt_nll_vs_oracle"]),
    # one form; the tests after the first walk the paths inside it (tile, pair-slot and query-group edges, offsets, want_adi, the scalars)
    (r"lc_pose_errors_kernel", ["test_gpu_metrics::test_pose_errors_vs_reference_golden", "test_gpu_metrics::test_pose_errors_packed_objects_and_large_cloud",
                                "test_gpu_metrics::test_witness_clouds_in_one_packed_launch",
                                "test_gpu_metrics::test_packed_poses_equal_their_own_launches_and_repeat_bit_for_bit",
                                "test_gpu_metrics::test_symmetric_object_adi_finds_another_vertex", "test_gpu_metrics::test_large_random_rotation_errors",
                                "test_gpu_metrics::test_identical_poses_give_exact_zeros", "test_gpu_metrics::test_without_adi_the_other_outputs_keep_their_bits",
                                "test_gpu_metrics::test_rotation_error_to_the_last_float32_digit", "test_gpu_metrics::test_translations_as_columns",
                                "test_gpu_metrics::test_pose_errors_from_states_with_quaternions_of_any_length"]),
    # ---- lc_labels.hip: on-device label preparation ----------------------------------------------------------------------------
    (r"lc_sym_select_kernelILi(?:1|4)ELi512E", ["test_gpu_labels::test_selection_sweep_vs_fp64_oracle"]),
    (r"lc_sym_select_kernelILi16ELi256E", ["test_gpu_labels::test_selection_sweep_vs_fp64_oracle"]),
    (r"lc_sym_select_kernelILi(?:2|8)ELi512E", ["test_gpu_labels::test_selection_points_per_lane_2_and_8_vs_fp64_oracle"]),
    (r"lc_label_targets_kernelILi8E", ["test_gpu_labels::test_annots_on_the_fly_vs_reference", "test_gpu_labels::test_label_targets_forms_are_identical_on_the_same_pixels"]),
    (r"lc_label_targets_kernelILi[14]E", ["test_gpu_labels::test_label_targets_pix4_and_pix1_vs_fp64_oracle",
                                          "test_gpu_labels::test_label_targets_forms_are_identical_on_the_same_pixels"]),
    # ---- lc_loss.hip: the LC loss ---------------------------------------------------------------------------------------------
    (r"lc_cov_loss_kernelILb1ELb0E", ["test_gpu_loss::test_loss_kernel_vs_oracle_shapes"]),
    (r"lc_cov_loss_kernelILb0ELb0E", ["test_gpu_loss::test_loss_kernel_vs_oracle_shapes", "test_gpu_loss::test_tiled_form_is_bit_identical_to_the_one_workgroup_form"]),
    (r"lc_cov_loss_tiled_kernelILb0E", ["test_gpu_loss::test_tiled_form_is_bit_identical_to_the_one_workgroup_form"]),
    (r"lc_cov_loss_kernelILb1ELb1E", ["test_gpu_loss::test_loss_kernel_vs_golden"]),
    (r"lc_cov_loss_kernelILb0ELb1E|lc_cov_loss_tiled_kernelILb1E", ["test_gpu_loss::test_cov2d_dense_forms_vs_oracle_and_each_other"]),
    # ---- lc_pnp*.hip: the PnP solve --------------------------------------------------------------------------------------------
    (r"lc_pnp_lm_kernelILb1ELi[12]ELb[01]E", ["test_gpu_pnp::test_pnp_device_route_vs_oracle", "test_gpu_pnp::test_large_grid_build_equals_the_latency_build",
                                              "test_gpu_pnp::test_fused_nan_filter_with_full_information_factor"]),
    (r"lc_pnp_lm_wide_kernelILb[01]ELb[01]ELi(?:0|4|8|16)ELb[01]E", ["test_gpu_pnp::test_pnp_device_route_vs_oracle", "test_gpu_edges::test_pnp_dense_sizes_vs_oracle",
                                                                     "test_gpu_pnp_split::test_shapes_outside_the_split_form_take_the_plain_kernel"]),
    (r"lc_pnp_lm_split_(?:rescue_)?kernelILb[01]E", ["test_gpu_pnp_split::test_split_solve_equals_the_one_workgroup_solve",
                                                      "test_gpu_pnp_split::test_split_solve_with_load_time_options_and_shared_poses"]),
    (r"lc_pnp_lm_chain_kernel|lc_pnp_lm_chain_small_kernel", ["test_gpu_pnp::test_chained_solves_equal_the_two_calls"]),
    (r"lc_pnp_lm_(?:wide_)?trace_kernel", ["test_gpu_pnp_trace::test_schedule_lockstep_well_posed"]),
    # ---- lc_pnp_init.hip: the P3P RANSAC ---------------------------------------------------------------------------------------
    (r"lc_pnp_ransac_kernel", ["test_gpu_pnp_init::test_p3p_ransac_noise_free_is_exact", "test_gpu_pnp_init_oracle::test_ransac_kernel_vs_oracle_fixture"]),
    (r"lc_ransac_(?:hypotheses|score|score_live|score_wide|score_select|select|select_wide)_kernel", ["test_gpu_pnp_init_oracle::test_split_form_equals_single_launch",
                                                                                                      "test_gpu_ransac_exact::test_ransac_integers_equal_the_float32_oracle_on_seeded_batches"]),
]

UNREACHABLE = {
    r"lc_bits_decode_gt_bwd_tile_kernelI(?:Li4Ef|Li8EDF16_|Li8EDF16b)Li2ELi3E":
        "sample 2, three rows per tile: R = 3 and R = 4 need the same ceil(R / 2) sampled rows, so R = 4 is refused only for a row of more than "
        "64 pieces, and no piece count dividing 256 lies in (64, 85] (launch_bits_decode_gt_bwd)",
    r"lc_head_bwd_kernelIfLi8ELb[01]E":
        "eight elements per access are chosen for 2-byte maps only (vec8 = sizeof(T) == 2 && ..., launch_head_bwd_t): compiled for float "
        "because the test is a run-time one",
}
