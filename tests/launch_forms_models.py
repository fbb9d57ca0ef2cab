"""Which GPU tests launch each compiled kernel form of liblc_amd_models.so: the table tests/launch_forms.py keeps for liblc_amd.so, for the
model-preparation library (checked by tests/test_models_library.py against the library's symbols).

FORMS: (regex over the mangled kernel name, tests "module::function" that launch every form the regex matches).  Which form a test launches
follows from its shapes: the entry point launches the resident instance of the points kernel when the set holds a mesh of up to
lc_amd.models.FPS_RESIDENT vertices and the streaming instance when it holds a larger one, and both diameter kernels whenever a diameter
output is given.
"""

FORMS = [
    (r"lc_model_points_kernelILb1E", ["test_gpu_models::test_single_mesh_equals_the_oracle_bit_for_bit", "test_gpu_models::test_fps_counts_and_prefixes"]),
    (r"lc_model_points_kernelILb0E", ["test_gpu_models::test_streaming_form_prefix_and_counts", "test_gpu_models::test_a_set_of_meshes_equals_the_single_mesh_calls"]),
    (r"lc_model_diameter_kernel", ["test_gpu_models::test_single_mesh_equals_the_oracle_bit_for_bit", "test_gpu_models::test_tie_rules_on_the_cube"]),
    (r"lc_model_diameter_reduce_kernel", ["test_gpu_models::test_single_mesh_equals_the_oracle_bit_for_bit", "test_gpu_models::test_tie_rules_on_the_cube"]),
]
