"""Registry of the library's tuning knobs (mdbn_set_option, csrc/mdbn_capi.hip): one entry per option name (TEST-ONLY data, no
GPU needed).

Each entry gives the knob's default (the value of a fresh context), the values mdbn_set_option accepts and some it must refuse
(MDBN_EINVAL, the previous setting kept), and the tests that drive the knob on a GPU (node ids relative to tests/).
tests/test_knob_registry.py keeps this table, the library and include/mdbn_hip.h in step: a knob added to mdbn_set_option
without an entry here -- and so without a test that sets it -- fails the CPU suite."""

_K = "test_gpu_knobs.py::"

KNOBS = {
    # --- tiled GEMM plan (plan_gemm / try_bf16x6) ---
    "gemm_bk": dict(default=0, valid=[0, 32, 64], invalid=[-1, 16, 128],
                    tests=[_K + "test_tiled_gemm_plan_knobs_against_forced_oracle"]),
    "gemm_cw": dict(default=0, valid=[0, 1, 2], invalid=[-1, 3],
                    tests=[_K + "test_tiled_gemm_plan_knobs_against_forced_oracle"]),
    "gemm_min_splitk": dict(default=128, valid=[32, 128, 4096], invalid=[0, 31, 1 << 31],
                            tests=[_K + "test_tiled_gemm_plan_knobs_against_forced_oracle"]),
    "gemm_bf16x6": dict(default=3, valid=[0, 1, 2, 3], invalid=[-1, 4, 7],
                        tests=["test_gpu_parity.py::test_bf16x6_gemm_is_f32_grade",
                               "test_gpu_parity.py::test_bf16x6_ragged_shapes_match_exact_kernel",
                               _K + "test_tiled_gemm_plan_knobs_against_forced_oracle"]),
    "x6_min_jobs": dict(default=48, valid=[0, 48, 1 << 20], invalid=[-1, 1 << 31],
                        tests=[_K + "test_bf16x6_job_floor_and_producer_waves"]),
    "x6_producer_waves": dict(default=4, valid=[2, 4], invalid=[0, 1, 3, 8],
                              tests=[_K + "test_bf16x6_job_floor_and_producer_waves"]),
    # --- activation epilogue of split-K forward passes ---
    "epilogue_cw": dict(default=0, valid=[0, 1, 2, 4], invalid=[-1, 3, 8],
                        tests=[_K + "test_epilogue_geometry_is_bitwise_the_auto_choice"]),
    "epilogue_threads": dict(default=0, valid=[0, 64, 128, 256], invalid=[-1, 32, 512],
                             tests=[_K + "test_epilogue_geometry_is_bitwise_the_auto_choice"]),
    "fused_epilogue": dict(default=1, valid=[0, 1], invalid=[],
                           tests=["test_gpu_parity.py::test_fused_epilogue_equals_unfused",
                                  _K + "test_epilogue_geometry_is_bitwise_the_auto_choice"]),
    # --- register-streaming kernels ---
    "skinny_gemm": dict(default=1, valid=[0, 1], invalid=[],
                        tests=["test_gpu_parity.py::test_skinny_gemm_matches_oracle_and_tile_kernel"]),
    "skinny_fused_max_k": dict(default=1024, valid=[0, 64, 1024, 1 << 20], invalid=[-1, 1 << 31],
                               tests=[_K + "test_skinny_limits_against_forced_oracle"]),
    "skinny_max_macs": dict(default=32 << 20, valid=[0, 32 << 20, 1 << 40], invalid=[-1, 1 << 62],
                            tests=[_K + "test_skinny_limits_against_forced_oracle"]),
    "stream_x6": dict(default=2, valid=[0, 1, 2], invalid=[-1, 3, 6],
                      tests=["test_gpu_stream.py::test_stream_step_against_forced_oracle",
                             "test_gpu_stream.py::test_stream_step_draws_the_uniforms_of_the_tiled_path"]),
    "stream_max_macs": dict(default=1 << 30, valid=[0, 1 << 30], invalid=[-1],
                            tests=[_K + "test_stream_size_limit_zero_keeps_every_pass_off_the_streaming_kernel"]),
    "stream_mi": dict(default=0, valid=[0, 1, 2], invalid=[-1, 3, 4],
                      tests=["test_gpu_stream.py::test_stream_step_against_forced_oracle",
                             _K + "test_every_stream_tile_shape_against_forced_oracle"]),
    "stream_ni": dict(default=0, valid=[0, 1, 2], invalid=[-1, 3, 4],
                      tests=[_K + "test_every_stream_tile_shape_against_forced_oracle"]),
    # --- one-launch / thin / group-chain steps ---
    "small_fused": dict(default=1, valid=[0, 1], invalid=[],
                        tests=["test_gpu_small.py::test_one_launch_step_draws_the_uniforms_of_the_multi_launch_path"]),
    "small_fin_lanes": dict(default=0, valid=[0, 1, 2, 4, 8, 16], invalid=[-1, 3, 32],
                            tests=[_K + "test_small_finish_lanes_against_forced_oracle"]),
    "thin_fused": dict(default=1, valid=[0, 1], invalid=[],
                       tests=["test_gpu_thin.py::test_thin_step_draws_the_uniforms_of_the_streaming_path"]),
    "gchain": dict(default=0, valid=[0, 1], invalid=[],
                   tests=["test_gpu_gchain.py::test_group_chain_step_against_forced_oracle"]),
    # --- bf16 plane path ---
    "gemm_planes": dict(default=1, valid=[0, 1], invalid=[],
                        tests=["test_gpu_planes.py::test_a_ragged_layer_trains_on_padded_planes_as_on_the_exact_path"]),
    "planes_mfma": dict(default=16, valid=[16, 32], invalid=[0, 8, 64],
                        tests=["test_gpu_planes.py::test_plane_step_equals_f32_operand_step_bit_for_bit"]),
    "planes_min_work": dict(default=1 << 30, valid=[0, 1 << 30], invalid=[-1],
                            tests=["test_gpu_planes.py::test_plane_path_serves_big_layers_only_by_default"]),
    "early_w": dict(default=1, valid=[0, 1], invalid=[],
                    tests=["test_gpu_planes.py::test_early_parameter_half_is_bitwise_the_epilogue_update"]),
    "narrow_tiles": dict(default=1, valid=[0, 1], invalid=[],
                         tests=["test_gpu_planes.py::test_plane_step_against_oracle_teacher_forced"]),
    "bf16_inputs": dict(default=0, valid=[0, 1], invalid=[],
                        tests=["test_gpu_planes.py::test_bf16_input_reporting_mode"]),
    "comm_cus": dict(default=0, valid=[0, 8, 192], invalid=[-1, 193],
                     tests=["test_gpu_planes.py::test_balanced_launches_match_and_repeat"]),
    "bal_blocks": dict(default=0, valid=[0, 7, 13, 256], invalid=[-1, 257],
                       tests=[_K + "test_balanced_workgroup_count_against_forced_oracle"]),
    # --- the training step ---
    "fused_update": dict(default=1, valid=[0, 1], invalid=[],
                         tests=["test_gpu_parity.py::test_fused_update_is_bitwise_the_separate_update",
                                _K + "test_fused_finalize_and_update_are_bitwise_the_separate_kernels"]),
    "fused_finalize": dict(default=1, valid=[0, 1], invalid=[],
                           tests=[_K + "test_fused_finalize_and_update_are_bitwise_the_separate_kernels"]),
    "update_overlap": dict(default=0, valid=[0, 1], invalid=[],
                           tests=[_K + "test_update_overlap_is_bitwise_the_serial_update"]),
    "gather_ahead": dict(default=1, valid=[0, 1], invalid=[],
                         tests=[_K + "test_gather_ahead_off_is_bitwise_the_same_run"]),
    "feed_copy_streams": dict(default=1, valid=[1, 2], invalid=[0, 3],
                              tests=[_K + "test_host_feed_copy_streams_are_bitwise_the_device_table"]),
}
