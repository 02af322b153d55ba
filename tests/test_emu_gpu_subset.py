"""Most of the -m gpu suite, run on the CPU: the SAME test functions (grouping, rotated-box kernels and IoU metrics, input
construction, the fused front, every stage of a PointNet scale, the fused FCN against the module path, and the whole model
against the golden vectors of the reference for the car, people, refine and SUN-RGBD configurations -- train + eval logits,
losses, gradient norms, running statistics --, every parameter gradient against the fp64 oracle, decode + NMS pipeline) with
the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness).
The hardware run of these tests stays the parity gate; this tier catches index / layout / reduction mistakes -- in the kernels
and in the host code that drives them -- without a GPU.  (FCN_EMULATE=1 python -m pytest tests -m gpu -k ... runs any other
GPU test the same way.  Not here: the B=32 full-size cases (minutes) and a few
whole-model cases that add run time but no new kernel path, hipGraph capture / replay and RCCL (cannot be emulated),
and the tests that assert the package REFUSES CPU tensors -- inside the shim it cannot tell.)"""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_gpu_grouping", "test_testpy_scenario", ()),
    ("test_gpu_grouping", "test_golden_full", ("car_b4_n512",)),
    ("test_gpu_grouping", "test_golden_full", ("car_b4_n512_uniform",)),
    ("test_gpu_grouping", "test_golden_full", ("refine_b4_n512",)),
    ("test_gpu_grouping", "test_golden_sha", ("car_b32_n1024",)),
    ("test_gpu_grouping", "test_golden_sha", ("people_b2_n512",)),
    ("test_gpu_grouping", "test_golden_sha", ("people_b32_n1024",)),
    ("test_gpu_grouping", "test_golden_sha", ("refine_b32_n512",)),
    ("test_gpu_grouping", "test_golden_sha", ("sunrgbd_b32_n2048",)),
    ("test_gpu_grouping", "test_ragged_shapes", (1, 1, 1, 1, 0.5)),
    ("test_gpu_grouping", "test_ragged_shapes", (2, 63, 5, 7, 0.3)),
    ("test_gpu_grouping", "test_ragged_shapes", (2, 65, 17, 64, 0.3)),
    ("test_gpu_grouping", "test_ragged_shapes", (3, 1000, 33, 200, 0.05)),
    ("test_gpu_grouping", "test_ragged_shapes", (1, 20000, 9, 16, 0.01)),
    ("test_gpu_grouping", "test_ragged_shapes", (2, 300, 70, 1, 1.0)),
    ("test_gpu_grouping", "test_boundary_is_strict_and_fp32", ()),
    ("test_gpu_grouping", "test_kernel_native_layout_matches", ()),
    ("test_gpu_grouping", "test_double_inputs_are_narrowed_like_the_reference_kernel", ()),
    ("test_gpu_grouping", "test_multi_scale_launch_equals_the_per_scale_operator", ()),
    ("test_gpu_box", "test_iou_pair_matches_golden", ()),
    ("test_gpu_box", "test_rotate_nms_matches_reference_keep_lists", ()),
    ("test_gpu_box", "test_decode_matches_oracle", (3, 64)),
    ("test_gpu_box", "test_decode_matches_oracle", (10, 128)),
    ("test_gpu_box", "test_loss_tail_iou_metrics_match_oracle", ("car_b4_n512",)),
    ("test_gpu_box", "test_loss_tail_iou_metrics_match_oracle", ("people_b2_n512",)),
    ("test_gpu_box", "test_loss_tail_iou_metrics_match_oracle", ("sunrgbd_b4_n1024",)),
    ("test_gpu_box", "test_all_background_batch_is_finite", ()),
    ("test_gpu_box", "test_detect_pipeline_matches_oracle", ()),
    ("test_gpu_box", "test_detect_matches_reference_test_loop", ("full",)),
    ("test_gpu_box", "test_half_finished_split_backward_is_refused", ()),
    ("test_gpu_inputs", "test_golden_batch_with_recorded_draws", ()),
    ("test_gpu_inputs", "test_same_numpy_seed_reproduces_the_reference_batch", ()),
    ("test_gpu_inputs", "test_against_oracle_without_augmentation_and_nearest_fallback", (False, False)),
    ("test_gpu_inputs", "test_against_oracle_without_augmentation_and_nearest_fallback", (True, False)),
    ("test_gpu_inputs", "test_against_oracle_without_augmentation_and_nearest_fallback", (False, True)),
    ("test_gpu_inputs", "test_ragged_and_odd_sizes_against_oracle", (1, 100, True)),
    ("test_gpu_inputs", "test_ragged_and_odd_sizes_against_oracle", (3, 257, False)),
    ("test_gpu_inputs", "test_ragged_and_odd_sizes_against_oracle", (6, 1024, True)),
    ("test_gpu_inputs", "test_synthetic_records_against_oracle_and_launch_into_given_buffers", ()),
    ("test_gpu_inputs", "test_batch_built_on_the_prefetch_branch_feeds_the_same_step", ()),
    ("test_gpu_inputs", "test_refine_builder_matches_reference_batch", ()),
    ("test_gpu_inputs", "test_sunrgbd_builder_matches_reference_batch", ()),
    ("test_gpu_group_compact", "test_group_compact_matches_oracle_and_unfused", (4, 512, (0.25, 0.5, 1.0, 2.0), "car")),
    ("test_gpu_group_compact", "test_group_compact_matches_oracle_and_unfused", (3, 700, (0.1, 0.2, 0.4, 0.8), "uniform")),
    ("test_gpu_group_compact", "test_group_compact_matches_oracle_and_unfused", (2, 130, (2.0, 2.0, 4.0, 8.0), "car")),
    ("test_gpu_group_compact", "test_phased_front_is_bit_identical_to_the_fused_front", (4, 512, (0.25, 0.5, 1.0, 2.0))),
    ("test_gpu_group_compact", "test_forward_weight_images_hold_the_fp16_split_bit_for_bit", ()),
    # (B4_N512_s0.25_K32_C128 of gpu_stage_check.CASES is left to the hardware: with the emulation's accumulation order ONE
    # pre-ReLU activation of that draw lands on the other side of zero -- DESIGN.md section 5 on ReLU kinks)
    ("test_gpu_pointnet", "test_stages", ((2, 128, 3.5, 16, (64, 64, 128), 1.0),)),
    ("test_gpu_pointnet", "test_stages", ((3, 200, 2.5, 32, (64, 64, 128), 0.7),)),
    ("test_gpu_pointnet", "test_stages", ((4, 512, 0.5, 64, (64, 64, 128), 0.5),)),
    ("test_gpu_pointnet", "test_stages", ((4, 512, 1.0, 64, (128, 128, 256), 1.0),)),
    ("test_gpu_pointnet", "test_stages", ((4, 512, 2.0, 128, (256, 256, 512), 2.0),)),
    ("test_gpu_pointnet", "test_uniform_variant_full_windows", ()),
    ("test_gpu_pointnet", "test_key_pool_matches_row_pool", ((4, 512, 0.25, 32, (64, 64, 128), 0.25), True)),
    ("test_gpu_pointnet", "test_key_pool_matches_row_pool", ((4, 512, 2.0, 128, (256, 256, 512), 2.0), True)),
    ("test_gpu_pointnet", "test_key_pool_matches_row_pool", ((4, 512, 1.0, 64, (128, 128, 256), 1.0), False)),
    ("test_gpu_pointnet", "test_key_pool_matches_row_pool", ((2, 128, 0.25, 16, (64, 64, 128), 0.3), True)),
    ("test_gpu_pointnet", "test_key_pool_backward_with_zero_and_negative_gamma", ((3, 200, 2.5, 32, (64, 64, 128), 0.7),)),
    ("test_gpu_pointnet", "test_key_pool_backward_with_zero_and_negative_gamma", ((4, 512, 2.0, 128, (256, 256, 512), 2.0),)),
    ("test_gpu_pointnet", "test_rebuilt_dy3_gives_bit_identical_gradients", ((3, 200, 2.5, 32, (64, 64, 128), 0.7),)),
    ("test_gpu_pointnet", "test_rebuilt_dy3_gives_bit_identical_gradients", ((4, 512, 2.0, 128, (256, 256, 512), 2.0),)),
    ("test_gpu_pointnet", "test_merged_mid_launch_gives_bit_identical_gradients", ((3, 200, 2.5, 32, (64, 64, 128), 0.7),)),
    ("test_gpu_pointnet", "test_merged_mid_launch_gives_bit_identical_gradients", ((4, 512, 1.0, 64, (128, 128, 256), 1.0),)),
    ("test_gpu_pointnet", "test_tail_launch_gives_bit_identical_gradients", ((3, 200, 2.5, 32, (64, 64, 128), 0.7), False)),
    ("test_gpu_pointnet", "test_tail_launch_gives_bit_identical_gradients", ((4, 512, 2.0, 128, (256, 256, 512), 2.0), True)),
    ("test_gpu_pointnet", "test_tail_launch_gives_bit_identical_gradients", ((2, 130, 0.5, 64, (128, 128, 256), 0.4), False)),
    ("test_gpu_model", "test_train_eval_parity", ("car_b4_n512",)),
    ("test_gpu_model", "test_train_eval_parity", ("people_b2_n512",)),
    ("test_gpu_model", "test_train_eval_parity", ("refine_b4_n512",)),
    ("test_gpu_model", "test_train_eval_parity", ("sunrgbd_b4_n1024",)),
    ("test_gpu_model", "test_dense_module_api_matches_oracle", ()),
    ("test_gpu_model", "test_fused_loss_tail_matches_torch_tail", ()),
    ("test_gpu_model", "test_fused_convnet_matches_module_path", ("refine_b4_n512",)),
    ("test_gpu_model", "test_fused_convnet_matches_module_path", ("people_b2_n512",)),
    ("test_gpu_model", "test_gradients_vs_fp64_oracle", ()),
    ("test_gpu_model", "test_fp16_operand_overflow_raises_the_flag", ()),
    # the loss tail / IoU metrics / decode / NMS off the fixture regime: every case of the two modules
    ("test_gpu_loss_tail_regimes", "test_generator_terminates_and_float32_oracle_error", ()),
    ("test_gpu_loss_tail_regimes", "test_fixture_census_is_printed", ()),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 1, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 2, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (2, 1, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 3, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (3, 1, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (7, 9, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (4, 16, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (5, 13, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (127, 1, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (2, 64, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (3, 43, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (149, 7, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (32, 140, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (33, 140, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (10, 252, 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("nfg0", 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("allfg", 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("allignored", 3)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("lastfg", 3)),
    ("test_gpu_loss_tail_regimes", "test_scratch_is_ready_for_the_next_launch", (3,)),
    ("test_gpu_loss_tail_regimes", "test_iou_metrics_scratch_resets_between_launches", (3,)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 1, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 2, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (2, 1, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (1, 3, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (3, 1, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (7, 9, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (4, 16, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (5, 13, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (127, 1, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (2, 64, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (3, 43, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (149, 7, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (32, 140, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (33, 140, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_regimes", (10, 252, 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("nfg0", 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("allfg", 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("allignored", 10)),
    ("test_gpu_loss_tail_regimes", "test_loss_tail_label_extremes", ("lastfg", 10)),
    ("test_gpu_loss_tail_regimes", "test_scratch_is_ready_for_the_next_launch", (10,)),
    ("test_gpu_loss_tail_regimes", "test_iou_metrics_scratch_resets_between_launches", (10,)),
    ("test_gpu_box_edges", "test_iou_family_closed_forms_hold_for_the_oracle", ()),
    ("test_gpu_box_edges", "test_iou_pair_families_at_depth", ()),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 1, 3, 64)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 255, 3, 64)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 256, 3, 64)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 257, 3, 64)),
    ("test_gpu_box_edges", "test_decode_shapes", (3, 700, 3, 64)),
    ("test_gpu_box_edges", "test_decode_ties_and_selection_branches", (3, 64)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 1, 10, 128)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 255, 10, 128)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 256, 10, 128)),
    ("test_gpu_box_edges", "test_decode_shapes", (1, 257, 10, 128)),
    ("test_gpu_box_edges", "test_decode_shapes", (3, 700, 10, 128)),
    ("test_gpu_box_edges", "test_decode_ties_and_selection_branches", (10, 128)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("small_r16",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("r1_novalid",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("r300_n1000",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("r300_novalid",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("r1024_n4096_4097",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("r1024_novalid_4096",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("topk_1",)),
    ("test_gpu_box_edges", "test_nms_sizes_ties_and_units", ("topk_below_kept",)),
    ("test_gpu_box_edges", "test_nms_duplicates_and_tie_order", ()),
    ("test_gpu_box_edges", "test_fast_nms_equals_cube_nms", ()),
    # the fused front off the fixture shapes and at its limits: every case of the module
    ("test_gpu_front_edges", "test_front_edge_case", ("nolds",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("lds_edge",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("big_l",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("big_b",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("fits",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("idx16",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("one_a",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("one_b",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("k_max",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("eight",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("single",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("all_empty",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("tile_edge",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("running",)),
    ("test_gpu_front_edges", "test_front_edge_case", ("frozen",)),
    ("test_gpu_front_edges", "test_phased_front_edge_case", ("big_b",)),
    ("test_gpu_front_edges", "test_phased_front_edge_case", ("eight",)),
    ("test_gpu_front_edges", "test_largest_accepted_window_count", ()),
    ("test_gpu_front_edges", "test_refusals_return_their_code_and_launch_nothing", ()),
]

# the batch-builder kernels off their fixtures: every case of the module (the case names come from tests/inputs_cases.py)
import inputs_cases  # noqa: E402

CASES += [("test_gpu_inputs_edges", "test_refine_case", (n,)) for n in inputs_cases.REFINE_CASES]
CASES += [("test_gpu_inputs_edges", "test_first_stage_case", (n,)) for n in inputs_cases.KITTI_CASES]
CASES += [("test_gpu_inputs_edges", "test_sunrgbd_matrix", (n,)) for n in inputs_cases.SUNRGBD_CASES]
CASES += [
    ("test_gpu_inputs_edges", "test_refine_inference_form", ()),
    ("test_gpu_inputs_edges", "test_refine_every_element_written", ("fallback_last_padded-off",)),
    ("test_gpu_inputs_edges", "test_refine_every_element_written", ("fallback_last_padded-on",)),
    ("test_gpu_inputs_edges", "test_kitti_infer_entry", ()),
    ("test_gpu_inputs_edges", "test_refusals_leave_the_outputs_alone", ("fcn_prepare_inputs",)),
    ("test_gpu_inputs_edges", "test_refusals_leave_the_outputs_alone", ("fcn_prepare_inputs_infer",)),
    ("test_gpu_inputs_edges", "test_refusals_leave_the_outputs_alone", ("fcn_prepare_inputs_sunrgbd",)),
    ("test_gpu_inputs_edges", "test_refusals_leave_the_outputs_alone", ("fcn_prepare_inputs_refine",)),
    ("test_gpu_inputs_edges", "test_refusals_leave_the_outputs_alone", ("fcn_prepare_inputs_sunrgbd_infer",)),
    ("test_gpu_inputs_edges", "test_sunrgbd_infer_entry", ()),
]
for _path in ("build", "build_infer", "build_device", "build_device_train"):
    CASES += [("test_gpu_inputs_edges", "test_a_sample_without_a_window_is_refused", (_path, (1.6, -0.3, 0.0), 1, "-0.3")),
              ("test_gpu_inputs_edges", "test_a_sample_without_a_window_is_refused", (_path, (1.6, 0.9, float("nan")), 2, "nan"))]

# the optimiser entries and FlatTrainState on a toy module against the fp64 restatement (tests/optim_ref.py): every case of the
# module but the captured-graph one (replay cannot be emulated)
import optim_ref  # noqa: E402

CASES += [("test_gpu_optim", "test_adam_entry_one_step_at_a_time", (n,)) for n in optim_ref.SIZES]
CASES += [("test_gpu_optim", "test_sgd_entry_one_step_at_a_time", (n,)) for n in optim_ref.SIZES]
CASES += [
    ("test_gpu_optim", "test_adam_entry_refusals_touch_nothing", ()),
    ("test_gpu_optim", "test_sgd_entry_refusals_touch_nothing", ()),
    ("test_gpu_optim", "test_toy_layout", ()),
    ("test_gpu_optim", "test_parameter_in_a_scale_tile_is_refused", ()),
    ("test_gpu_optim", "test_toy_twins_whole_bucket_and_scale_steps", ("adam",)),
    ("test_gpu_optim", "test_toy_twins_whole_bucket_and_scale_steps", ("sgd",)),
    ("test_gpu_optim", "test_toy_world_of_eight_applies_one_eighth", ()),
    ("test_gpu_optim", "test_toy_state_transfer", ("adam",)),
    ("test_gpu_optim", "test_toy_state_transfer", ("sgd",)),
]

# the ConvFeatNet kernels layer by layer off the fixture shapes (tests/fcn_ref.py): every case of the module
import fcn_ref  # noqa: E402

for _fn, _cases in (("test_train_case", fcn_ref.TRAIN_CASES), ("test_sentinel_rows", fcn_ref.SENTINEL_CASES),
                    ("test_widths", fcn_ref.WIDTH_CASES), ("test_modes", fcn_ref.MODE_CASES)):
    CASES += [("test_gpu_fcn_layers", _fn, (c.name, p)) for c in _cases for p in (fcn_ref.SPLIT, fcn_ref.F32)]
CASES += [
    ("test_gpu_fcn_layers", "test_second_run_on_the_same_workspace_is_bit_identical", ("plain_3x33",)),
    ("test_gpu_fcn_layers", "test_second_run_on_the_same_workspace_is_bit_identical", ("base3_57x9",)),
    ("test_gpu_fcn_layers", "test_prepacked_forward_is_bit_identical_to_the_inline_pack", ("plain_3x33",)),
    ("test_gpu_fcn_layers", "test_prepacked_forward_is_bit_identical_to_the_inline_pack", ("frozen_base3_57x9",)),
    ("test_gpu_fcn_layers", "test_running_logits_do_not_depend_on_the_rest_of_the_batch", (fcn_ref.SPLIT,)),
    ("test_gpu_fcn_layers", "test_running_logits_do_not_depend_on_the_rest_of_the_batch", (fcn_ref.F32,)),
    ("test_gpu_fcn_layers", "test_refusals_return_their_code_and_write_nothing", ()),
]


def _ident(c):
    a = c[2]
    if a and isinstance(a[0], tuple):
        a = a[0]
    return ("%s-%s" % (c[1][5:], "_".join(str(x) for x in a)))[:72].replace(" ", "")


@pytest.mark.parametrize("mod,fn,args", CASES, ids=[_ident(c) for c in CASES])
def test_gpu_test_under_emulation(mod, fn, args):
    from emu_shim import emulated_gpu
    m = importlib.import_module(mod)
    with emulated_gpu():
        getattr(m, fn)(*args)
