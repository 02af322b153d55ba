"""The -m gpu tests of the refinement stage's training link (tests/test_gpu_refine_label.py), run on the CPU: the SAME test
functions with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py +
tests/host_harness).  The emulated library exports fcn_refine_match and fcn_refine_label_count / _fill like every other entry point
(csrc/refine_label.h is included from inputs.hip), so _native.lib() binds them as it stands.  The hardware run stays the gate; this
tier catches index, order and bounds mistakes in the three kernels and in the host code around them without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_entry_points_match_the_referee", (3,)),
    ("test_entry_points_match_the_referee", (4,)),
    ("test_entry_points_match_the_referee", (5,)),
    ("test_entry_points_match_the_referee", ("unaligned4",)),
    ("test_count_and_fill_over_the_frame_lengths_the_scan_turns_on", (3,)),
    ("test_count_and_fill_over_the_frame_lengths_the_scan_turns_on", (4,)),
    ("test_count_and_fill_over_the_frame_lengths_the_scan_turns_on", (5,)),
    ("test_one_copy_without_jitter_equals_the_unlabelled_selection", ()),
    ("test_copies_chain_as_the_references_do", ()),
    ("test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside", ()),
    ("test_slices_bound_the_stores", ()),
    ("test_rejected_units_take_no_room", ()),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("row_high",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("row_negative",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("frame_high",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("frame_negative",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("gt_high",)),
    ("test_bad_arguments_are_refused_with_nothing_written", ()),
    ("test_empty_results_launch_nothing_behind_them", ()),
    ("test_label_boxes_as_their_own_candidates", ()),
    ("test_build_device_train_equals_build_on_host_records", ()),
    ("test_draw_box3d_jitter_reproduces_the_references_draws", ()),
    ("test_one_training_step_on_the_device_built_batch", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_refine_label_under_emulation(fn, args):
    import test_gpu_refine_label as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
