"""The -m gpu tests of the labelled frustum extraction (tests/test_gpu_frustum_label.py), run on the CPU: the SAME test functions
with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness).
The emulated library exports fcn_frustum_label_count / _fill like every other entry point (csrc/frustum_label.h is included from
inputs.hip), so _native.lib() binds them as it stands.  The hardware run stays the gate; this tier catches index, order and bounds
mistakes in the two kernels and in the host code around them without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_label_entry_points_match_the_referee", (3,)),
    ("test_label_entry_points_match_the_referee", (4,)),
    ("test_label_entry_points_match_the_referee", (5,)),
    ("test_label_rows_that_are_not_16_byte_aligned", ()),
    ("test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside", ()),
    ("test_slices_bound_both_stores", ()),
    ("test_label_bad_arguments_are_refused_with_nothing_written", ()),
    ("test_out_of_range_box_frame_is_reported_and_never_dereferenced", ("frame_high",)),
    ("test_out_of_range_box_frame_is_reported_and_never_dereferenced", ("frame_negative",)),
    ("test_training_candidates_equal_the_references_recorded_run", ()),
    ("test_build_device_train_equals_build_on_host_records", ()),
    ("test_one_training_step_on_the_device_built_batch", ()),
    ("test_empty_results_launch_nothing_behind_them", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_frustum_label_under_emulation(fn, args):
    import test_gpu_frustum_label as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
