"""The -m gpu tests of the SUN-RGBD frustum extraction (tests/test_gpu_frustum_sunrgbd.py), run on the CPU: the SAME test functions
with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness).
The emulated library exports fcn_frustum_sunrgbd_count / _fill / _label_count / _label_fill, fcn_frustum_subset_pos and
fcn_prepare_inputs_sunrgbd_infer like every other entry point (csrc/frustum_sunrgbd.h is included from inputs.hip), so
_native.lib() binds them as it stands.  The hardware run stays the gate; this tier catches index, order and bounds mistakes in the
kernels and in the host code around them without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_entry_points_match_the_referee", (3,)),
    ("test_entry_points_match_the_referee", (5,)),
    ("test_entry_points_match_the_referee", (6,)),
    ("test_entry_points_match_the_referee", (7,)),
    ("test_entry_points_match_the_referee", (4,)),
    ("test_entry_points_match_the_referee", ("4+4",)),
    ("test_entry_points_match_the_referee", ("4+8",)),
    ("test_entry_points_match_the_referee", ("6+4",)),
    ("test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside", ()),
    ("test_slices_bound_both_stores", ()),
    ("test_bad_arguments_are_refused_with_nothing_written", ()),
    ("test_out_of_range_box_frame_is_reported_and_never_dereferenced", ("frame_high",)),
    ("test_out_of_range_box_frame_is_reported_and_never_dereferenced", ("frame_negative",)),
    ("test_subset_pos_equals_numpy", ()),
    ("test_training_candidates_equal_the_references_recorded_run", ()),
    ("test_candidates_equal_the_references_recorded_run", ()),
    ("test_build_device_train_equals_the_loaders_batch_and_build", ()),
    ("test_build_device_equals_the_loaders_batch", ()),
    ("test_one_training_step_on_the_device_built_batch", ()),
    ("test_empty_results_launch_nothing_behind_them", ()),
    ("test_infer_entry_point_refuses_bad_arguments", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_frustum_sunrgbd_under_emulation(fn, args):
    import test_gpu_frustum_sunrgbd as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
