"""The -m gpu tests of the capturable first-stage training input (tests/test_gpu_frustum_plan.py), run on the CPU: the SAME test
functions with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py +
tests/host_harness).  The emulated library exports fcn_box2d_perturb and fcn_frustum_train_count / _plan / _fill like every other
entry point (csrc/frustum_plan.h is included from inputs.hip).  Left out: the two tests that need a real graph capture.  The
hardware run stays the gate; this tier catches index, order and bounds mistakes in the kernels and in FrameTrainSource without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_perturb_equals_the_restatement_bit_for_bit", (1, 0)),
    ("test_perturb_equals_the_restatement_bit_for_bit", (1, 1)),
    ("test_perturb_equals_the_restatement_bit_for_bit", (1, 2 ** 32 + 5)),
    ("test_perturb_equals_the_restatement_bit_for_bit", (300, 0)),
    ("test_perturb_equals_the_restatement_bit_for_bit", (300, 1)),
    ("test_perturb_equals_the_restatement_bit_for_bit", (300, 2 ** 32 + 5)),
    ("test_perturb_failures_are_flagged_and_copy_the_input", ()),
    ("test_plan_equals_the_restatement", (4,)),
    ("test_plan_equals_the_restatement", (12,)),
    ("test_plan_at_its_smallest_and_over_many_boxes", ()),
    *[("test_plan_where_a_threads_run_goes_from_one_box_to_two", (D, S)) for D in (255, 256, 257) for S in (1, 3)],
    ("test_no_read_count_and_fill_equal_the_label_entries_bit_for_bit", (4,)),
    ("test_no_read_count_and_fill_equal_the_label_entries_bit_for_bit", (5,)),
    ("test_step_equals_the_existing_path_on_the_same_boxes", (4, 4)),
    ("test_step_equals_the_existing_path_on_the_same_boxes", (12, 4)),
    ("test_step_equals_the_existing_path_on_the_same_boxes", (4, 5)),
    ("test_overflow_is_truncated_flagged_and_stays_in_bounds", ()),
    ("test_step_reproduces_the_references_recorded_run", ()),
    ("test_one_training_step_on_a_step_batch", ()),
    ("test_constructor_refusals", ()),
    ("test_entry_refusals_write_nothing", ()),
    ("test_check_raises_names_the_bits_and_clears", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_frustum_plan_under_emulation(fn, args):
    import test_gpu_frustum_plan as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
