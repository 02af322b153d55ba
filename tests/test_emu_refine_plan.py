"""The -m gpu tests of the capturable refine-stage training input (tests/test_gpu_refine_plan.py), run on the CPU: the SAME test
functions with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py +
tests/host_harness).  The emulated library exports fcn_box3d_jitter_draw and fcn_refine_train_match / _count / _plan / _fill like
every other entry point (csrc/refine_plan.h is included from inputs.hip).  Left out: the test that needs a real graph capture.  The
hardware run stays the gate; this tier catches index, order and bounds mistakes in the kernels and in RefineTrainSource without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_jitter_draw_equals_the_restatement_bit_for_bit", (D, A, step))
         for D, A in ((1, 1), (1, 64), (300, 3)) for step in (0, 1, 2 ** 32 + 5)]
CASES += [
    ("test_plan_equals_the_restatement", (4,)),
    ("test_plan_equals_the_restatement", (10,)),
    ("test_plan_equals_the_restatement", (12,)),
    *[("test_plan_where_a_threads_run_goes_from_one_unit_to_two", (U, S)) for U in (255, 256, 257) for S in (1, 3)],
    ("test_plan_at_its_smallest_and_at_its_limits", ()),
    ("test_plan_widths", ()),
    ("test_no_read_entries_equal_the_reading_entries_bit_for_bit", (4,)),
    ("test_no_read_entries_equal_the_reading_entries_bit_for_bit", (5,)),
]
CASES += [("test_out_of_range_candidate_is_skipped_silently_and_never_dereferenced", (w,))
          for w in ("row_high", "row_negative", "frame_high", "frame_negative", "gt_high")]
CASES += [("test_step_equals_the_existing_path_on_the_same_boxes", (rel, stride)) for stride in (4, 5) for rel in (-3, 0, 4)]
CASES += [
    ("test_step_reproduces_the_references_recorded_run", ()),
    ("test_overflow_is_truncated_flagged_and_stays_in_bounds", ()),
    ("test_one_training_step_on_a_step_batch", ()),
    ("test_constructor_refusals", ()),
    ("test_entry_refusals_write_nothing", ()),
    ("test_check_raises_names_the_bits_and_clears", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_refine_plan_under_emulation(fn, args):
    import test_gpu_refine_plan as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
