"""The -m gpu tests of the capturable two-stage inference link (tests/test_gpu_cascade_plan.py), run on the CPU: the SAME test
functions with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py +
tests/host_harness).  The emulated library exports fcn_cascade_candidates and fcn_refine_detect_count / _plan / _fill like every
other entry point (csrc/cascade_plan.h is included from inputs.hip).  Left out: the test that needs a real graph capture.  The
hardware run stays the gate; this tier catches index, order and bounds mistakes in the kernels and in CascadeLink without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_candidates_equal_the_restatement", (c,))
         for c in ("one_group", "empty_group", "overflowed_group", "count_beyond_top_k", "exactly_D", "D_plus_one", "D_is_one",
                   "entries_out_of_range", "many_groups", "at_the_limits")]
CASES += [("test_segmented_selection_equals_the_reading_selection_bit_for_bit", (stride,)) for stride in (4, 5)]
CASES += [("test_segmented_selection_over_the_frame_lengths_the_scan_turns_on", (stride, S)) for stride in (4, 5) for S in (1, 2, 3)]
CASES += [("test_out_of_range_candidate_is_skipped_silently_and_never_dereferenced", (w,))
          for w in ("row_high", "row_negative", "frame_high", "frame_negative")]
CASES += [
    ("test_plan_equals_the_restatement", (4,)),
    ("test_plan_equals_the_restatement", (10,)),
    ("test_plan_equals_the_restatement", (12,)),
    *[("test_plan_where_a_threads_run_goes_from_one_candidate_to_two", (D, S)) for D in (255, 256, 257) for S in (1, 3)],
    ("test_plan_at_its_smallest_and_at_its_limits", ()),
    ("test_plan_widths", ()),
    ("test_count_plan_fill_stays_within_capacity_plus_one_rows", ()),
    ("test_step_equals_the_existing_path_on_the_same_first_stage_output", ()),
    ("test_a_first_stage_that_keeps_nothing", ()),
    ("test_constructor_refusals", ()),
    ("test_entry_refusals_write_nothing", ()),
    ("test_check_raises_names_the_bits_and_clears", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_cascade_plan_under_emulation(fn, args):
    import test_gpu_cascade_plan as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
