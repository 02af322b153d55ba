"""The -m gpu tests of the cascade link (tests/test_gpu_cascade.py), run on the CPU: the SAME test functions with the package's
GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness).  The emulated
library exports fcn_refine_select_count / _fill like every other entry point (csrc/refine_select.h is included from
inputs.hip), so _native.lib() binds them as it stands.  The hardware run stays the gate; this tier catches index, order and
bounds mistakes in the two kernels and in the host code around them without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_select_entry_points_match_the_referee", (3,)),
    ("test_select_entry_points_match_the_referee", (4,)),
    ("test_select_rows_that_are_not_16_byte_aligned", ()),
    ("test_select_nothing_to_do_and_bad_arguments", ()),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("frame_high",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("frame_negative",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("row_high",)),
    ("test_out_of_range_candidate_is_reported_and_never_dereferenced", ("row_negative",)),
    ("test_fill_never_writes_past_a_candidates_slice", ()),
    ("test_select_over_the_frame_lengths_the_scan_turns_on", (3,)),
    ("test_select_over_the_frame_lengths_the_scan_turns_on", (4,)),
    ("test_select_over_the_frame_lengths_the_scan_turns_on", (5,)),
    ("test_build_device_equals_build_on_host_records", ()),
    ("test_two_stage_detector_equals_the_hand_composed_sequence", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_cascade_under_emulation(fn, args):
    import test_gpu_cascade as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
