"""The -m gpu tests of capturable SUN-RGBD inference (tests/test_gpu_sunrgbd_detect_source.py), run on the CPU: the SAME test
functions with the package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py +
tests/host_harness).  The emulated library exports fcn_frustum_sunrgbd_detect_count / _plan / _fill and fcn_det_rows like every other
entry point (csrc/frustum_sunrgbd_detect_plan.h is included from inputs.hip, csrc/det_eval.h from box_iou.hip).  Left out: the two
tests that need a real graph capture.  The hardware run stays the gate; this tier catches index, order and bounds mistakes in the
kernels, in SunrgbdDetectSource and in SunrgbdFrameChain without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_plan_box_count_ranges_and_slots", (c,))
         for c in ("n_boxes_0", "n_boxes_D", "n_boxes_D_plus_1", "n_boxes_negative", "frame_minus_1", "frame_F", "class_minus_1", "class_C",
                   "exactly_B", "B_plus_1", "no_survivor")]
CASES += [("test_plan_knife_edges", ())]
CASES += [("test_plans_where_a_threads_run_goes_from_one_box_to_two", (D, S)) for D in (255, 256, 257) for S in (1, 3)]
CASES += [("test_plan_at_its_limits_and_refusals", ())]
CASES += [("test_selection_equals_the_reading_selection_byte_for_byte", (stride,)) for stride in (4, 6)]
CASES += [("test_count_plan_fill_on_frames_of_4096_4097_and_0_rows", ())]
CASES += [("test_det_rows_equals_the_restatement", gk) for gk in ((1, 6), (255, 3), (256, 3), (257, 3), (40, 1), (7, 300))]
CASES += [
    ("test_det_rows_refusals", ()),
    ("test_alloc_infer_and_launch_infer_equal_build_device", ()),
    ("test_source_equals_the_existing_path_and_the_recorded_run", ()),
    ("test_source_with_empty_slots", ()),
    ("test_source_check_names_the_bits_and_clears", ()),
    ("test_source_refusals", ()),
    ("test_frame_chain_equals_detect_frames_and_evaluates_alike", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_sunrgbd_detect_source_under_emulation(fn, args):
    import test_gpu_sunrgbd_detect_source as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
