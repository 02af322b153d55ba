"""The decode-rule, corner, matching and AP cases of the -m gpu suite (tests/test_gpu_sunrgbd_detect.py, tests/test_gpu_det_eval.py),
run on the CPU: the SAME test functions with the package's GPU-only Python layer pointed at the host emulation of the kernels
(tests/emu_shim.py + tests/host_harness), in the style of tests/test_emu_gpu_subset.py.  The hardware run stays the parity gate;
this tier catches index / reduction / barrier mistakes of csrc/det_eval.h and of the decode kernel's second instantiation without a
GPU.  Not here: the whole-model cases (run time, no new kernel path) and the refusal of CPU tensors (inside the shim it cannot
tell)."""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_gpu_sunrgbd_detect", "test_decode_rule_matches_the_fixture_and_the_restatement", (5, 69)),
    ("test_gpu_sunrgbd_detect", "test_decode_rule_matches_the_fixture_and_the_restatement", (5, 128)),
    ("test_gpu_sunrgbd_detect", "test_decode_rule_matches_the_fixture_and_the_restatement", (300, 69)),
    ("test_gpu_sunrgbd_detect", "test_decode_rule_matches_the_fixture_and_the_restatement", (300, 128)),
    ("test_gpu_sunrgbd_detect", "test_the_kitti_rule_on_the_same_inputs_differs_and_is_the_old_entry", ()),
    ("test_gpu_sunrgbd_detect", "test_decode_refusals_write_nothing", ()),
    ("test_gpu_sunrgbd_detect", "test_corners_of_kept_rows", ()),
    ("test_gpu_det_eval", "test_matcher_and_ap_reproduce_the_references_recorded_run", ()),
    ("test_gpu_det_eval", "test_group_and_class_sizes_by_construction", ()),
    ("test_gpu_det_eval", "test_equal_scores_rank_the_lower_index_first", ()),
    ("test_gpu_det_eval", "test_raw_entries_poisoned_outputs_and_refusals", ()),
]


def _ident(c):
    return ("%s-%s" % (c[1][5:], "_".join(str(x) for x in c[2])))[:72]


@pytest.mark.parametrize("mod,fn,args", CASES, ids=[_ident(c) for c in CASES])
def test_gpu_test_under_emulation(mod, fn, args):
    from emu_shim import emulated_gpu
    m = importlib.import_module(mod)
    with emulated_gpu():
        getattr(m, fn)(*args)
