"""The kernel-level cases of tests/test_gpu_kitti_eval.py run on the CPU: the SAME test functions with the package's GPU-only
Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness), in the style of
tests/test_emu_det_eval.py.  The hardware run stays the parity gate; this tier catches index / reduction / barrier mistakes of
csrc/kitti_eval.h without a GPU.  Not here: the whole-model case (run time, no new kernel path), the 200-true-positive scene (run
time) and the refusal of CPU tensors (inside the shim it cannot tell)."""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_scene_matches_the_referee", (name,)) for name in ("mixed", "single", "no_cyclist", "alpha10", "tp1", "tp40", "tp41", "perfect", "hand1", "hand_trunc", "hand_ignored")] + [
    ("test_overlaps_at_60_m_depth", ()),
    ("test_classes_argument_leaves_the_others_out", ()),
    ("test_label_rows_match_the_golden_file_and_the_restatement", ()),
    ("test_raw_entries_poisoned_outputs_and_refusals", ()),
    ("test_kitti_results_on_a_hand_built_detect_frames_dict", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:40], "_".join(c[1])) for c in CASES])
def test_gpu_test_under_emulation(fn, args):
    from emu_shim import emulated_gpu
    m = importlib.import_module("test_gpu_kitti_eval")
    with emulated_gpu():
        getattr(m, fn)(*args)
