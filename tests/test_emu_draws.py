"""The kernel-level cases of tests/test_gpu_draws.py run on the CPU: the SAME test functions with the package's GPU-only Python
layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness), in the style of
tests/test_emu_kitti_eval.py.  The hardware run stays the parity gate; this tier catches index, histogram, compaction and barrier
mistakes of csrc/draws.h without a GPU (the host's libm stands in for the device's log / sqrt / cos: the 1e-12 bar on `normal` is
the hardware run's to hold).  Not here: the graph capture (the emulation runs every launch at once), the three public builders
(their scenes are other kernels' run time) and the refusal of CPU tensors (inside the shim it cannot tell)."""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_mixed_rows_in_one_launch_match_the_restatement", (N,)) for N in (1, 4, 8, 1024, 2048)] + [
    ("test_single_rows_match_the_restatement", ()),
    ("test_flags_off_write_the_constants", ()),
    ("test_state_advances_and_restoring_it_reproduces_the_draw", ()),
] + [("test_steps_at_and_above_two_to_the_32", (s,)) for s in (2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 62 - 2)] + [
    ("test_rows_without_a_point_are_zeroed_and_flagged", ()),
    ("test_composition_through_a_packed_subsample", ()),
    ("test_refusals_of_the_entry_and_of_the_wrapper", ()),
]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:40], "_".join(str(a) for a in c[1])) for c in CASES])
def test_gpu_test_under_emulation(fn, args):
    from emu_shim import emulated_gpu
    m = importlib.import_module("test_gpu_draws")
    with emulated_gpu():
        getattr(m, fn)(*args)
