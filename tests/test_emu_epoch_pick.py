"""The kernel-level cases of tests/test_gpu_epoch_pick.py run on the CPU: the SAME test functions with the package's GPU-only
Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness), in the style of
tests/test_emu_draws.py.  The hardware run stays the parity gate; this tier catches index, histogram, compaction and barrier mistakes
of csrc/epoch_pick.h without a GPU.  Not here: the graph capture (the emulation runs every launch at once) and the three training
sources (their scenes are other kernels' run time)."""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")


def _cases():
    m = importlib.import_module("test_gpu_epoch_pick")
    cases = [("test_limits_and_the_case_table", ())]
    cases += [("test_whole_epoch_and_the_first_turn_of_the_next", c) for c in m.WHOLE]
    cases += [("test_chosen_turns_of_a_large_epoch", c) for c in m.TURNS]
    cases += [("test_turn_zero_equals_the_draw_kernels_choice_row", c) for c in ((5, 2), (257, 16), (4096, 2048), (4097, 48), (70000, 2048), (70000, 1))]
    cases += [("test_epochs_at_and_above_two_to_the_32", (e,)) for e in (2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5)]
    cases += [("test_a_key_tie_inside_a_window_and_across_a_window_boundary", ())]
    cases += [("test_ranks_take_disjoint_windows_of_one_epoch", c) for c in ((1000, 16, 3), (5000, 48, 2), (4100, 2048, 2))]
    cases += [("test_state_restores_and_advance_zero_keeps_it", ())]
    cases += [("test_defined_failures_give_zeros_the_bit_and_the_state_as_it_was", f) for f in m.FAILURES]
    cases += [("test_refusals_of_the_entry_and_of_the_wrapper", ())]
    return cases


CASES = _cases()


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:40], "_".join(str(a).replace(" ", "_") for a in c[1])) for c in CASES])
def test_gpu_test_under_emulation(fn, args):
    from emu_shim import emulated_gpu
    m = importlib.import_module("test_gpu_epoch_pick")
    with emulated_gpu():
        getattr(m, fn)(*args)
