"""The -m gpu test of the shared detection table (tests/test_resident_tables.py), run on the CPU: the SAME test function with the
package's GPU-only Python layer pointed at the host emulation of the kernels (tests/emu_shim.py + tests/host_harness).  The hardware
run stays the gate; this tier catches a table that set_boxes fills wrongly, or a plan that reads behind n_boxes, without a GPU."""
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [("test_set_boxes_fills_the_table_and_the_plan_ignores_stale_rows", (which,)) for which in ("kitti", "sunrgbd")]


@pytest.mark.parametrize("fn,args", CASES, ids=["%s-%s" % (c[0][5:45], "_".join(str(a) for a in c[1])) for c in CASES])
def test_resident_tables_under_emulation(fn, args):
    import test_resident_tables as m
    from emu_shim import emulated_gpu
    with emulated_gpu():
        getattr(m, fn)(*args)
