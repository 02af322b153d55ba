"""CPU: the entry points of capturable SUN-RGBD inference (fcn_frustum_sunrgbd_detect_count / _plan / _fill, fcn_det_rows) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a STAND-ALONE host program: tests/host_harness/sunrgbd_detect_main.cpp +
csrc/inputs.hip and csrc/box_iou.hip (the tail lives in csrc/det_eval.h) compiled for the host against the HIP stand-in of
tests/host_harness/hip_emu, exactly as tests/test_frustum_detect_sanitizer.py builds its program.  Every buffer the program hands in is
exactly sized, so a plan that reads the box table at or beyond n_boxes' overflow, a count or a box past its inputs or writes past its
outputs, a kernel that dereferences a box whose frame or class is out of range or that is not live, a fill that stores into the spare
row or past the capacity + 1 rows the plan's clamp promises, a subsample draw that writes past sub_off[B] entries, or a tail that reads
a detection at or beyond num_dets, is reported.  (Leak checking is off: the emulation keeps its worker threads and their coroutine
stacks for the life of the process.)"""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")


def test_entry_points_are_clean_under_asan_and_ubsan(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "host_harness"))
    import build_emu
    # a private copy of the kernel sources with the emulation's two mechanical substitutions (build_emu.PATCHES)
    src = tmp_path / "frustum_convnet_amd" / "csrc"
    src.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "fcn_hip.h"), tmp_path / "include")
    for f in os.listdir(build_emu.CSRC):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(build_emu.CSRC, f)).read()
            for pat, rep in build_emu.PATCHES:
                text = pat.sub(rep, text)
            (src / f).write_text(text)
    src = str(src)
    exe = str(tmp_path / "sunrgbd_detect_asan")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-mf16c", "-pthread", "-ffp-contract=off", "-w",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(HERE, "host_harness", "hip_emu"), "-I", ROOT,
           os.path.join(src, "inputs.hip"), os.path.join(src, "box_iou.hip"), os.path.join(HERE, "host_harness", "sunrgbd_detect_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", FCN_EMU_THREADS="2")
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "all ok" in p.stdout and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
