"""CPU: the epoch sampler (fcn_epoch_pick / fcn_epoch_pick_limits, csrc/epoch_pick.h) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a STAND-ALONE host program: tests/host_harness/epoch_pick_main.cpp + csrc/inputs.hip compiled for the
host against the HIP stand-in of tests/host_harness/hip_emu, exactly as tests/test_draws_sanitizer.py builds its program.  Every
buffer the program hands in is exactly sized -- count one word, state two, pick D -- so a pick written past D or a state word read
past the second is reported.  The program also runs the kernel instantiated with 2-bit digits and 64 composites of LDS at G up to
5000, which drives both boundary walks of the rank-window select many digits deep, and compares every window of two epochs with a
plain std::sort.  (Leak checking is off: the emulation keeps its worker threads and their coroutine stacks for the life of the
process.)"""
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
    shutil.copy(os.path.join(HERE, "host_harness", "epoch_pick_main.cpp"), tmp_path)
    exe = str(tmp_path / "epoch_pick_asan")
    # the program includes csrc/epoch_pick.h through the copy's root, so both translation units see the same text
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-mf16c", "-pthread", "-ffp-contract=off", "-w",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(HERE, "host_harness", "hip_emu"), "-I", str(tmp_path),
           str(src / "inputs.hip"), str(tmp_path / "epoch_pick_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", FCN_EMU_THREADS="2")
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "all ok" in p.stdout and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
