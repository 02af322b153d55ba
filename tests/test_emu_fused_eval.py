"""The single-launch inference forward (fuse_eval) on the CPU: test functions of tests/test_gpu_fused_eval.py run against the host
emulation of the kernels (tests/emu_shim.py + tests/host_harness: the .hip sources compiled unmodified for the CPU) -- one scale
against the fp64 oracle on small shapes of all three kernel instantiations, the exact properties (without the graph capture, which
the emulation cannot run), side effects, modes and fallbacks, the C-ABI contract; and once more under the guard-page audit.  This
pins the index arithmetic, the LDS choreography and the cross-tile pooling before any GPU time is spent; the hardware run stays the
gate."""
import importlib
import os
import shutil
import subprocess
import sys

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")


def _cases():
    import test_gpu_fused_eval as m
    out = [("test_one_scale_vs_fp64_oracle", (c, p)) for c in m.SMALL_CASES for p in ("split", "bf16")]
    out += [(fn, ()) for fn in ("test_empty_windows_and_repeatability", "test_layouts_are_transposes_with_one_hot_rows",
                                "test_no_side_effects_and_new_weights_are_used", "test_training_and_frozen_modes_ignore_the_flag",
                                "test_f32_precision_takes_the_layered_path", "test_c_abi_contract")]
    return out


def _id(c):
    fn, args = c
    return fn[5:] + ("" if not args else "-%s-%s" % (args[0][0], args[1]))


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_fused_eval_under_emulation(case, monkeypatch):
    from emu_shim import emulated_gpu
    fn, args = case
    monkeypatch.setenv("FCN_EMULATE", "1")          # (the tests pick their small shapes and leave out what the emulation cannot run)
    m = importlib.import_module("test_gpu_fused_eval")
    with emulated_gpu():
        getattr(m, fn)(*args)


def test_prefetched_front_under_emulation(monkeypatch):
    """The whole-model front (PointNetFeat: prefetch, fused front, all four scales) on the smallest fixture."""
    from emu_shim import emulated_gpu
    monkeypatch.setenv("FCN_EMULATE", "1")
    m = importlib.import_module("test_gpu_fused_eval")
    with emulated_gpu():
        m.test_prefetched_front_is_not_consumed_across_the_flag()


def test_fused_eval_under_the_guard_page_audit(tmp_path):
    """The emulated run once more with every tensor storage between two inaccessible pages (tests/host_harness/guard), guard behind
    and guard in front: an out-of-bounds access of the fold or infer kernel ends the child with a fault instead of passing."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = str(tmp_path / "libguard_malloc.so")
    # (the interposer is C: the host clang++ of the emulation build compiles it with -x c, so the audit needs no second compiler)
    subprocess.check_call([CLANG, "-x", "c", "-O2", "-shared", "-fPIC", os.path.join(here, "host_harness", "guard", "guard_malloc.c"),
                           "-o", lib, "-ldl", "-lpthread"])
    sel = "empty_windows or layouts or c_abi or small256-split or small64-bf16"
    old = os.environ.get("LD_PRELOAD", "")
    preload = lib + (":" + old if old else "")      # added in front of whatever is preloaded already, never instead of it
    for mode in ("", "front"):
        env = dict(os.environ, LD_PRELOAD=preload, FCN_EMULATE="1", FCN_GUARD_MODE=mode)
        r = subprocess.run([sys.executable, "-X", "faulthandler", "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                            os.path.join(here, "test_emu_fused_eval.py"), "-k", "under_emulation and (%s)" % sel],
                           env=env, cwd=os.path.dirname(here), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (mode, r.stdout[-3000:])
        assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]


def test_library_without_the_kernels_is_an_error_not_a_fallback(monkeypatch):
    """A loaded library that lacks fcn_pn_infer (an FCN_LIB_NAME build of older kernel sources) with the flag on: fused_eval_supported
    raises for a scale the kernel would take, and still answers False for the shapes and modes that keep the layered path."""
    from frustum_convnet_amd import _native, pointnet_fused as pf, precision
    monkeypatch.setattr(_native, "lib", lambda: object())
    split, f32 = precision.CODES["split"], precision.CODES["f32"]
    with pytest.raises(RuntimeError, match="fcn_pn_infer"):
        pf.fused_eval_supported(_native.BN_RUNNING, split, 128)
    assert pf.fused_eval_supported(_native.BN_RUNNING, f32, 128) is False
    assert pf.fused_eval_supported(_native.BN_TRAIN, split, 128) is False
    assert pf.fused_eval_supported(_native.BN_RUNNING, split, 512) is False
