"""Frozen BatchNorm (FCN_BN_FROZEN) on the CPU: test functions of tests/test_gpu_frozen_bn.py run against the host emulation of the
kernels (tests/emu_shim.py + tests/host_harness: the .hip sources compiled unmodified for the CPU) -- the whole frozen model (PointNet
scales, fused ConvFeatNet forward and backward, loss tail) against the fp64 oracle with running statistics, one PointNet scale
through the key-pooled and the row-pooled forward, the reference-shaped module API and the C-ABI mode contract.  This pins the
index arithmetic and the roles of the frozen coefficients before any GPU time is spent; the hardware run stays the gate.  (Not
here: graph capture and the three-stream backward, which the emulation cannot run.)"""
import importlib
import os
import shutil

import pytest

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")

CASES = [
    ("test_frozen_model_matches_oracle", ("car_b4_n512",), False),
    ("test_mixed_frozen_and_training_parts", ("conv",), True),
    ("test_frozen_key_pool_backward_with_zero_and_negative_gamma", (), True),
    ("test_frozen_dense_module_api_matches_oracle", (1, 0.25, 32), False),
    ("test_frozen_modes_agree", (), False),
    ("test_c_abi_bn_modes", (), False),
]


@pytest.mark.parametrize("fn,args,f32", CASES, ids=[c[0][5:] for c in CASES])
def test_frozen_bn_under_emulation(fn, args, f32, monkeypatch):
    from emu_shim import emulated_gpu
    from frustum_convnet_amd import precision
    monkeypatch.setenv("FCN_EMULATE", "1")          # (the tests leave out what the emulation cannot run)
    m = importlib.import_module("test_gpu_frozen_bn")
    with emulated_gpu():
        if f32:
            with precision.precision("f32"):
                getattr(m, fn)(*args, None)
        else:
            getattr(m, fn)(*args)
