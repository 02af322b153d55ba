"""CPU referee of tests/fcn_ref.py: no kernel runs here.  It holds the REFERENCE of every case of tests/test_gpu_fcn_layers.py to the
conditions that keep a GPU failure from being the reference's fault:
  * a draw that keeps every BatchNorm output KINK_MIN from zero exists within MAX_DRAWS;
  * every BatchNorm of a BN_TRAIN case takes its statistics over at least MIN_BN_ROWS distinct rows (fewer is ill-conditioned: the
    kernels and the fp32 module alike are 15 % to 100 % off fp64 at B = 1, L = (9,5,3,2)); B = 1 with fewer appears in the
    BN_RUNNING / BN_FROZEN lists only, where no batch statistic is involved;
  * the cap: the fp32 evaluation of the same module on the same inputs is within CAP_GRAD (5e-5, half the exact-fp32 gradient bar) of
    the fp64 maximum on every gradient tensor and within CAP_LOGITS (1e-5) absolute on the logits -- a case that misses it gets more
    bases or another seed (fcn_ref.py says which have one), never a wider bar;
  * the layer order and arena totals restated in fcn_ref.plan() equal fcn_convnet_sizes of the emulated library.
It also prints the fp32 module's per-layer error, the number the per-layer bars of the kernels are 4 x of."""
import os
import shutil

import pytest
import torch

import fcn_ref as F
from frustum_convnet_amd import _native as N

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
NAMES = [c.name for c in F.ALL_CASES]
GRADS = ("dfeats", "dW", "dgamma", "dbeta", "dWh", "dbias")
LAYER = ("y", "mean", "rstd", "scale", "shift")


def test_case_lists_hold_what_they_should():
    for c in F.TRAIN_CASES + F.SENTINEL_CASES + F.WIDTH_CASES:
        assert c.mode == N.BN_TRAIN
    assert {c.mode for c in F.MODE_CASES} == {N.BN_RUNNING, N.BN_FROZEN}
    assert {c.nvec for c in F.WIDTH_CASES} | {3} == set(F.NVECS) and {c.reg_out for c in F.WIDTH_CASES} >= set(F.REG_OUTS)
    assert {(len(c.Ls), c.c1) for c in F.TRAIN_CASES} == {(4, 128), (4, 64), (5, 64), (5, 128)}
    for c in F.ALL_CASES:
        for j in range(1, len(c.Ls)):
            assert c.Ls[j] == (c.Ls[j - 1] + 1) // 2, c
    # the row counts the big cases exist for
    rows = {c.name: c.B * c.Ls[0] for c in F.TRAIN_CASES}
    assert rows["base3_57x9"] == 513 and rows["base3_58x9"] == 522 and rows["base3_40x33"] == 1320 and rows["base4_103x5"] == 515
    big5 = F.BY_NAME["base2_47x21_5lev"]
    assert big5.B * big5.Ls[0] > 512 and big5.B * big5.Ls[1] > 512
    # sentinel rows: the ones the L2 grid has, the last one among them
    assert F.sentinel_rows(F.BY_NAME["base3_57x9_rows"]) == [0, 31, 32, 159, 160, 284]
    assert F.sentinel_rows(F.BY_NAME["base3_40x33_rows"]) == [0, 31, 32, 255, 256, 511, 512, 679]
    for c in F.SENTINEL_CASES:                     # both sides of every boundary between two weight-gradient splits of the heads
        starts = F.heads_split_starts(c)
        assert len(starts) >= 2 and all(s - 1 in F.sentinel_rows(c) and s in F.sentinel_rows(c) for s in starts[1:]), (c.name, starts)
    # the one-hot width cases make the last column, the first and both sides of the segment's middle hot
    for c in F.WIDTH_CASES:
        if c.nvec > 3:
            assert len(c.hot) == c.B and {c.nvec - 1, 0, c.nvec // 2, c.nvec // 2 - 1} <= set(c.hot), c
    assert {31, 32, 63} <= set(F.BY_NAME["nvec64"].hot)


@pytest.mark.parametrize("name", [c.name for c in F.ALL_CASES if c.nbase])
def test_slot_map_uses_every_base_and_mixes_neighbours(name):
    c = F.BY_NAME[name]
    m = F.slot_map(c)
    assert m.shape == (c.B,) and set(m.tolist()) == set(range(c.nbase))
    assert torch.equal(m, F.slot_map(c))                                    # fixed per case
    differ = float((m[1:] != m[:-1]).float().mean())
    assert differ >= 0.35, differ                                           # (1 - 1 / nbase on average; 0.35: two bases, 46 pairs)


@pytest.mark.parametrize("name", NAMES)
def test_reference_supports_the_case(name):
    c = F.BY_NAME[name]
    ref = F.reference(c)                                                    # raises when no draw is kink-free
    assert ref.draws <= F.MAX_DRAWS and ref.kink >= F.KINK_MIN, (ref.draws, ref.kink)
    rows = F.distinct_bn_rows(ref)
    if c.mode == N.BN_TRAIN:
        assert rows >= F.MIN_BN_ROWS, rows
    assert ref.e32["logits"] <= F.CAP_LOGITS, ref.e32["logits"]
    over = {k: v for k, v in ref.e32.items() if k.split("/")[0] in GRADS and not v <= F.CAP_GRAD}
    assert not over, over
    if c.rows is not None:                                                  # dlogits is zero off the sentinel rows, nonzero on them
        nz = sorted(set(torch.nonzero(ref.G.abs().sum(1)).reshape(-1).tolist()))
        assert nz == F.sentinel_rows(c), nz
    lay = max((v, k) for k, v in ref.e32.items() if k.split("/")[0] in LAYER)
    grad = max([(v, k) for k, v in ref.e32.items() if k.split("/")[0] in GRADS], default=(0.0, "-"))
    print("%s: draws %d, kink %.1e, distinct BN rows %d, fp32 module: logits %.1e, worst gradient %.1e (%s), worst per-layer %.1e (%s)"
          % (name, ref.draws, ref.kink, rows, ref.e32["logits"], grad[0], grad[1], lay[0], lay[1]))
    for prec in (F.SPLIT, F.F32):                                           # every bar is a finite positive number or an exact 0
        for k, b in F.bars(ref, prec).items():
            assert b == 0.0 or 1e-5 <= b < 1e-3 + 1e-12, (k, b)


@pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")
@pytest.mark.parametrize("name", NAMES)
def test_restated_plan_equals_fcn_convnet_sizes(name):
    c = F.BY_NAME[name]
    rc, got = F.sizes(F.load_emu(), F.make_desc(c))
    assert rc == 0, rc
    lay, want = F.plan(c.B, c.Ls, c.c1, c.reg_out)
    assert got == want, (got, want)
    assert len(lay) == 4 * len(c.Ls) - 2
