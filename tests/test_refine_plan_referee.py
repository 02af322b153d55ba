"""CPU: the numpy restatement of the capturable refine-stage training input (tests/refine_plan_ref.py) against the host path it
replaces -- its plan against the kept list, the zeroed counts and the one cumulative sum cascade.refine_training_candidates computes
from the same (random) segment counts, which the test feeds in place of the host emulation's count and reads off its fill call; its
window rule against RefineInputBuilder._lpad at widths on and beside exact multiples of every stride -- plus the known properties of
the jitter draw's counter layout."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import draws_ref
import refine_plan_ref as ref
from test_refine_label_referee import golden

CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
STRIDES = (0.1, 0.2, 0.4, 0.8)
BIG = (1 << 20,) * 4


def test_jitter_draw_contract_stream():
    j = ref.jitter_draw(1234, (1 << 32) + 5, 3, 2)
    assert j.shape == (3, 2, 7) and j.dtype == np.float64 and (j >= 0).all() and (j < 1).all()
    w = draws_ref._words(1234, (1 << 32) + 5, 2 * 2 + 1, 3, 16)                 # unit u = d * A + a = 5
    assert j[2, 1].tolist() == [draws_ref._u53(w[2 * i], w[2 * i + 1]) * 2.0 ** -53 for i in range(7)]
    assert len(set(j.reshape(-1).tolist())) == 42                               # no two uniforms share their words
    assert not np.array_equal(j, ref.jitter_draw(1234, 5, 3, 2)) and not np.array_equal(j, ref.jitter_draw(1235, (1 << 32) + 5, 3, 2))
    # the table of (D, A) is the first D * A units of any larger one: a unit's draws depend on u alone
    assert np.array_equal(ref.jitter_draw(7, 0, 6, 1).reshape(-1), ref.jitter_draw(7, 0, 3, 2).reshape(-1))
    for tag in (0, 1, 2):                                                       # no stream of fcn_draw_batch shares a counter
        assert not np.array_equal(draws_ref._words(1234, 5, 7, tag, 16), draws_ref._words(1234, 5, 7, 3, 16))


def test_plan_cases_by_hand():
    cnt = np.asarray([[5, 0, 2], [3, 3, 3], [0, 0, 0], [4, 1, 0], [7, 7, 7]])
    pos = np.asarray([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 0], [2, 0, 0]])
    psz = np.asarray([[4.0, 1.6, 1.5]] * 5)
    su, n, so, off, counts, st = ref.plan(cnt, pos, psz, STRIDES, BIG, 4, 100)  # units 0, 3, 4 survive
    assert su.tolist() == [0, 3, 4, 5] and n == 3 and st == ref.ST_FEW
    assert so.tolist() == [0, 5, 5, 7, 7, 7, 7, 7, 7, 7, 11, 12, 12, 19, 26, 33] and off.tolist() == [0, 7, 12, 100, 33]
    assert counts.tolist() == [7, 5, 21, 0]
    su, n, so, off, counts, st = ref.plan(cnt, pos, psz, STRIDES, BIG, 2, 11)   # two slots, one row short
    assert su.tolist() == [0, 3] and n == 2 and st == ref.ST_TRUNC and off.tolist() == [0, 7, 11] and counts.tolist() == [7, 4]
    su, n, so, off, counts, st = ref.plan(cnt, pos * 0, psz, STRIDES, BIG, 2, 11)
    assert su.tolist() == [5, 5] and n == 0 and st == ref.ST_FEW and not so.any() and off.tolist() == [11, 11, 0] and not counts.any()
    assert su.dtype == np.int32 and so.dtype == np.int64 and off.dtype == np.int64 and counts.dtype == np.int64
    # widths: a bad one counts only on a unit with positives; a wide one likewise
    bad = psz.copy()
    bad[1, 1], bad[3, 1] = np.nan, -1.0
    su, n, so, off, counts, st = ref.plan(cnt, pos, bad, STRIDES, BIG, 2, 100)
    assert su.tolist() == [0, 4] and st == ref.ST_WIDTH
    su, n, so, off, counts, st = ref.plan(cnt, pos, psz, STRIDES, (16, 8, 4, 1), 2, 100)       # 1.6 / 0.8 = 2 windows > 1
    assert n == 0 and st == ref.ST_WIDE | ref.ST_FEW
    assert ref.plan(cnt, pos, psz, STRIDES, (16, 8, 4, 2), 3, 100)[5] == 0


def test_window_rule_equals_the_builders_lpad():
    """len(np.arange(-w/2, w/2, s)) through RefineInputBuilder._lpad against the restated rule, at widths on an exact multiple of
    each stride, one ulp and a little to either side of it, and at plain widths."""
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    b = inputs.RefineInputBuilder(64, strides=STRIDES, device="cpu")
    widths = [0.05, 1.6, 1.9, 2.345, 4.2, 7.0]
    for s in STRIDES:
        for k in (1, 3, 8, 21):
            w = k * s
            widths += [w, np.nextafter(w, 0.0), np.nextafter(w, 100.0), w - 1e-9, w + 1e-9]
    for w in widths:
        want = b._lpad([w])
        got = [ref.windows(float(w), s) for s in STRIDES]
        assert got == [float(x) for x in want], (w, got, want)
        # the plan keeps the unit at exactly these window counts and drops it one window short on any single stride
        one = (np.asarray([[3]]), np.asarray([[1]]), np.asarray([[4.0, w, 1.5]]))
        assert ref.plan(*one, STRIDES, want, 1, 10)[5] == 0
        for s in range(4):
            if want[s] > 1:
                short = list(want)
                short[s] -= 1
                assert ref.plan(*one, STRIDES, short, 1, 10)[5] == ref.ST_WIDE | ref.ST_FEW, (w, s)
    for w in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            b._lpad([w])
        assert ref.plan(np.asarray([[3]]), np.asarray([[1]]), np.asarray([[4.0, w, 1.5]]), STRIDES, BIG, 1, 10)[5] == ref.ST_WIDTH | ref.ST_FEW


@pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_equals_what_refine_training_candidates_computes_from_the_same_counts(seed):
    """B >= survivors, capacity >= total and lpad non-binding: the regime in which the host path and the plan describe the same
    packed buffers.  The counts are random (U, S) tables written in place of the count's outputs."""
    import torch
    from emu_shim import emulated_gpu
    from frustum_convnet_amd import cascade
    g = golden()
    D, A, S = 8, 3, 3
    U = D * A
    rs = np.random.RandomState(seed)
    cnt = rs.randint(0, 900, (U, S)).astype(np.int32)
    pos = np.minimum(cnt, rs.randint(0, 5, (U, S))).astype(np.int32)
    pos[rs.uniform(size=U) < 0.4] = 0                                           # rejected: no positive
    if seed == 2:
        pos[:] = 0
    psz = np.tile(np.asarray([[4.0, 1.6, 1.5]]), (U, 1))
    seen = {}
    with emulated_gpu() as L:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        real_count, real_fill = L.fcn_refine_label_count, L.fcn_refine_label_fill

        def count(*a):
            assert a[8] * a[13] == U and a[16] == S
            ctypes.memmove(a[17], cnt.ctypes.data, cnt.nbytes)
            ctypes.memmove(a[18], pos.ctypes.data, pos.nbytes)
            return 0

        def fill(*a):
            seen["seg_off"] = np.frombuffer((ctypes.c_int64 * (U * S + 1)).from_address(a[17]), dtype=np.int64).copy()
            return 0
        try:
            L.fcn_refine_label_count, L.fcn_refine_label_fill = count, fill
            sel = cascade.refine_training_candidates(dev(g["points"]), dev(g["off"]), dev(g["dets"]), g["cand_row"], g["cand_frame"],
                                                     g["ref_gt_idx"].astype(np.int32), g["gt_box3d"], jitter=g["jitter"])
        finally:
            L.fcn_refine_label_count, L.fcn_refine_label_fill = real_count, real_fill
        off = sel["off"].numpy().copy() if "off" in sel else None
    slot_unit, n, seg_off, poff, counts, st = ref.plan(cnt, pos, psz, STRIDES, BIG, U, 1 << 40)
    kept = sel["kept"]
    assert n == len(kept) and np.array_equal(slot_unit[:n], kept) and (slot_unit[n:] == U).all()
    assert st == (ref.ST_FEW if n < U else 0)
    if seed == 2:
        assert n == 0 and not seg_off.any() and "seg_off" not in seen            # (no fill without a survivor)
        return
    assert 0 < n < U
    assert np.array_equal(seg_off, seen["seg_off"])                              # the zeroed counts and the cumulative sum
    assert np.array_equal(poff[:n], off[:n]) and poff[U] == off[-1] and (poff[n:U] == 1 << 40).all()
    assert np.array_equal(counts[:n], sel["counts"]) and not counts[n:].any()
