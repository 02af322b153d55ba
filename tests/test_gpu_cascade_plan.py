"""-m gpu: the capturable two-stage inference link -- fcn_cascade_candidates, fcn_refine_detect_count / _plan / _fill
(csrc/cascade_plan.h) through the C-ABI against the numpy restatement of tests/cascade_plan_ref.py (pinned to the host path by
tests/test_cascade_plan_referee.py) and against the reading selection fcn_refine_select_count / _fill, and cascade.CascadeLink
against the path it replaces (TwoStageDetector.detect: refine_candidates + RefineInputBuilder.build_device + stage2.detect), against
the second stage run by hand on the link's own batch, and under a captured graph.  The models and the first-stage batch are those of
tests/test_gpu_cascade.py (hash-initialised car_b4_n512 and refine_b4_n512, B1 = 4, N = 512, top_k = 6, two groups);
tests/test_emu_cascade_plan.py runs the same functions on the host emulation of the kernels (all but the graph capture)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cascade_plan_ref as R
from refine_plan_ref import windows
from test_gpu_cascade import BADARG, _bits, _dev, _edge_scene, _expected_rows, _p, _scene, _tensors
from test_gpu_cascade import _count as _select_count
from test_gpu_cascade import _fill as _select_fill
from test_gpu_refine_plan import _guarded, _intact

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
SEED = 20240917
STRIDES = (0.1, 0.2, 0.4, 0.8)
BIG = (64, 32, 16, 8)              # window counts for widths up to 6.4


# ------------------------------------------------------------------------------------------------ the candidate table
CAND_OUT = (("cand_row", torch.int32), ("cand_frame", torch.int32), ("cand_class", torch.int32), ("cand_group", torch.int32),
            ("cand_score", torch.float32))
UFRAME, UCLASS, UGROUP = np.asarray([0, 0, 1, 1], np.int32), np.asarray([2, 0, 1, 1], np.int32), np.asarray([0, 0, 1, 2], np.int32)


def _dets(R_=20, seed=0):
    return np.random.RandomState(seed).uniform(-1, 1, (R_, 8)).astype(np.float32)


def _cands(keep, cnt, D, L2=5, uframe=UFRAME, uclass=UCLASS, ugroup=UGROUP, dets=None):
    """The raw entry on exactly sized inputs and poisoned, guarded outputs, held to the restatement -> outputs, n_cand, status."""
    from frustum_convnet_amd import _native
    dets = _dets() if dets is None else dets
    keep, cnt = np.asarray(keep, dtype=np.int32), np.asarray(cnt, dtype=np.int32)
    G, top_k = keep.shape
    o = {k: _guarded((D,), dt, -7) for k, dt in CAND_OUT}
    n, nbuf = _guarded((1,), torch.int32, -7)
    status, sbuf = _guarded((1,), torch.int32, 0)
    ins = [_dev(x) for x in (keep, cnt, uframe, uclass, ugroup, dets)]
    rc = _native.lib().fcn_cascade_candidates(_p(ins[0]), _p(ins[1]), G, top_k, L2, _p(ins[2]), _p(ins[3]), _p(ins[4]), len(uframe),
                                              _p(ins[5]), len(dets), D, *[_p(o[k][0]) for k, _ in CAND_OUT], _p(n), _p(status),
                                              _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(_intact(buf, -7) for _, buf in o.values()) and _intact(nbuf, -7) and _intact(sbuf, 0)
    got = {k: v.cpu().numpy() for k, (v, _) in o.items()}
    want, wn, wst = R.candidates(keep, cnt, L2, uframe, uclass, ugroup, dets, D)
    for k, _ in CAND_OUT:                                                   # (poisoned first: equality says every row is written)
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert int(n.cpu()[0]) == wn and int(status.cpu()[0]) == wst
    return got, wn, wst


KEEP3 = [[7, 3, 9, 4, 0, 1], [12, 11, 10, 13, 14, 2], [19, 15, 16, 17, 18, 5]]


@pytest.mark.parametrize("case", ["one_group", "empty_group", "overflowed_group", "count_beyond_top_k", "exactly_D", "D_plus_one",
                                  "D_is_one", "entries_out_of_range", "many_groups", "at_the_limits"])
def test_candidates_equal_the_restatement(case):
    if case == "one_group":
        got, n, st = _cands([KEEP3[0]], [4], 6)
        assert n == 4 and st == 0 and got["cand_row"].tolist() == [7, 3, 9, 4, -1, -1] and got["cand_group"].tolist() == [0, 0, 0, 0, 1, 1]
    elif case == "empty_group":
        got, n, st = _cands(KEEP3, [2, 0, 3], 8)
        assert n == 5 and st == 0 and got["cand_row"][:5].tolist() == [7, 3, 19, 15, 16] and got["cand_frame"].tolist() == [0, 0, 1, 1, 1, -1, -1, -1]
    elif case == "overflowed_group":
        got, n, st = _cands(KEEP3, [2, -1, 3], 8)
        assert n == 5 and st == R.ST_GROUP and got["cand_row"][:5].tolist() == [7, 3, 19, 15, 16]
    elif case == "count_beyond_top_k":
        got, n, st = _cands(KEEP3, [2, 7, 3], 8)
        assert n == 5 and st == R.ST_GROUP
        assert _cands(KEEP3, [2 ** 31 - 1, 1, -2 ** 31], 8)[1:] == (1, R.ST_GROUP)
    elif case == "exactly_D":                                               # cnt = top_k in two groups: 12 rows for 12 candidates
        got, n, st = _cands(KEEP3, [6, 6, 0], 12)
        assert n == 12 and st == 0 and got["cand_row"].tolist() == KEEP3[0] + KEEP3[1]
    elif case == "D_plus_one":
        got, n, st = _cands(KEEP3, [6, 6, 0], 11)
        assert n == 11 and st == R.ST_ROWS and got["cand_row"].tolist() == (KEEP3[0] + KEEP3[1])[:11]
        assert _cands(KEEP3, [6, 6, 6], 7)[1:] == (7, R.ST_ROWS)
    elif case == "D_is_one":
        got, n, st = _cands(KEEP3, [0, 3, 1], 1)
        assert n == 1 and st == R.ST_ROWS and got["cand_row"].tolist() == [12] and got["cand_class"].tolist() == [1]
        assert _cands(KEEP3, [0, 0, 1], 1)[1:] == (1, 0) and _cands(KEEP3, [0, 0, 0], 1)[1:] == (0, 0)
    elif case == "entries_out_of_range":
        bad = np.asarray(KEEP3)
        bad[0, 1], bad[1, 0], bad[2, 2], bad[2, 3] = 20, -1, -2 ** 31, 2 ** 31 - 1
        got, n, st = _cands(bad, [3, 3, 4], 8)
        assert n == 6 and st == 0 and got["cand_row"][:6].tolist() == [7, 9, 11, 10, 19, 15]
        got, n, st = _cands(KEEP3, [3, 3, 3], 8, uframe=UFRAME[:3], uclass=UCLASS[:3], ugroup=UGROUP[:3])      # B1 = 3: rows >= 15 belong to nobody
        assert n == 6 and st == 0 and got["cand_row"][:6].tolist() == [7, 3, 9, 12, 11, 10]
    else:
        rs = np.random.RandomState(4)
        G, top_k = (700, 3) if case == "many_groups" else (65536, 2)         # more groups than threads; the largest call
        dets = _dets(4000, 1)
        keep = rs.randint(-3, 4003, (G, top_k))
        cnt = rs.randint(-1, top_k + 2, G) * (rs.uniform(size=G) < (0.9 if G == 700 else 0.02))
        uf, uc, ug = (rs.randint(0, 9, 790).astype(np.int32) for _ in range(3))
        for D in (2048, 100):
            got, n, st = _cands(keep, cnt, D, uframe=uf, uclass=uc, ugroup=ug, dets=dets)
            assert st & R.ST_GROUP and bool(st & R.ST_ROWS) == (D == 100) and (n == 100 if D == 100 else 400 < n < 2048)


# ------------------------------------------------------------------------------------------------ count / fill on the (S, D) grid
def _dcount(t, S, ratio=1.2):
    """The raw count entry on device tensors t (pts, off, dets, crow, cframe) -> rc, outputs (sentinel-filled first)."""
    from frustum_convnet_amd import _native
    D = t["crow"].numel()
    o = {"seg_cnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "pred_box3d": torch.full((D, 8, 3), -7.0, dtype=torch.float64, device="cuda"),
         "pred_angle": torch.full((D,), -7.0, dtype=torch.float64, device="cuda"),
         "pred_size": torch.full((D, 3), -7.0, dtype=torch.float64, device="cuda")}
    rc = _native.lib().fcn_refine_detect_count(
        _p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, t["pts"].shape[1], _p(t["dets"]), t["dets"].shape[0], _p(t["crow"]),
        _p(t["cframe"]), D, ratio, S, _p(o["seg_cnt"]), _p(o["pred_box3d"]), _p(o["pred_angle"]), _p(o["pred_size"]),
        _native.current_stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _dfill(t, S, seg_counts, ratio=1.2, front=0, guard=5):
    """The raw fill entry on offsets from seg_counts (D, S) -> rc, the whole buffer (front + total + guard rows), seg_off."""
    from frustum_convnet_amd import _native
    D, ps = t["crow"].numel(), t["pts"].shape[1]
    soff = (front + np.concatenate([[0], np.cumsum(np.asarray(seg_counts).reshape(-1))])).astype(np.int64)
    out = torch.full((int(soff[-1]) + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    soff_d = _dev(soff)
    rc = _native.lib().fcn_refine_detect_fill(
        _p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, ps, _p(t["dets"]), t["dets"].shape[0], _p(t["crow"]), _p(t["cframe"]),
        D, ratio, S, _p(soff_d), _p(out), _native.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), soff


@pytest.mark.parametrize("stride", [4, 5])
def test_segmented_selection_equals_the_reading_selection_bit_for_bit(stride):
    """The scene of tests/test_gpu_cascade.py (frames of 1000, 77 and 0 rows: S = 1, and S = 2 with an empty second segment)."""
    sc = _scene(stride)
    t = _tensors(sc)
    rc, want = _select_count(t)
    assert rc == 0
    want = {k: v.cpu().numpy() for k, v in want.items()}
    rcf, wrows, _, _ = _select_fill(t, want["cnt"])
    assert rcf == 0 and len(wrows) > 1000
    for S in (1, 2):
        rc, got = _dcount(t, S)
        assert rc == 0 and np.array_equal(got["seg_cnt"].sum(1), want["cnt"]) and (got["seg_cnt"] >= 0).all()
        for k in ("pred_box3d", "pred_angle", "pred_size"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        rc, buf, soff = _dfill(t, S, got["seg_cnt"], front=4)
        assert rc == 0 and np.array_equal(_bits(buf[4:soff[-1]]), _bits(wrows))
        assert (buf[:4] == -7.0).all() and (buf[soff[-1]:] == -7.0).all() and len(buf) == soff[-1] + 5


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("stride", [4, 5])
def test_segmented_selection_over_the_frame_lengths_the_scan_turns_on(stride, S):
    """Frames of 0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1 and 2 * seg + 100 rows, one candidate each: segment s of a candidate
    counts the referee's rows of [s * seg, (s + 1) * seg); S = 3 covers every frame and equals the reading selection bit for bit;
    with S = 1 or 2 the frames that fit are whole and the longer ones are searched S segments deep (the caller's duty)."""
    from frustum_convnet_amd import _native
    seg = int(_native.lib().fcn_frustum_select_seg())
    sc = _edge_scene(stride)
    ref = sc["ref"]
    t = _tensors(sc)
    want = np.asarray([[((idx // seg) == s).sum() for s in range(S)] for idx in ref["index"]])
    assert want[-1].all() and (want[6:9, 0] > 0).all() and (S < 2 or (want[8, 1] <= 1 and want[:8, 1:].sum() == 0))
    rc, got = _dcount(t, S)
    assert rc == 0 and np.array_equal(got["seg_cnt"], want)
    rows = np.concatenate([sc["pts"][int(sc["off"][f]):][idx[idx < S * seg]] for idx, f in zip(ref["index"], sc["cframe"])], 0)
    rc, buf, soff = _dfill(t, S, got["seg_cnt"])
    assert rc == 0 and np.array_equal(_bits(buf[:soff[-1]]), _bits(rows)) and (buf[soff[-1]:] == -7.0).all()
    if S == 3:
        rc, o = _select_count(t)
        assert rc == 0 and np.array_equal(got["seg_cnt"].sum(1), o["cnt"].cpu().numpy())
        for k in ("pred_box3d", "pred_angle", "pred_size"):
            assert got[k].tobytes() == o[k].cpu().numpy().tobytes(), k
        rc, wrows, _, _ = _select_fill(t, o["cnt"].cpu().numpy())
        assert rc == 0 and np.array_equal(_bits(buf[:soff[-1]]), _bits(wrows))
        assert np.array_equal(_bits(rows), _bits(_expected_rows(sc)))
    # offsets that grant a segment too little drop the surplus and touch nothing else; the empty grant stores nothing
    less = got["seg_cnt"].copy()
    less[-1, 0] -= 50
    rc, buf2, soff2 = _dfill(t, S, less)
    assert rc == 0 and (buf2[soff2[-1]:] == -7.0).all()
    at = soff[(len(less) - 1) * S]
    assert np.array_equal(_bits(buf2[:at + less[-1, 0]]), _bits(buf[:at + less[-1, 0]]))
    assert np.array_equal(_bits(buf2[at + less[-1, 0]:soff2[-1]]), _bits(buf[at + less[-1, 0] + 50:soff[-1]]))
    rc, buf3, _ = _dfill(t, S, less * 0)
    assert rc == 0 and (buf3 == -7.0).all()


@pytest.mark.parametrize("what", ["row_high", "row_negative", "frame_high", "frame_negative"])
def test_out_of_range_candidate_is_skipped_silently_and_never_dereferenced(what):
    """Exactly sized device buffers (nothing beyond them can be read), sentinel-filled outputs: the bad candidate's counts are 0,
    nothing else of it is written, the others are processed, every call returns 0."""
    sc = _scene(4)
    crow, cframe = sc["crow"].copy(), sc["cframe"].copy()
    bad = 5                                                                 # the candidate with the most rows
    if what.startswith("row"):
        crow[bad] = 10 if what == "row_high" else -(2 ** 31)                # R = 10
    else:
        cframe[bad] = 3 if what == "frame_high" else -1                     # F = 3
    rc, good = _dcount(_tensors(sc), 1)
    t = _tensors(sc, crow=crow, cframe=cframe)
    rc2, got = _dcount(t, 1)
    assert rc == 0 and rc2 == 0 and good["seg_cnt"][bad, 0] > 256
    others = [d for d in range(len(crow)) if d != bad]
    assert got["seg_cnt"][bad, 0] == 0 and np.array_equal(got["seg_cnt"][others], good["seg_cnt"][others])
    for k in ("pred_box3d", "pred_angle", "pred_size"):
        assert (got[k][bad] == -7.0).all() and got[k][others].tobytes() == good[k][others].tobytes(), k
    rc, buf, soff = _dfill(t, 1, good["seg_cnt"])                           # granted its reference rows: it stores none of them
    rcg, gbuf, _ = _dfill(_tensors(sc), 1, good["seg_cnt"])
    assert rc == 0 and rcg == 0 and (buf[soff[-1]:] == -7.0).all()
    assert (buf[soff[bad]:soff[bad + 1]] == -7.0).all()
    assert np.array_equal(_bits(buf[:soff[bad]]), _bits(gbuf[:soff[bad]])) and np.array_equal(_bits(buf[soff[bad + 1]:]), _bits(gbuf[soff[bad + 1]:]))


# ------------------------------------------------------------------------------------------------ the plan
PLAN_OUT = (("slot_unit", torch.int32, lambda D, S, B: (B,)), ("n_kept", torch.int32, lambda D, S, B: (1,)),
            ("seg_off", torch.int64, lambda D, S, B: (D * S + 1,)), ("off", torch.int64, lambda D, S, B: (B + 1,)),
            ("counts", torch.int64, lambda D, S, B: (B,)))


def _plan_equals(cnt, psz, B, capacity, lpad=BIG, strides=STRIDES):
    """The raw entry on exactly sized inputs and poisoned, guarded outputs, held to the restatement (every output is poisoned
    first, so equality also says that every output is written) -> the restatement's tuple."""
    from frustum_convnet_amd import _native
    cnt = np.asarray(cnt)
    D, S = cnt.shape
    o = {k: _guarded(shape(D, S, B), dt, -7) for k, dt, shape in PLAN_OUT}
    status, sbuf = _guarded((1,), torch.int32, 0)
    ins = (_dev(cnt.astype(np.int32)), _dev(np.asarray(psz, dtype=np.float64).reshape(D, 3)))
    rc = _native.lib().fcn_refine_detect_plan(_p(ins[0]), _p(ins[1]), (ctypes.c_double * 4)(*strides), (ctypes.c_int32 * 4)(*lpad),
                                              D, S, B, capacity, *[_p(o[k][0]) for k, _, _ in PLAN_OUT], _p(status),
                                              _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(_intact(buf, -7) for _, buf in o.values()) and _intact(sbuf, 0)
    got = {k: v.cpu().numpy() for k, (v, _) in o.items()}
    want = R.plan(cnt, psz, strides, lpad, B, capacity)
    for k, w in (("slot_unit", want[0]), ("seg_off", want[2]), ("off", want[3]), ("counts", want[4])):
        assert np.array_equal(got[k], w), k
    assert int(got["n_kept"][0]) == want[1] and int(status.cpu()[0]) == want[5]
    return want


def _counts(D=12, S=3, seed=0):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 900, (D, S))
    cnt[[1, 6]] = 0                                                         # no row: rejected
    cnt[3, 1] = 0
    psz = np.stack([rs.uniform(3, 5, D), rs.uniform(0.5, 2.5, D), rs.uniform(1, 2, D)], 1)
    return cnt, psz


@pytest.mark.parametrize("B", [4, 10, 12])
def test_plan_equals_the_restatement(B):
    """B below, equal to and above the 10 survivors (two candidates without a row between candidates with rows); a capacity that
    is exactly met, one row short, inside a segment, at a candidate boundary, and 0."""
    cnt, psz = _counts()
    survivors = [d for d in range(12) if d not in (1, 6)]
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, B, 1 << 40)
    assert slot_unit[:n].tolist() == survivors[:B] and n == min(B, 10) and st == (R.ST_MANY if B == 4 else 0)      # never bit 1
    held = survivors[:B]
    total = int(cnt[held].sum())
    assert off[B] == total and (off[n:B] == 1 << 40).all() and (slot_unit[n:] == 12).all()
    assert np.array_equal(counts[:n], cnt[held].sum(1)) and not counts[n:].any()
    many = st
    assert _plan_equals(cnt, psz, B, total)[5] == many                      # exactly met: no bit 2
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, B, total - 1)
    assert st == many | R.ST_TRUNC and off[B] == total - 1 and counts[n - 1] == cnt[held[-1]].sum() - 1 and (off[n:B] == total - 1).all()
    first = int(cnt[held[0]].sum())
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, B, first + 5)
    assert st & R.ST_TRUNC and counts[:3].tolist() == [first, 5, 0] and off[1] == first and off[2] == first + 5
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, B, first)
    assert st & R.ST_TRUNC and counts[:2].tolist() == [first, 0] and not counts[2:].any() and n == min(B, 10)
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, B, 0)
    assert st & R.ST_TRUNC and not counts.any() and not off.any() and not seg_off.any()
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt * 0, psz, B, 1000)       # nobody survives: the normal case, no bit
    assert n == 0 and st == 0 and not seg_off.any() and off.tolist() == [1000] * B + [0] and (slot_unit == 12).all()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [255, 256, 257])
def test_plan_where_a_threads_run_goes_from_one_candidate_to_two(D, S):
    """The run-per-thread split is csrc/slot_plan.h's, shared by every plan: over 256 threads, 255 and 256 candidates are runs of
    one (the last thread's empty, then not), 257 candidates are runs of two with threads 129.. owning nothing.  B = D, some
    candidates without a row, a capacity one row short of the total."""
    rs = np.random.RandomState(4 * D + S)
    cnt = rs.randint(0, 900, (D, S)) * (rs.uniform(size=(D, 1)) < 0.7)
    psz = np.stack([rs.uniform(3, 5, D), rs.uniform(0.5, 2.5, D), rs.uniform(1, 2, D)], 1)
    total = int(cnt.sum())
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, D, total - 1)
    assert 0 < n < D and st == R.ST_TRUNC and seg_off[-1] == total - 1 and counts.sum() == total - 1


def test_plan_at_its_smallest_and_at_its_limits():
    assert _plan_equals([[7]], [[4.0, 1.6, 1.5]], 1, 100)[3].tolist() == [0, 7]        # D = B = S = 1
    assert _plan_equals([[0]], [[4.0, 1.6, 1.5]], 1, 100)[5] == 0
    rs = np.random.RandomState(1)
    D, S = 777, 5                                                           # more candidates than threads, sums beyond 2^31
    cnt = rs.randint(0, 2 ** 31 - 1, (D, S)) * (rs.uniform(size=(D, 1)) < 0.6)
    psz = np.tile(np.asarray([[4.0, 1.6, 1.5]]), (D, 1))
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, 300, 1 << 50)
    assert n == 300 and st == R.ST_MANY and seg_off[-1] > 2 ** 33 and (np.diff(slot_unit) > 0).all()
    _plan_equals(cnt, psz, 700, 1 << 36)
    from frustum_convnet_amd import cascade
    max_u, max_segs = cascade.RefineTrainSource.limits()
    D, S = max_u, max_segs // max_u                                         # the largest plan: 2048 candidates of 32 segments
    cnt = rs.randint(0, 50, (D, S)) * (rs.uniform(size=(D, 1)) < 0.5)
    psz = np.tile(np.asarray([[4.0, 1.6, 1.5]]), (D, 1))
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, psz, D, 1 << 40)
    assert (D, S) == (2048, 32) and 500 < n < D and st == 0


def test_plan_widths():
    cnt, psz = _counts()
    bad = psz.copy()
    bad[[0, 2, 5, 9], 1] = [0.0, -1.5, np.nan, np.inf]                      # on candidates with rows: bit 6, no slot
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, bad, 12, 1 << 40)
    assert st == R.ST_WIDTH and slot_unit[:n].tolist() == [3, 4, 7, 8, 10, 11]
    for w in (0.0, -1.5, np.nan, np.inf, 1e300):
        quiet = psz.copy()
        quiet[[1, 6], 1] = w                                                # on candidates without a row: never read
        assert _plan_equals(cnt, quiet, 10, 1 << 40)[5] == 0, w
        loud = psz.copy()
        loud[4, 1] = w
        slot_unit, n, _, _, _, st = _plan_equals(cnt, loud, 10, 1 << 40)
        assert st == (R.ST_WIDE if w == 1e300 else R.ST_WIDTH) and 4 not in slot_unit.tolist(), w
    # ceil(w / stride) == lpad[s] passes, one window under passes, one window over does not: on each of the four strides alone
    for s, stride in enumerate(STRIDES):
        for k in (2, 3, 8):
            lpad = [1 << 20] * 4
            lpad[s] = k
            on = k * stride                                                 # (k * stride rounds: walk to the last width of k windows)
            while windows(on, stride) > k:
                on = np.nextafter(on, 0.0)
            while windows(np.nextafter(on, 100.0), stride) <= k:
                on = np.nextafter(on, 100.0)
            over = np.nextafter(on, 100.0)
            under = (k - 1) * stride * 0.999
            assert windows(under, stride) == k - 1 and windows(on, stride) == k and windows(over, stride) == k + 1
            for w in (under, on):
                assert _plan_equals([[3, 4]], [[4.0, w, 1.5]], 1, 100, lpad=lpad)[5] == 0, (s, k, w)
            slot_unit, n, seg_off, off, counts, st = _plan_equals([[3, 4]], [[4.0, over, 1.5]], 1, 100, lpad=lpad)
            assert st == R.ST_WIDE and n == 0 and slot_unit.tolist() == [1] and off.tolist() == [100, 0], (s, k)
    _plan_equals(cnt, psz, 6, 1 << 40, lpad=(9, 5, 3, 2), strides=(0.25, 0.5, 1.0, 2.0))


def test_count_plan_fill_stays_within_capacity_plus_one_rows():
    """count -> plan -> fill on the scene with the capacity exactly met and exceeded by one row, into a buffer of exactly
    capacity + 1 rows between guard rows."""
    from frustum_convnet_amd import _native
    sc = _scene(4)
    t = _tensors(sc)
    rc, o = _dcount(t, 1)
    total = int(o["seg_cnt"].sum())
    rc2, full, _ = _dfill(t, 1, o["seg_cnt"], guard=0)
    assert rc == 0 and rc2 == 0 and total > 1000
    for cap, bit in ((total, 0), (total - 1, R.ST_TRUNC)):
        slot_unit, n, seg_off, off, counts, st = _plan_equals(o["seg_cnt"], o["pred_size"], 7, cap, lpad=(1 << 20,) * 4)
        assert st == bit and n == 5 and seg_off[-1] == cap and counts.sum() == cap
        buf = torch.full((cap + 1 + 8, 4), -7.0, dtype=torch.float32, device="cuda")
        soff = _dev(seg_off)
        assert _native.lib().fcn_refine_detect_fill(_p(t["pts"]), _p(t["off"]), 3, 4, _p(t["dets"]), 10, _p(t["crow"]), _p(t["cframe"]), 7,
                                                    1.2, 1, _p(soff), _p(buf[4:]), _native.current_stream()) == 0
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:4] == -7.0).all() and (h[4 + cap:] == -7.0).all() and np.array_equal(_bits(h[4:4 + cap]), _bits(full[:cap]))


# ------------------------------------------------------------------------------------------------ CascadeLink
FRUSTUM_FRAME, TYPES, UG = [0, 0, 1, 1], ["Car", "Car", "Pedestrian", "Cyclist"], [0, 0, 1, 1]
KW = dict(method="nms", thresh=0.1, top_k=6)
DD_KEYS = ("point_cloud", "one_hot", "center_ref1", "center_ref2", "center_ref3", "center_ref4")
BATCH_KEYS = ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "rot_angle", "ref_center", "one_hot", "rgb_prob")


def _stages():
    """The two hash-initialised models, the refine builder and the first-stage batch of test_two_stage_detector_equals_..."""
    from helpers import load_golden, golden_inputs
    from test_gpu_model import _model
    from frustum_convnet_amd import inputs, synth
    g1, g2 = load_golden("car_b4_n512"), load_golden("refine_b4_n512")
    m1 = _model(g1).eval()
    data = synth.to_torch(golden_inputs(g1), "cuda")
    m2 = _model(g2).eval()                                       # (cfg now holds the refine strides: the builder reads them)
    builder = inputs.RefineInputBuilder(int(g2["meta_npoint"]))
    return m1, m2, builder, {k: data[k].contiguous() for k in DD_KEYS}


@functools.lru_cache(maxsize=None)
def _frames_np(where, d1_bytes, rows):
    """Two frames as that test builds them -- each frustum's own points and a cloud around every kept first-stage box -- behind
    4000 far rows in frame 0, so that its boxes' rows lie in the second 4096-row segment (S = 2)."""
    from helpers import load_golden, golden_inputs
    pc = golden_inputs(load_golden("car_b4_n512"))["point_cloud"]
    d1 = np.frombuffer(d1_bytes, dtype=np.float32).reshape(-1, 8).astype(np.float64)
    rng = np.random.RandomState(9)
    L2 = len(d1) // 4
    frames = []
    for f in range(2):
        own = [np.asarray(pc[u]).T for u in range(4) if FRUSTUM_FRAME[u] == f]
        near = [np.array([d1[r, 0], d1[r, 1] - d1[r, 5] / 2.0, d1[r, 2]]) + rng.uniform(-2.5, 2.5, (150, 3))
                for r in rows if FRUSTUM_FRAME[r // L2] == f]
        far = [rng.uniform(500, 600, (4000 if f == 0 else 0, 3))]
        xyz = np.concatenate(far + own + near, 0)
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], 1).astype(np.float32))
    return np.concatenate(frames, 0), np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)


def _first_stage(m1, dd):
    """stage1.detect and the frames around its kept rows -> s1, rows (host), fpts, foff."""
    s1 = m1.detect(dd, unit_group=torch.tensor(UG, dtype=torch.int32), num_groups=2, **KW)
    keep, cnt = s1[2].cpu().numpy(), s1[3].cpu().numpy()
    rows = np.concatenate([keep[g, :cnt[g]] for g in range(2)]).astype(np.int64)
    pts, off = _frames_np(str(s1[0].device), s1[0].cpu().numpy().tobytes(), tuple(rows.tolist()))
    assert len(rows) > 2 and off[1] > 4096
    return s1, rows, _dev(pts), off


def _host_batch(builder, s1, rows, fpts, foff, seed):
    """The existing path's batch on the same first-stage output: refine_candidates + build_device(draws=DeviceDraws(seed))."""
    from frustum_convnet_amd import cascade, inputs
    L2 = s1[0].shape[0] // 4
    unit = rows // L2
    cands = cascade.refine_candidates(fpts, foff, s1[0], rows.astype(np.int32), np.asarray(FRUSTUM_FRAME)[unit].astype(np.int32), 1.2)
    batch = builder.build_device(cands, [TYPES[u] for u in unit], draws=inputs.DeviceDraws(seed))
    return cands, batch


def _link(m1, m2, builder, fpts, foff, D, B, lpad, capacity=40000, seed=SEED, **over):
    from frustum_convnet_amd import cascade
    a = dict(frame_points=fpts, frame_off=foff, B1=4, L2=over.pop("L2", None), G=2, top_k=6, D=D, B=B, capacity=capacity, lpad=lpad,
             seed=seed, method="nms", thresh=0.1)
    a.update(over)
    units = a.pop("units", (FRUSTUM_FRAME, TYPES, UG))
    lk = cascade.CascadeLink(m1, m2, builder, a.pop("frame_points"), a.pop("frame_off"), a.pop("B1"), a.pop("L2"), a.pop("G"),
                             a.pop("top_k"), a.pop("D"), a.pop("B"), a.pop("capacity"), a.pop("lpad"), a.pop("seed"), a.pop("method"),
                             a.pop("thresh"), **a)
    return lk.set_units(*units)


def _host(x):
    return {k: v.cpu().clone() for k, v in x.items() if isinstance(v, torch.Tensor)}


def test_step_equals_the_existing_path_on_the_same_first_stage_output():
    """B = n_kept, lpad = the existing path's own batch maxima, the capacity exactly met, D one more than the kept rows: the batch,
    stage1_row and the detections equal TwoStageDetector.detect's bit for bit.  Then B = n_kept + 2 and lpad one larger: the filled
    slots' point_cloud / rot_angle / ref_center / one_hot / rgb_prob are still bit-identical, the detections equal stage2.detect
    run by hand on the link's batch, and no returned keep entry points into an empty slot's rows."""
    from frustum_convnet_amd import cascade, inputs
    m1, m2, builder, dd = _stages()
    L2 = int(dd["center_ref2"].shape[2])
    s1, rows, fpts, foff = _first_stage(m1, dd)
    cands, want = _host_batch(builder, s1, rows, fpts, foff, SEED)
    kept = want.pop("kept")
    n = len(kept)
    lpad = [int(want["center_ref%d" % (s + 1)].shape[2]) for s in range(4)]
    total = int(cands["counts"].sum())
    assert 2 <= n <= len(rows) and lpad == builder._lpad(cands["pred_size"][:, 1].cpu().numpy()[kept])
    two = cascade.TwoStageDetector(m1, m2, builder)
    res = two.detect(dd, fpts, foff, FRUSTUM_FRAME, TYPES, "nms", 0.1, unit_group=torch.tensor(UG, dtype=torch.int32), num_groups=2,
                     top_k=6, draws=inputs.DeviceDraws(SEED))
    assert np.array_equal(res["stage1_row"], rows[kept])
    # ---- the bit-identity conditions
    lk = two.link(fpts, foff, FRUSTUM_FRAME, TYPES, 4, L2, len(rows) + 1, n, total, lpad, SEED, "nms", 0.1,
                  unit_group=UG, num_groups=2, top_k=6)
    assert isinstance(lk, cascade.CascadeLink) and lk.S == 2 and (lk.D, lk.B, lk.G, lk.R) == (len(rows) + 1, n, 2, 4 * L2)
    got = lk.step(dd)
    torch.cuda.synchronize()
    lk.check()                                                              # nothing dropped, no empty slot: no bit
    assert int(got["n_kept"].cpu()[0]) == n and int(got["n_cand"].cpu()[0]) == len(rows)
    assert np.array_equal(got["cand_row"].cpu().numpy(), np.concatenate([rows, [-1, -1]]))
    assert np.array_equal(got["slot_unit"].cpu().numpy(), kept) and np.array_equal(got["stage1_row"].cpu().numpy(), res["stage1_row"])
    for k in BATCH_KEYS + ("lens",):
        g = lk.out[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and torch.equal(g.cpu(), want[k].cpu()), k
    assert sorted(got["batch"].keys()) == sorted(BATCH_KEYS)
    for k in ("dets", "valid", "keep", "cnt"):
        assert got[k].dtype == res[k].dtype and got[k].shape == res[k].shape and torch.equal(got[k].cpu(), res[k].cpu()), k
    for a, w in zip(got["stage1"], s1):
        assert torch.equal(a.cpu(), w.cpu())
    assert int(got["cnt"].sum()) > 0 and int(lk.draws.state.cpu()[0]) == 1
    assert got["dets"] is lk.res["dets"] and got["batch"] is lk.batch      # the link's own tensors, the same every call
    # ---- two empty slots and a larger lpad: one more window on the second stride, the other strides as the second stage's own
    # shape rule needs them (L[s + 1] = ceil(L[s] / 2): two more on the first, at least as many as before on the last two)
    B, lpad2 = n + 2, [lpad[0] + 2]
    for s in range(3):
        lpad2.append((lpad2[s] + 1) // 2)
    assert lpad2[1] == lpad[1] + 1 and all(x >= y for x, y in zip(lpad2, lpad))
    D2 = len(rows) + 3
    lk2 = _link(m1, m2, builder, fpts, foff, D2, B, lpad2, L2=L2)
    got2 = lk2.step(dd)
    torch.cuda.synchronize()
    assert int(got2["n_kept"].cpu()[0]) == n and got2["slot_unit"].cpu().numpy().tolist() == kept.tolist() + [D2, D2]
    assert got2["stage1_row"].cpu().numpy().tolist() == rows[kept].tolist() + [-1, -1]
    for k in ("point_cloud", "rot_angle", "ref_center", "one_hot", "rgb_prob"):
        assert torch.equal(lk2.out[k][:n].cpu(), want[k].cpu()), k
    assert lk2.slot_group.cpu().numpy().tolist() == [UG[r // L2] for r in rows[kept]] + [2, 2]
    assert all(torch.isfinite(v).all() for v in got2["batch"].values())
    hand = m2.detect(got2["batch"], unit_group=lk2.slot_group, num_groups=3, **KW)
    torch.cuda.synchronize()
    assert torch.equal(got2["dets"].cpu(), hand[0].cpu()) and torch.equal(got2["valid"].cpu(), hand[1].cpu())
    assert torch.equal(got2["keep"].cpu(), hand[2][:2].cpu()) and torch.equal(got2["cnt"].cpu(), hand[3][:2].cpu())
    keep2, cnt2 = got2["keep"].cpu().numpy(), got2["cnt"].cpu().numpy()
    assert got2["keep"].shape == (2, 6) and cnt2.sum() > 0
    assert all((0 <= keep2[g, :cnt2[g]]).all() and (keep2[g, :cnt2[g]] // lpad2[1] < n).all() for g in range(2))
    with pytest.raises(ValueError, match="bit 0") as e:                     # the draws' own bit: an empty slot has no row either
        lk2.check()
    assert not any("bit %d" % i in str(e.value) for i in (1, 2, 5, 6, 7, 8, 9)) and int(lk2.status.cpu()[0]) == 0
    lk2.check()


class _Canned:
    """A first stage that returns a prepared (dets, valid, keep, cnt): what CascadeLink asks of stage1 is .training and .detect."""
    training = False

    def __init__(self, dets, keep, cnt):
        self.out = (dets, torch.ones((dets.shape[0],), dtype=torch.int32, device="cuda"), keep, cnt)

    def detect(self, data_dicts, **kw):
        return tuple(x.clone() for x in self.out)


def test_a_first_stage_that_keeps_nothing():
    m1, m2, builder, dd = _stages()
    L2 = int(dd["center_ref2"].shape[2])
    dets = _dev(_dets(4 * L2, 3))
    stub = _Canned(dets, torch.full((2, 6), -1, dtype=torch.int32, device="cuda"), torch.zeros((2,), dtype=torch.int32, device="cuda"))
    fpts = _dev(np.random.RandomState(2).uniform(-5, 30, (5000, 4)).astype(np.float32))
    lk = _link(stub, m2, builder, fpts, [0, 4500, 5000], 5, 3, BIG, L2=L2)
    lk.slot_unit.fill_(0)                                                   # (every output is written: nothing of these survives)
    lk.n_kept.fill_(-7)
    got = lk.step(dd)
    torch.cuda.synchronize()
    assert int(got["n_kept"].cpu()[0]) == 0 and int(got["n_cand"].cpu()[0]) == 0 and not got["cnt"].cpu().numpy().any()
    assert (got["slot_unit"].cpu().numpy() == 5).all() and (got["stage1_row"].cpu().numpy() == -1).all()
    assert (got["cand_row"].cpu().numpy() == -1).all() and (lk.slot_group.cpu().numpy() == 2).all()
    assert int(lk.status.cpu()[0]) == 0                                     # no bit of the link's own: this is the normal case
    assert all(torch.isfinite(v).all() for v in got["batch"].values()) and torch.isfinite(got["dets"]).all()
    assert not lk.points.cpu().numpy().any() and not lk.counts.cpu().numpy().any() and (lk.off.cpu().numpy()[:3] == lk.capacity).all()
    with pytest.raises(ValueError, match="bit 0") as e:                     # (the draws' word alone: every slot is empty)
        lk.check()
    assert not any("bit %d" % i in str(e.value) for i in (1, 2, 5, 6, 7, 8, 9))
    # a group that overflowed and more kept rows than candidates: said, the kept rows are the first D in order
    stub.out[2][0, :4] = torch.tensor([3, 1, 2, 0], dtype=torch.int32)
    stub.out[2][1, :3] = torch.tensor([2 * L2, 2 * L2 + 1, 3 * L2], dtype=torch.int32)
    stub.out[3].copy_(torch.tensor([4, 3], dtype=torch.int32))
    got = lk.step(dd)
    torch.cuda.synchronize()
    assert got["cand_row"].cpu().numpy().tolist() == [3, 1, 2, 0, 2 * L2, -1] and int(got["n_cand"].cpu()[0]) == 5
    assert lk.cand_group.cpu().numpy().tolist() == [0, 0, 0, 0, 1, 2] and lk.cand_frame.cpu().numpy().tolist() == [0, 0, 0, 0, 1, -1]
    stub.out[3].copy_(torch.tensor([-1, 1], dtype=torch.int32))
    lk.step(dd)
    with pytest.raises(ValueError, match="bit 7") as e:
        lk.check()
    assert "bit 9" in str(e.value) and int(lk.n_cand.cpu()[0]) == 1


def test_captured_step_replays_on_new_first_stage_batches_equal_to_eager_steps():
    """ONE capture of step(); three replays, the first-stage batch tensors and the frustum tables overwritten in place between them;
    every replay equals the eager step() of a twin link on the same seed and the same data, bit for bit; the draw advances."""
    m1, m2, builder, dd = _stages()
    L2 = int(dd["center_ref2"].shape[2])
    s1, rows, fpts, foff = _first_stage(m1, dd)
    src, twin = (_link(m1, m2, builder, fpts, foff, 12, 12, BIG, L2=L2) for _ in range(2))     # (a slot for every candidate: nothing dropped)
    base = {k: v.clone() for k, v in dd.items()}
    units = [np.asarray(x) for x in (FRUSTUM_FRAME, [builder.classes.index(t) for t in TYPES], UG)]
    orders = ([1, 0, 3, 2], [3, 2, 1, 0], [0, 1, 2, 3])                     # (groups stay whole: the frustums of a group trade places)

    def write(order):
        idx = torch.tensor(order, device="cuda")
        for k in dd:
            dd[k].copy_(base[k].index_select(0, idx))
        for lk in (src, twin):
            for dst, u in zip((lk.unit_frame, lk.unit_class, lk.unit_group), units):
                dst.copy_(_dev(u[order].astype(np.int32)))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        src.step(dd)                                                        # warm-up on a side stream: step 0
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step(dd)
    torch.cuda.synchronize()
    assert int(src.draws.state.cpu()[0]) == 1                               # capturing runs nothing
    twin.step(dd)
    seen = []
    for r, order in enumerate(orders):
        write(order)
        graph.replay()
        torch.cuda.synchronize()
        got = _host(out)
        gb = _host(out["batch"])
        want_out = twin.step(dd)
        torch.cuda.synchronize()
        want, wb = _host(want_out), _host(want_out["batch"])
        assert int(src.draws.state.cpu()[0]) == 2 + r == int(twin.draws.state.cpu()[0])
        for k in ("dets", "valid", "keep", "cnt", "stage1_row", "n_kept", "slot_unit", "cand_row", "n_cand"):
            assert torch.equal(got[k], want[k]), (r, k)
        for k in wb:
            assert torch.equal(gb[k], wb[k]), (r, k)
        for a, w in zip(out["stage1"], want_out["stage1"]):
            assert torch.equal(a.cpu(), w.cpu()), r
        assert int(got["n_kept"][0]) >= 2 and int(got["cnt"].sum()) > 0
        seen.append((out["stage1"][0].cpu().clone(), gb))
    assert not torch.equal(seen[0][1]["point_cloud"], seen[2][1]["point_cloud"]) and not torch.equal(seen[0][0], seen[2][0])
    assert int(src.status.cpu()[0]) == 0 and int(twin.status.cpu()[0]) == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    from frustum_convnet_amd import cascade
    m1, m2, builder, dd = _stages()
    fpts = _dev(np.random.RandomState(2).uniform(-5, 30, (9000, 4)).astype(np.float32))
    off = [0, 4500, 9000]
    lk = _link(m1, m2, builder, fpts, off, 12, 8, BIG, L2=10)
    assert lk.S == 2 and lk.frames[0].data_ptr() == fpts.data_ptr()         # held, not copied
    for kw in (dict(frame_off=[0, 9000, 700]), dict(frame_off=[0]), dict(frame_off=[0, 700, 10 ** 6]),
               dict(frame_points=fpts.double()), dict(frame_points=fpts[:, :2].contiguous()),
               dict(frame_points=fpts[::2]), dict(frame_points=fpts.cpu().numpy()),
               dict(B=0), dict(B=13), dict(D=0), dict(D=2049, B=8), dict(B1=0), dict(L2=0), dict(G=0), dict(G=65537),
               dict(top_k=0), dict(top_k=4097), dict(capacity=0), dict(lpad=(64, 32, 16)), dict(lpad=(64, 32, 16, 0)), dict(lpad=(64, 32, 16, 9)), dict(lpad=(65, 32, 16, 8)),
               dict(ratio=0.0), dict(thresh=float("nan")), dict(method="both"),
               dict(units=([0, 0, 1], TYPES[:3], UG[:3])), dict(units=([0, 0, 1, 2], TYPES, UG)), dict(units=([0, 0, 1, -1], TYPES, UG)),
               dict(units=(FRUSTUM_FRAME, ["Tram"] + TYPES[1:], UG)), dict(units=(FRUSTUM_FRAME, TYPES, [0, 0, 1, 2])),
               dict(units=(FRUSTUM_FRAME, TYPES, None))):
        kw = dict(kw)
        B, D, lpad = kw.pop("B", 8), kw.pop("D", 12), kw.pop("lpad", BIG)
        kw.setdefault("L2", 10)
        with pytest.raises(ValueError):
            _link(m1, m2, builder, kw.pop("frame_points", fpts), kw.pop("frame_off", off), D, B, lpad, **kw)
    with pytest.raises(ValueError):                                         # D * S beyond the plan's segments
        _link(m1, m2, builder, torch.zeros((4096 * 40, 4), dtype=torch.float32, device="cuda"), [0, 4096 * 40], 2048, 8, BIG, L2=10,
              units=([0] * 4, TYPES, UG))
    m1.train()
    with pytest.raises(ValueError, match="eval"):
        _link(m1, m2, builder, fpts, off, 12, 8, BIG, L2=10)
    m1.eval()
    m2.train()
    with pytest.raises(ValueError, match="eval"):
        _link(m1, m2, builder, fpts, off, 12, 8, BIG, L2=10)
    m2.eval()
    stub = _Canned(_dev(_dets(4 * 7, 3)), torch.full((2, 6), -1, dtype=torch.int32, device="cuda"), torch.zeros((2,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="first-stage batch"):              # a batch of another L2 than the link was built for
        _link(stub, m2, builder, fpts, off, 12, 8, BIG, L2=10).step(dd)
    _link(m1, m2, builder, fpts, off, 4, 4, BIG, L2=10, G=4, units=(FRUSTUM_FRAME, TYPES, None))


def test_entry_refusals_write_nothing():
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    # ---- the candidate table
    o = {k: torch.full((8,), -7, dtype=dt, device="cuda") for k, dt in CAND_OUT}
    n, status = torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ins = [_dev(np.asarray(KEEP3, np.int32)), _dev(np.asarray([2, 1, 3], np.int32)), _dev(UFRAME), _dev(UCLASS), _dev(UGROUP), _dev(_dets())]
    good = [_p(ins[0]), _p(ins[1]), 3, 6, 5, _p(ins[2]), _p(ins[3]), _p(ins[4]), 4, _p(ins[5]), 20, 8] + [_p(o[k]) for k, _ in CAND_OUT] + [_p(n), _p(status), s]
    for i in (0, 1, 5, 6, 7, 9, 12, 13, 14, 15, 16, 17, 18):
        bad = list(good)
        bad[i] = None
        assert L.fcn_cascade_candidates(*bad) == BADARG, i
    for i, v, rc in ((2, 0, BADARG), (3, 0, BADARG), (4, 0, BADARG), (8, 0, BADARG), (10, 0, BADARG), (11, 0, BADARG), (2, -1, BADARG),
                     (2, 65537, LIMIT), (11, 2049, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_cascade_candidates(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o.values()) and int(n.cpu()[0]) == -7 and int(status.cpu()[0]) == -7
    status.zero_()
    assert L.fcn_cascade_candidates(*good) == 0
    torch.cuda.synchronize()
    assert int(n.cpu()[0]) == 6 and int(status.cpu()[0]) == 0
    # ---- the plan
    cnt, psz = _counts()
    D, S, B = 12, 3, 4
    po = {k: torch.full(shape(D, S, B), -7, dtype=dt, device="cuda") for k, dt, shape in PLAN_OUT}
    po["status"] = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    pin = (_dev(cnt.astype(np.int32)), _dev(psz))
    st4, lp4 = (ctypes.c_double * 4)(*STRIDES), (ctypes.c_int32 * 4)(*BIG)
    good = [_p(pin[0]), _p(pin[1]), st4, lp4, D, S, B, 10000] + [_p(po[k]) for k in ("slot_unit", "n_kept", "seg_off", "off", "counts", "status")] + [s]
    for i in (0, 1, 2, 3, 8, 9, 10, 11, 12, 13):
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_detect_plan(*bad) == BADARG, i
    for i, v, rc in ((4, -1, BADARG), (5, 0, BADARG), (6, 0, BADARG), (7, -1, BADARG), (4, 2049, LIMIT), (6, 2049, LIMIT), (5, 5462, LIMIT),
                     (3, (ctypes.c_int32 * 4)(64, 0, 16, 8), BADARG), (2, (ctypes.c_double * 4)(0.1, 0.2, 0.0, 0.8), BADARG),
                     (2, (ctypes.c_double * 4)(0.1, float("nan"), 0.4, 0.8), BADARG)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_refine_detect_plan(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in po.values())
    # ---- count and fill: the reading entries' argument refusals, and S
    sc = _scene(3)
    t = _tensors(sc)
    w = {"seg_cnt": torch.full((7, 1), -7, dtype=torch.int32, device="cuda"), "pred_box3d": torch.full((7, 8, 3), -7.0, dtype=torch.float64, device="cuda"),
         "pred_angle": torch.full((7,), -7.0, dtype=torch.float64, device="cuda"), "pred_size": torch.full((7, 3), -7.0, dtype=torch.float64, device="cuda")}
    good = [_p(t["pts"]), _p(t["off"]), 3, 3, _p(t["dets"]), 10, _p(t["crow"]), _p(t["cframe"]), 7, 1.2, 1] + [_p(w[k]) for k in w] + [s]
    for i in (0, 1, 4, 6, 7, 11, 12, 13, 14):
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_detect_count(*bad) == BADARG, i
    for i, v in ((3, 2), (10, 0), (10, -1), (8, -1), (2, -1), (5, -1), (8, 65536)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_refine_detect_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in w.values())
    soff = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    goodf = good[:11] + [_p(soff), _p(out), s]
    for i in (0, 1, 4, 6, 7, 11, 12):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_refine_detect_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (10, 0), (8, -1), (2, -1), (8, 65536)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_refine_detect_fill(*bad) == BADARG, (i, v)
    assert L.fcn_refine_detect_fill(*goodf) == 0                            # (every slice empty: nothing to write)
    zero = list(good)
    zero[2] = 0                                                             # F = 0: the counts are zeroed, nothing else is written
    assert L.fcn_refine_detect_count(*zero) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and not w["seg_cnt"].cpu().numpy().any() and (w["pred_size"].cpu().numpy() == -7.0).all()


def test_check_raises_names_the_bits_and_clears():
    m1, m2, builder, dd = _stages()
    fpts = _dev(np.random.RandomState(2).uniform(-5, 30, (5000, 4)).astype(np.float32))
    lk = _link(m1, m2, builder, fpts, [0, 4500, 5000], 12, 8, BIG, L2=10)
    lk.check()
    lk.status.fill_(R.ST_ROWS | R.ST_TRUNC)
    with pytest.raises(ValueError) as e:
        lk.check()
    assert "bit 7" in str(e.value) and "bit 2" in str(e.value) and not any("bit %d" % i in str(e.value) for i in (0, 1, 5, 6, 8, 9))
    lk.check()                                                              # cleared
    for bit, name in ((R.ST_MANY, "bit 8"), (R.ST_GROUP, "bit 9"), (R.ST_WIDE, "bit 5"), (R.ST_WIDTH, "bit 6")):
        lk.status.fill_(bit)
        with pytest.raises(ValueError, match=name):
            lk.check()
        assert int(lk.status.cpu()[0]) == 0
    lk.draws.status.fill_(1)
    with pytest.raises(ValueError, match="bit 0"):
        lk.check()
    assert int(lk.draws.status.cpu()[0]) == 0
    lk.check()
