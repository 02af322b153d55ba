"""-m gpu: the capturable refine-stage training input -- fcn_box3d_jitter_draw, fcn_refine_train_match / _count / _plan / _fill
(csrc/refine_plan.h) through the C-ABI against the numpy restatement of tests/refine_plan_ref.py (pinned to the host path by
tests/test_refine_plan_referee.py), and cascade.RefineTrainSource against the host path it replaces (match_detections,
refine_training_candidates on the step's jitter read back, RefineInputBuilder.build_device_train), against the reference's recorded
run, under a captured graph, and through one training step.  The scene is that of tests/test_gpu_refine_label.py
(tests/golden/refine_label.npz: three frames, S = 3, A = 3); tests/test_emu_refine_plan.py runs the same functions on the host
emulation of the kernels (all but the graph capture)."""
import ctypes

import numpy as np
import pytest
import torch

import draws_ref
import refine_plan_ref as R
from test_gpu_cascade import BADARG, _bits, _dev, _p
from test_gpu_refine_label import A, IOU_BAR, OUT_ORDER, _builder, _check_boxes, _common, _outputs, _rows, _scene, _tensors
from test_gpu_refine_label import _count as _label_count
from test_gpu_refine_label import _fill as _label_fill
from test_gpu_refine_label import _match as _label_match

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
SEED = 20240611
STRIDES = (0.1, 0.2, 0.4, 0.8)
BIG = (64, 32, 16, 8)              # window counts no unit of the scene comes near (widths up to 6.4)


def _guarded(shape, dtype, fill, g=4):
    """A tensor of `shape` as a view into a buffer with g poisoned elements on either side -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device="cuda")
    return buf[g:g + n].view(shape), buf


def _intact(buf, fill, g=4):
    h = buf.cpu()
    return bool((h[:g] == fill).all() and (h[-g:] == fill).all())


# ------------------------------------------------------------------------------------------------ the jitter draw
def _jitter(D, Ax, seed, step, advance):
    from frustum_convnet_amd import _native
    out, obuf = _guarded((D, Ax, 7), torch.float64, -7.0)
    state = _dev(np.asarray([step], dtype=np.int64))
    rc = _native.lib().fcn_box3d_jitter_draw(D, Ax, seed, _p(state), advance, _p(out), _native.current_stream())
    torch.cuda.synchronize()
    assert _intact(obuf, -7.0)
    return rc, out.cpu().numpy(), int(state.cpu()[0])


@pytest.mark.parametrize("step", [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize("D,Ax", [(1, 1), (1, 64), (300, 3)])
def test_jitter_draw_equals_the_restatement_bit_for_bit(D, Ax, step):
    want = R.jitter_draw(SEED, step, D, Ax)
    for advance in (0, 1):
        rc, got, state = _jitter(D, Ax, SEED, step, advance)
        assert rc == 0 and state == step + advance
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, Ax, step, advance)
    assert (got >= 0).all() and (got < 1).all()


# ------------------------------------------------------------------------------------------------ the plan
PLAN_OUT = (("slot_unit", torch.int32, lambda U, S, B: (B,)), ("n_kept", torch.int32, lambda U, S, B: (1,)),
            ("seg_off", torch.int64, lambda U, S, B: (U * S + 1,)), ("off", torch.int64, lambda U, S, B: (B + 1,)),
            ("counts", torch.int64, lambda U, S, B: (B,)))


def _plan(cnt, pos, psz, B, capacity, lpad=BIG, strides=STRIDES):
    """The raw entry on exactly sized inputs and poisoned, guarded outputs -> rc, outputs as numpy, status."""
    from frustum_convnet_amd import _native
    U, S = cnt.shape
    o = {k: _guarded(shape(U, S, B), dt, -7) for k, dt, shape in PLAN_OUT}
    status, sbuf = _guarded((1,), torch.int32, 0)
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)), _dev(np.asarray(psz, dtype=np.float64).reshape(U, 3)))
    rc = _native.lib().fcn_refine_train_plan(_p(ins[0]), _p(ins[1]), _p(ins[2]), (ctypes.c_double * 4)(*strides),
                                             (ctypes.c_int32 * 4)(*lpad), U, S, B, capacity, *[_p(o[k][0]) for k, _, _ in PLAN_OUT],
                                             _p(status), _native.current_stream())
    torch.cuda.synchronize()
    assert all(_intact(buf, -7) for _, buf in o.values()) and _intact(sbuf, 0)
    return rc, {k: v.cpu().numpy() for k, (v, _) in o.items()}, int(status.cpu()[0])


def _plan_equals(cnt, pos, psz, B, capacity, lpad=BIG, strides=STRIDES):
    """Every output is poisoned first, so equality with the restatement also says that every output is written."""
    rc, got, status = _plan(cnt, pos, psz, B, capacity, lpad, strides)
    slot_unit, n, seg_off, off, counts, st = R.plan(cnt, pos, psz, strides, lpad, B, capacity)
    assert rc == 0
    for k, want in (("slot_unit", slot_unit), ("seg_off", seg_off), ("off", off), ("counts", counts)):
        assert np.array_equal(got[k], want), k
    assert int(got["n_kept"][0]) == n and status == st
    return slot_unit, n, seg_off, off, counts, st


def _counts(U=12, S=3, seed=0):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(0, 900, (U, S))
    pos = np.minimum(cnt, rs.randint(0, 40, (U, S)))
    pos[[1, 6]] = 0                                                         # no positive: rejected
    cnt[3, 1] = 0
    psz = np.stack([rs.uniform(3, 5, U), rs.uniform(0.5, 2.5, U), rs.uniform(1, 2, U)], 1)
    return cnt, pos, psz


@pytest.mark.parametrize("B", [4, 10, 12])
def test_plan_equals_the_restatement(B):
    """B below, equal to and above the 10 survivors; a capacity that cuts inside a segment, at a unit boundary, and 0."""
    cnt, pos, psz = _counts()
    survivors = [u for u in range(12) if u not in (1, 6)]
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, B, 1 << 40)
    assert slot_unit[:n].tolist() == survivors[:B] and n == min(B, 10) and st == (R.ST_FEW if B == 12 else 0)
    held = survivors[:B]
    total = int(cnt[held].sum())
    assert off[B] == total and (off[n:B] == 1 << 40).all() and (slot_unit[n:] == 12).all()
    assert np.array_equal(counts[:n], cnt[held].sum(1)) and not counts[n:].any()
    # one row short: bit 2, the last slot's STORED count one lower; exactly enough: no bit
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, B, total - 1)
    assert st & R.ST_TRUNC and off[B] == total - 1 and counts[n - 1] == cnt[held[-1]].sum() - 1 and (off[n:B] == total - 1).all()
    assert not _plan_equals(cnt, pos, psz, B, total)[5] & R.ST_TRUNC
    # inside the first segment of the second unit; at the boundary behind the first unit
    first = int(cnt[held[0]].sum())
    assert cnt[held[1], 0] > 5
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, B, first + 5)
    assert st & R.ST_TRUNC and counts[:3].tolist() == [first, 5, 0] and off[1] == first and off[2] == first + 5
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, B, first)
    assert st & R.ST_TRUNC and counts[:2].tolist() == [first, 0] and not counts[2:].any() and n == min(B, 10)
    # no room at all; no survivor at all
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, B, 0)
    assert st & R.ST_TRUNC and not counts.any() and not off.any() and not seg_off.any()
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos * 0, psz, B, 1000)
    assert n == 0 and st == R.ST_FEW and not seg_off.any() and off.tolist() == [1000] * B + [0] and (slot_unit == 12).all()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("U", [255, 256, 257])
def test_plan_where_a_threads_run_goes_from_one_unit_to_two(U, S):
    """The run-per-thread split is csrc/slot_plan.h's, shared by every plan: over 256 threads, 255 and 256 units are runs of one
    (the last thread's empty, then not), 257 units are runs of two with threads 129.. owning nothing.  B = U, some units rejected,
    a capacity one row short of the total."""
    rs = np.random.RandomState(4 * U + S)
    cnt = rs.randint(0, 900, (U, S))
    pos = np.minimum(cnt, rs.randint(0, 40, (U, S))) * (rs.uniform(size=(U, 1)) < 0.7)
    psz = np.stack([rs.uniform(3, 5, U), rs.uniform(0.5, 2.5, U), rs.uniform(1, 2, U)], 1)
    total = int(R.plan(cnt, pos, psz, STRIDES, BIG, U, 1 << 40)[2][-1])
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, U, total - 1)
    assert 0 < n < U and st == R.ST_FEW | R.ST_TRUNC and seg_off[-1] == total - 1 and counts.sum() == total - 1


def test_plan_at_its_smallest_and_at_its_limits():
    one = (np.asarray([[7]]), np.asarray([[2]]), np.asarray([[4.0, 1.6, 1.5]]))
    assert _plan_equals(*one, 1, 100)[3].tolist() == [0, 7]                 # U = S = B = 1
    assert _plan_equals(one[0], one[1] * 0, one[2], 1, 100)[5] == R.ST_FEW
    # more units than the workgroup has threads, a count that is no multiple of it, S = 5, sums beyond 2^31
    rs = np.random.RandomState(1)
    U, S = 777, 5
    cnt = rs.randint(0, 2 ** 31 - 1, (U, S))
    pos = (rs.randint(0, 2, (U, S)) * (rs.uniform(size=(U, 1)) < 0.6)).astype(np.int64)
    psz = np.tile(np.asarray([[4.0, 1.6, 1.5]]), (U, 1))
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, 300, 1 << 50)
    assert n == 300 and st == 0 and seg_off[-1] > 2 ** 33 and (np.diff(slot_unit) > 0).all()
    _plan_equals(cnt, pos, psz, 700, 1 << 36)                               # fewer than B and truncated at once
    from frustum_convnet_amd import cascade
    max_u, max_segs = cascade.RefineTrainSource.limits()
    assert (max_u, max_segs) == (2048, 65536)
    U, S = max_u, max_segs // max_u                                         # the largest plan: 2048 units of 32 segments
    assert S == 32
    cnt = rs.randint(0, 50, (U, S))
    pos = (rs.uniform(size=(U, S)) < 0.02).astype(np.int64)
    psz = np.tile(np.asarray([[4.0, 1.6, 1.5]]), (U, 1))
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, psz, U, 1 << 40)
    assert 500 < n < U and st == R.ST_FEW


def test_plan_widths():
    cnt, pos, psz = _counts()
    # 0, negative, NaN and inf on units with positives: bit 6, no slot; the same widths on the units without positives: no bit
    bad = psz.copy()
    bad[[0, 2, 5, 9], 1] = [0.0, -1.5, np.nan, np.inf]
    slot_unit, n, seg_off, off, counts, st = _plan_equals(cnt, pos, bad, 12, 1 << 40)
    assert st == R.ST_WIDTH | R.ST_FEW and slot_unit[:n].tolist() == [3, 4, 7, 8, 10, 11]
    for w in (0.0, -1.5, np.nan, np.inf, 1e300):
        quiet = psz.copy()
        quiet[[1, 6], 1] = w
        assert _plan_equals(cnt, pos, quiet, 4, 1 << 40)[5] == 0, w
        loud = psz.copy()
        loud[4, 1] = w
        slot_unit, n, _, _, _, st = _plan_equals(cnt, pos, loud, 4, 1 << 40)
        assert st == (R.ST_WIDE if w == 1e300 else R.ST_WIDTH) and 4 not in slot_unit.tolist(), w       # (1e300: compared in fp64)
    # ceil(w / stride) == lpad[s] passes, one window over does not: on each of the four strides alone
    one = (np.asarray([[3, 4]]), np.asarray([[0, 1]]))
    for s, stride in enumerate(STRIDES):
        for k in (1, 3, 8):
            lpad = [1 << 20] * 4
            lpad[s] = k
            on = k * stride                                                 # (k * stride rounds: walk to the last width of k windows)
            while R.windows(on, stride) > k:
                on = np.nextafter(on, 0.0)
            while R.windows(np.nextafter(on, 100.0), stride) <= k:
                on = np.nextafter(on, 100.0)
            over = np.nextafter(on, 100.0)
            assert R.windows(on, stride) == k and R.windows(over, stride) == k + 1 and abs(on - k * stride) < 1e-12
            assert _plan_equals(*one, [[4.0, on, 1.5]], 1, 100, lpad=lpad)[5] == 0, (s, k)
            slot_unit, n, seg_off, off, counts, st = _plan_equals(*one, [[4.0, over, 1.5]], 1, 100, lpad=lpad)
            assert st == R.ST_WIDE | R.ST_FEW and n == 0 and slot_unit.tolist() == [1] and off.tolist() == [100, 0], (s, k)
    # other strides than the fixture's
    _plan_equals(cnt, pos, psz, 6, 1 << 40, lpad=(9, 5, 3, 2), strides=(0.25, 0.5, 1.0, 2.0))


# ------------------------------------------------------------------------------------------------ the no-read entries
def _train_match(t, thresh=0.5):
    from frustum_convnet_amd import _native
    D = t["crow"].numel()
    gidx = torch.full((D,), -7, dtype=torch.int32, device="cuda")
    best = torch.full((D,), -7.0, dtype=torch.float32, device="cuda")
    rc = _native.lib().fcn_refine_train_match(_p(t["dets"]), t["dets"].shape[0], _p(t["crow"]), _p(t["cframe"]), D, _p(t["gt"]),
                                              t["gt"].shape[0], _p(t["goff"]), t["goff"].numel() - 1, thresh, _p(gidx), _p(best),
                                              _native.current_stream())
    torch.cuda.synchronize()
    return rc, gidx.cpu().numpy(), best.cpu().numpy()


def _train_count(t, S):
    from frustum_convnet_amd import _native
    c = _common(t, S)
    o = _outputs(c[8] * c[13], S)
    rc = _native.lib().fcn_refine_train_count(*c, *[_p(o[k]) for k in OUT_ORDER], _native.current_stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _train_fill(t, S, seg_counts, front=0, guard=5):
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    soff = (front + np.concatenate([[0], np.cumsum(np.asarray(seg_counts).reshape(-1))])).astype(np.int64)
    out = torch.full((int(soff[-1]) + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    soff_d = _dev(soff)
    rc = _native.lib().fcn_refine_train_fill(*_common(t, S), _p(soff_d), _p(out), _native.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), soff


@pytest.mark.parametrize("stride", [4, 5])
def test_no_read_entries_equal_the_reading_entries_bit_for_bit(stride):
    sc = _scene(stride)
    S, ref = sc["S"], sc["ref"]
    t = _tensors(sc)
    rc, gidx, best = _label_match(t)
    rc2, gidx2, best2 = _train_match(t)
    assert rc == 0 and rc2 == 0 and np.array_equal(gidx, gidx2) and np.array_equal(_bits(best), _bits(best2)) and (gidx >= 0).sum() == 6
    rc, want = _label_count(t, S)
    rc2, got = _train_count(t, S)
    assert rc == 0 and rc2 == 0 and all(got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() for k in want)
    assert np.array_equal(got["scnt"], ref["seg_cnt"]) and got["scnt"].sum() > 1000
    counts = got["scnt"].copy()
    counts[3] = 0                                                           # a unit granted nothing
    counts[4 * A, 1] -= 10                                                  # a segment granted too little
    rc, wbuf, soff = _label_fill(t, S, counts, front=4)
    rc2, buf, soff2 = _train_fill(t, S, counts, front=4)
    assert rc == 0 and rc2 == 0 and np.array_equal(soff, soff2) and np.array_equal(_bits(buf), _bits(wbuf))
    assert (buf[:4] == -7.0).all() and (buf[soff[-1]:] == -7.0).all() and len(buf) == soff[-1] + 5
    # S too small for the longest frame is the caller's duty now: the reading entry refuses, the new one searches S segments
    rc, short = _train_count(t, S - 1)
    assert rc == 0 and np.array_equal(short["scnt"], ref["seg_cnt"][:, :S - 1]) and _label_count(t, S - 1)[0] == BADARG


@pytest.mark.parametrize("what", ["row_high", "row_negative", "frame_high", "frame_negative", "gt_high"])
def test_out_of_range_candidate_is_skipped_silently_and_never_dereferenced(what):
    """Exactly sized device buffers (nothing beyond them can be read), sentinel-filled outputs: the bad candidate's counts are 0,
    nothing else of it is written, the others are processed, every call returns 0."""
    sc = _scene(4)
    S, ref, g = sc["S"], sc["ref"], sc["g"]
    crow, cframe, cgt = sc["crow"].copy(), sc["cframe"].copy(), sc["cgt"].copy()
    bad = 4                                                                 # the candidate with rows in every segment
    if what.startswith("row"):
        crow[bad] = 10 if what == "row_high" else -(2 ** 31)                # R = 10
    elif what.startswith("frame"):
        cframe[bad] = 3 if what == "frame_high" else -1                     # F = 3
    else:
        cgt[bad] = 7                                                        # G = 7
    t = _tensors(sc, crow=crow, cframe=cframe, cgt=cgt)
    if what != "gt_high":
        rc, gidx, best = _train_match(t)
        want = g["ref_gt_idx"].copy()
        want[bad] = -1
        assert rc == 0 and np.array_equal(gidx, want) and best[bad] == 0.0
    rc, o = _train_count(t, S)
    assert rc == 0
    units = np.arange(bad * A, (bad + 1) * A)
    want_c, want_p = ref["seg_cnt"].copy(), ref["seg_pos"].copy()
    want_c[units], want_p[units] = 0, 0
    assert np.array_equal(o["scnt"], want_c) and np.array_equal(o["spos"], want_p)
    for k in OUT_ORDER[2:]:
        assert (o[k][units] == -7.0).all(), k
    _check_boxes(o, ref, g, [u for u in range(len(crow) * A) if sc["cgt"][u // A] >= 0 and u // A != bad])
    # the fill is granted the bad candidate's reference rows: it stores none of them
    rc, buf, soff = _train_fill(t, S, ref["seg_cnt"])
    assert rc == 0 and (buf[soff[-1]:] == -7.0).all()
    for u in range(len(crow) * A):
        rows = buf[soff[u * S]:soff[(u + 1) * S]]
        if u // A == bad:
            assert (rows == -7.0).all() and len(rows) > 100, u
        else:
            assert np.array_equal(_bits(rows), _bits(_rows(sc, [u]))), u


# ------------------------------------------------------------------------------------------------ RefineTrainSource
def _table(sc):
    """The scene's candidates as the resident table of the source: R = 8 rows, their frames and their types."""
    dets = np.ascontiguousarray(sc["dets"][sc["crow"]])
    return dets, sc["cframe"].copy(), [str(x) for x in sc["g"]["types"]]


def _source(sc, B, lpad=BIG, D=8, Ax=A, seed=SEED, builder=None, capacity=40000, **kw):
    from frustum_convnet_amd import cascade
    dets, dframe, types = _table(sc)
    over = {k: kw.pop(k) for k in ("dets", "det_frame", "det_types", "off", "gt", "goff") if k in kw}
    return cascade.RefineTrainSource(_dev(sc["pts"]), over.get("off", sc["off"]), over.get("dets", _dev(dets)),
                                     over.get("det_frame", dframe), over.get("det_types", types), over.get("gt", sc["gt"]),
                                     over.get("goff", sc["goff"]), builder or _builder(64, random_flip=True, random_shift=True),
                                     B, D, Ax, capacity, lpad, seed, **kw)


def _host_path(sc, src, builder, step, seed):
    """The existing path on the step's picks and jitter read back: match_detections + refine_training_candidates +
    build_device_train with the restated per-sample draws of `step` -> (gt_idx, best_iou, sel, batch)."""
    from frustum_convnet_amd import cascade
    dets, dframe, types = _table(sc)
    crow = src.cand_row.cpu().numpy().reshape(-1)
    jit = None if src.jitter is None else src.jitter.cpu().numpy()
    d8 = _dev(dets)
    gidx, best = cascade.match_detections(d8, crow, dframe[crow], sc["gt"], sc["goff"], src.thresh)
    sel = cascade.refine_training_candidates(_dev(sc["pts"]), sc["off"], d8, crow, dframe[crow], gidx, sc["gt"], jitter=jit)
    if len(sel["kept"]) == 0:
        return gidx, best, sel, None
    d = draws_ref.draw(seed + 2, step, sel["counts"], builder.npoints, builder.random_flip, builder.random_shift)
    return gidx, best, sel, builder.build_device_train(sel, [types[r] for r in crow], draws=d[:3])


def _spare_rows(src, builder, n):
    """The batch rows of the empty slots n..B-1: RefineInputBuilder.launch on the spare entry -- a unit box at the origin, its
    label box equal to it, one all-zero row of points -- with the slots' own coin and normal."""
    B, ps = src.B, src.ps
    E = B - n
    f64 = dict(dtype=torch.float64, device="cuda")
    hx, hz = np.asarray([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5, np.asarray([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
    hy = np.asarray([1, 1, 1, 1, -1, -1, -1, -1]) * 0.5
    corners = _dev(np.tile(np.stack([hx, hy, hz], 1).reshape(1, 24), (E, 1)))
    t = {"raw": torch.zeros((1, ps), dtype=torch.float32, device="cuda"), "off": torch.zeros((E + 1,), dtype=torch.int64, device="cuda"),
         "choice": torch.zeros((E, builder.npoints), dtype=torch.int32, device="cuda"),
         "pcorners": corners, "pangle": torch.zeros((E,), **f64), "psize": torch.ones((E, 3), **f64),
         "corners": corners.clone(), "heading": torch.zeros((E,), **f64), "size": torch.ones((E, 3), **f64),
         "coin": src.t["coin"][n:].clone(), "normal": src.t["normal"][n:].clone()}
    return builder.launch(t, builder.alloc(E, src.lpad), ps, src.lpad)


@pytest.mark.parametrize("rel,stride", [(-3, 4), (0, 4), (4, 4), (-3, 5), (0, 5), (4, 5)])
def test_step_equals_the_existing_path_on_the_same_boxes(rel, stride):
    """B = K + rel slots for the K units the existing path keeps at step 0; lpad = that call's _lpad(widths).  A probe source at
    generous window counts reads the step's picks and jitter off the device first (the same seed: the same step).  One step per
    source: the next step's jitter gives other widths, so the existing path's batch maximum would no longer be lpad."""
    sc = _scene(stride)
    b = _builder(64, random_flip=True, random_shift=True)
    probe = _source(sc, 4, builder=b)
    probe.step()
    torch.cuda.synchronize()
    _, _, sel, _ = _host_path(sc, probe, b, 0, SEED)
    K = len(sel["kept"])
    lpad = b._lpad(sel["pred_size"][:, 1].cpu().numpy())
    assert K >= 6 and all(x < y for x, y in zip(lpad, BIG))
    B = K + rel
    src = _source(sc, B, lpad=lpad, builder=b)
    assert (src.S, src.D, src.A, src.U, src.R) == (3, 8, 3, 24, 8)
    step = 0
    got = src.step()
    torch.cuda.synchronize()
    crow = src.cand_row.cpu().numpy().reshape(-1)
    assert np.array_equal(crow, draws_ref.choice_row(SEED, step, 0, 8, 8)) and sorted(crow.tolist()) == list(range(8))
    jit = src.jitter.cpu().numpy()
    assert np.array_equal(jit.view(np.uint64), R.jitter_draw(SEED + 1, step, 8, A).view(np.uint64))
    gidx, best, sel, want = _host_path(sc, src, b, step, SEED)
    assert torch.equal(src.gt_idx.cpu(), gidx.cpu()) and torch.equal(src.best_iou.cpu(), best.cpu())
    Ks = len(sel["kept"])
    n = min(Ks, B)
    slot_unit = src.slot_unit.cpu().numpy()
    assert int(src.n_kept.cpu()[0]) == n and np.array_equal(slot_unit[:n], sel["kept"][:n]) and (slot_unit[n:] == 24).all()
    assert sorted(got.keys()) == sorted(want.keys()) and "lens" in got and "one_hot" in got and "cls_label" in got
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape[1:] == want[k].shape[1:] and got[k].shape[0] == B, k
        assert torch.equal(got[k][:n].cpu(), want[k][:n].cpu()), (step, k)
    off = src.off.cpu().numpy()
    assert np.array_equal(off[:n], sel["off"].cpu().numpy()[:n]) and (off[n:B] == src.capacity).all()
    assert np.array_equal(src.counts.cpu().numpy()[:n], sel["counts"][:n])
    if n == B:
        src.check()
    else:                                                               # empty slots: flagged by the plan and by the draw
        with pytest.raises(ValueError, match="bit 1") as e:
            src.check()
        assert "bit 0" in str(e.value) and not any("bit %d" % i in str(e.value) for i in (2, 5, 6))
        src.check()                                                     # cleared
        spare = _spare_rows(src, b, n)
        torch.cuda.synchronize()
        for k in spare:
            assert torch.equal(got[k][n:].cpu(), spare[k].cpu()), (step, k)
        assert not got["size_class"][n:].any() and torch.equal(got["one_hot"][n:].cpu(), src.eye[0].cpu().expand(B - n, -1))
    assert [int(x.state.cpu()[0]) for x in (src.draws_pick, src.draws_jitter, src.draws_sample)] == [step + 1] * 3
    if rel == 4:
        assert n < B


def test_step_reproduces_the_references_recorded_run():
    """pick=False, jitter = the fixture's table, B = U on the fixture: the checks of test_entry_points_match_the_referee, through
    the source -- the match, the per-segment counts, the jittered boxes, the kept units and their rows."""
    sc = _scene(4)
    ref, g = sc["ref"], sc["g"]
    U = 8 * A
    src = _source(sc, U, pick=False, jitter=sc["jit"], thresh=float(g["meta_thresh"]))
    got = src.step()
    torch.cuda.synchronize()
    assert src.cand_row.cpu().numpy().reshape(-1).tolist() == list(range(8))
    gidx, best = src.gt_idx.cpu().numpy(), src.best_iou.cpu().numpy()
    want_best = np.nan_to_num(np.nanmax(np.where(np.isnan(g["ref_iou"]), -1.0, g["ref_iou"]), 1).clip(0.0))
    assert np.array_equal(gidx, g["ref_gt_idx"]) and (np.abs(best - want_best) <= IOU_BAR).all()
    assert np.array_equal(src.both[0].cpu().numpy(), ref["seg_cnt"]) and np.array_equal(src.both[1].cpu().numpy(), ref["seg_pos"])
    o = {"pred_box3d": src.pred_box3d[:U].cpu().numpy().reshape(U, 8, 3), "pred_angle": src.pred_angle[:U].cpu().numpy(),
         "pred_size": src.pred_size[:U].cpu().numpy(), "box3d": src.box3d[:U].cpu().numpy().reshape(U, 8, 3),
         "heading": src.heading[:U].cpu().numpy(), "size": src.size[:U].cpu().numpy()}
    _check_boxes(o, ref, g, [u for u in range(U) if sc["cgt"][u // A] >= 0])
    kept = np.nonzero(~g["ref_reject"])[0]
    K = len(kept)
    assert K == 12 and int(src.n_kept.cpu()[0]) == K and np.array_equal(src.slot_unit.cpu().numpy()[:K], kept)
    counts = ref["counts"][kept]
    off = src.off.cpu().numpy()
    assert np.array_equal(off[:K], np.concatenate([[0], np.cumsum(counts)])[:K]) and off[U] == counts.sum()
    assert np.array_equal(src.counts.cpu().numpy()[:K], counts)
    pts_h = src.points.cpu().numpy()
    assert np.array_equal(_bits(pts_h[:counts.sum()]), _bits(_rows(sc, kept))) and not pts_h[counts.sum():].any()
    classes = src.builder.classes
    types = _table(sc)[2]
    assert got["size_class"].cpu().numpy()[:K, 0].tolist() == [classes.index(types[u // A]) for u in kept]
    assert np.array_equal(src.t["psize"].cpu().numpy()[:K], o["pred_size"][kept])
    with pytest.raises(ValueError, match="bit 1"):                         # K < B: said, not silent
        src.check()
    assert [int(x.state.cpu()[0]) for x in (src.draws_pick, src.draws_jitter, src.draws_sample)] == [1, 1, 1]
    # jitter=False: one un-jittered copy per candidate, the rows of the A = 1 labelled selection
    src1 = _source(sc, 8, Ax=1, pick=False, jitter=False)
    src1.step()
    torch.cuda.synchronize()
    rc, o1 = _label_count(_tensors(sc), sc["S"], jitter=False)
    assert rc == 0 and np.array_equal(src1.both[0].cpu().numpy(), o1["scnt"]) and src1.jitter is None
    assert np.array_equal(src1.pred_size[:8].cpu().numpy()[sc["cgt"] >= 0], o1["pred_size"][sc["cgt"] >= 0])


def _snapshot(batch):
    return {k: v.cpu().clone() for k, v in batch.items()}


def test_captured_step_replays_fresh_batches_equal_to_eager_steps():
    sc = _scene(4)
    src, eager = _source(sc, 8), _source(sc, 8)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        src.step()                                                          # warm-up on a side stream: step 0
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step()
    torch.cuda.synchronize()
    states = lambda s: [int(x.state.cpu()[0]) for x in (s.draws_pick, s.draws_jitter, s.draws_sample)]
    assert states(src) == [1, 1, 1]                                         # capturing runs nothing
    eager.step()
    seen = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(out)
        want = _snapshot(eager.step())
        assert states(src) == [2 + r] * 3 == states(eager)
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
        assert torch.equal(src.jitter.cpu(), eager.jitter.cpu()) and torch.equal(src.slot_unit.cpu(), eager.slot_unit.cpu())
        assert torch.equal(src.cand_row.cpu(), eager.cand_row.cpu()) and torch.equal(src.gt_idx.cpu(), eager.gt_idx.cpu())
        seen.append(got)
    assert not torch.equal(seen[0]["point_cloud"], seen[1]["point_cloud"]) and not torch.equal(seen[1]["point_cloud"], seen[2]["point_cloud"])
    assert states(src) == [1 + 3] * 3


def test_overflow_is_truncated_flagged_and_stays_in_bounds():
    """The point buffer is replaced by a view into a poisoned one: capacity + 1 rows between guard rows."""
    sc = _scene(4)
    kept = np.nonzero(~sc["g"]["ref_reject"])[0][:6]
    want = _rows(sc, kept)
    cap = len(want) - 37
    assert cap > 100
    src = _source(sc, 6, capacity=cap, pick=False, jitter=sc["jit"])
    buf = torch.full((cap + 1 + 8, 4), -7.0, dtype=torch.float32, device="cuda")
    buf[4:cap + 5] = 0.0
    src.points = buf[4:cap + 5]
    src.t["raw"] = src.points
    got = src.step()
    torch.cuda.synchronize()
    off, counts = src.off.cpu().numpy(), src.counts.cpu().numpy()
    h = buf.cpu().numpy()
    assert (h[:4] == -7.0).all() and (h[cap + 5:] == -7.0).all() and not h[cap + 4].any()       # guards intact, the spare row never written
    assert off[-1] == cap and int(src.seg_off.cpu()[-1]) == cap and counts.sum() == cap and (off[:6] + counts <= cap).all()
    assert np.array_equal(src.slot_unit.cpu().numpy(), kept) and np.array_equal(_bits(h[4:cap + 4]), _bits(want[:cap]))
    with pytest.raises(ValueError, match="bit 2"):
        src.check()
    assert all(torch.isfinite(v).all() for v in got.values() if v.dtype.is_floating_point)


def test_one_training_step_on_a_step_batch():
    """The hash-initialised refine_b4_n512 model on a step() batch: finite losses and gradients."""
    from helpers import load_golden
    from test_gpu_model import _model
    from frustum_convnet_amd import inputs
    g2 = load_golden("refine_b4_n512")
    m = _model(g2).train()                                                  # (cfg now holds the refine strides: the builder reads them)
    b = inputs.RefineInputBuilder(int(g2["meta_npoint"]), random_flip=True, random_shift=True)
    src = _source(_scene(4), 6, builder=b)
    batch = {k: v for k, v in src.step().items() if k != "lens"}
    losses, _ = m(batch)
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    src.check()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    print({k: float(v.detach()) for k, v in losses.items()})
    assert all(torch.isfinite(v).all() for v in losses.values()) and float(losses["total_loss"].detach()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    from frustum_convnet_amd import cascade
    sc = _scene(4)
    dets, dframe, types = _table(sc)
    _source(sc, 4)
    hi, neg = dframe.copy(), dframe.copy()
    hi[0], neg[7] = 3, -1
    for kw in (dict(off=np.asarray([0, 9000, 700])), dict(off=np.asarray([0])), dict(off=np.asarray([0, 700, 700, 10 ** 6])),
               dict(dets=dets), dict(dets=_dev(dets).double()), dict(dets=_dev(dets)[:, :7]), dict(dets=_dev(np.zeros((16, 8), np.float32))[::2]),
               dict(det_frame=hi), dict(det_frame=neg), dict(det_frame=dframe[:7]), dict(det_frame=dframe.astype(np.float64)),
               dict(det_types=types[:7]), dict(det_types=["Tram"] + types[1:]),
               dict(goff=sc["goff"][:3]), dict(goff=np.asarray([0, 3, 2, 7])), dict(goff=np.asarray([0, 3, 3, 8])), dict(gt=sc["gt"][:0], goff=np.zeros(4, np.int64)),
               dict(B=0), dict(B=25), dict(D=9), dict(D=0), dict(Ax=0), dict(Ax=65), dict(D=8, Ax=64 * 5),
               dict(capacity=0), dict(lpad=(64, 32, 16)), dict(lpad=(64, 32, 16, 0)), dict(shift_ratio=1.0), dict(shift_ratio=-0.1), dict(ratio=0.0),
               dict(jitter=False), dict(jitter=sc["jit"][:7]), dict(jitter=sc["jit"][:, :2])):
        kw = dict(kw)
        B = kw.pop("B", 4)
        with pytest.raises(ValueError):
            _source(sc, B, **kw)
    _source(sc, 8, Ax=1, jitter=False)
    with pytest.raises(ValueError):                                         # D * A beyond the plan's units
        cascade.RefineTrainSource(_dev(sc["pts"]), sc["off"], _dev(np.tile(dets, (100, 1))), np.tile(dframe, 100), types * 100, sc["gt"],
                                  sc["goff"], _builder(64), 4, 700, 3, 100, BIG, 1)
    with pytest.raises(ValueError):                                         # D * A * S beyond the plan's segments
        cascade.RefineTrainSource(torch.zeros((4096 * 40, 4), dtype=torch.float32, device="cuda"), [0, 4096 * 40],
                                  _dev(np.tile(dets, (256, 1))), np.zeros(2048, np.int32), ["Car"] * 2048, sc["gt"], [0, 7],
                                  _builder(64), 4, 2048, 1, 100, BIG, 1, jitter=False)
    assert cascade.RefineTrainSource.limits() == (2048, 65536)


def test_entry_refusals_write_nothing():
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    # ---- the jitter draw
    out, obuf = _guarded((5, 3, 7), torch.float64, -7.0)
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    good = [5, 3, 9, _p(state), 1, _p(out), s]
    for i, v, rc in ((3, None, BADARG), (5, None, BADARG), (0, -1, BADARG), (1, 0, BADARG), (1, 65, BADARG), (1, -1, BADARG),
                     (0, 21846, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_box3d_jitter_draw(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and int(state.cpu()[0]) == 0
    assert L.fcn_box3d_jitter_draw(*good) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != -7.0).all() and int(state.cpu()[0]) == 1 and _intact(obuf, -7.0)
    before = out.cpu().clone()
    zero = list(good)
    zero[0] = 0                                                             # no unit: only the counter moves
    assert L.fcn_box3d_jitter_draw(*zero) == 0
    torch.cuda.synchronize()
    assert int(state.cpu()[0]) == 2 and torch.equal(out.cpu(), before)
    # ---- the plan
    cnt, pos, psz = _counts()
    U, S, B = 12, 3, 4
    o = {k: torch.full(shape(U, S, B), -7, dtype=dt, device="cuda") for k, dt, shape in PLAN_OUT}
    o["status"] = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)), _dev(psz))
    st4, lp4 = (ctypes.c_double * 4)(*STRIDES), (ctypes.c_int32 * 4)(*BIG)
    good = [_p(ins[0]), _p(ins[1]), _p(ins[2]), st4, lp4, U, S, B, 10000] + [_p(o[k]) for k in ("slot_unit", "n_kept", "seg_off", "off", "counts", "status")] + [s]
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14):
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_train_plan(*bad) == BADARG, i
    for i, v, rc in ((5, -1, BADARG), (6, 0, BADARG), (7, 0, BADARG), (8, -1, BADARG), (5, 2049, LIMIT), (7, 2049, LIMIT), (6, 5462, LIMIT),
                     (4, (ctypes.c_int32 * 4)(64, 0, 16, 8), BADARG), (4, (ctypes.c_int32 * 4)(64, 32, 16, -1), BADARG),
                     (3, (ctypes.c_double * 4)(0.1, 0.2, 0.0, 0.8), BADARG), (3, (ctypes.c_double * 4)(0.1, float("nan"), 0.4, 0.8), BADARG),
                     (3, (ctypes.c_double * 4)(-0.1, 0.2, 0.4, 0.8), BADARG)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_refine_train_plan(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o.values())
    assert L.fcn_refine_train_plan(*good) == 0 and L.fcn_refine_train_plan_limits(None, None) == BADARG
    torch.cuda.synchronize()
    assert int(o["n_kept"].cpu()[0]) == 4
    # ---- the no-read match, count and fill: the reading entries' argument refusals
    sc = _scene(3)
    S = sc["S"]
    t = _tensors(sc)
    w = _outputs(t["crow"].numel() * A, S)
    good = _common(t, S) + [_p(w[k]) for k in OUT_ORDER] + [s]
    for i in (0, 1, 4, 6, 7, 10, 11, 14, 17, 18, 19, 20, 21, 22, 23, 24):
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_train_count(*bad) == BADARG, i
    for i, v in ((3, 2), (16, 0), (16, -1), (13, 0), (13, 65), (13, -1), (8, -1), (2, -1), (5, -1), (12, -1), (8, 21846)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_refine_train_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((w[k].cpu().numpy() == -7).all() for k in w)
    soff = torch.zeros(t["crow"].numel() * A * S + 1, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    goodf = good[:17] + [_p(soff), _p(out), s]
    for i in (0, 1, 4, 6, 7, 10, 11, 14, 17, 18):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_refine_train_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (16, 0), (13, 0), (13, 65), (8, -1), (2, -1), (8, 21846)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_refine_train_fill(*bad) == BADARG, (i, v)
    assert L.fcn_refine_train_fill(*goodf) == 0                             # (every slice empty: nothing to write)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    gidx = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    best = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    goodm = [_p(t["dets"]), 10, _p(t["crow"]), _p(t["cframe"]), 8, _p(t["gt"]), 7, _p(t["goff"]), 3, 0.5, _p(gidx), _p(best), s]
    for i in (0, 2, 3, 5, 7, 10, 11):
        bad = list(goodm)
        bad[i] = None
        assert L.fcn_refine_train_match(*bad) == BADARG, i
    for i in (1, 4, 6, 8):
        bad = list(goodm)
        bad[i] = -1
        assert L.fcn_refine_train_match(*bad) == BADARG, i
    torch.cuda.synchronize()
    assert (gidx.cpu().numpy() == -7).all() and (best.cpu().numpy() == -7.0).all()


def test_check_raises_names_the_bits_and_clears():
    sc = _scene(4)
    src = _source(sc, 4)
    src.check()
    src.status.fill_(R.ST_WIDE | R.ST_TRUNC)
    with pytest.raises(ValueError) as e:
        src.check()
    assert "bit 5" in str(e.value) and "bit 2" in str(e.value) and not any("bit %d" % i in str(e.value) for i in (0, 1, 6))
    src.check()
    src.status.fill_(R.ST_WIDTH)
    with pytest.raises(ValueError, match="bit 6"):
        src.check()
    src.draws_sample.status.fill_(1)
    with pytest.raises(ValueError, match="bit 0"):
        src.check()
    assert int(src.draws_sample.status.cpu()[0]) == 0
    src.check()
    # a width the fixed window counts cannot hold: the unit is dropped and bit 5 says so
    tight = _source(sc, 4, lpad=(8, 4, 2, 1), pick=False, jitter=sc["jit"])
    tight.step()
    with pytest.raises(ValueError, match="bit 5"):
        tight.check()
